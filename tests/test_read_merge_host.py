"""CPU: the merging contract (rcorrector_amd/csrc/rc_merge.h, what k_merge_plan and k_merge_write run per unit) as a host program
against tests/merge_model.py -- tests/hostmath/read_merge.cpp runs the word, lane and granule arithmetic one lane after another
over the batches of tests/merge_cases.py and prints every unit's row and its bytes of the output arenas.  Built and run twice:
plain, and with AddressSanitizer + UndefinedBehaviorSanitizer, directly, nothing preloaded.  Then the feature's public surface --
the header as C, the struct sizes, ABI_SYMBOLS, the binding -- and the usage errors of tools/read_merge, which need no GPU."""
import ctypes
import importlib.machinery
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import merge_cases as mc
import merge_model as mm
import trim_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "read_merge")
FX = os.path.join(ROOT, "tests", "golden", "fx_pe_k23")
LEFT, RIGHT = os.path.join(FX, "reads_1.fq"), os.path.join(FX, "reads_2.fq")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_the_header_equals_the_model_line_by_line(flags, tmp_path):
    exe = str(tmp_path / "read_merge")
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I", os.path.join(ROOT, "rcorrector_amd", "csrc"),
                                                             os.path.join(ROOT, "tests", "hostmath", "read_merge.cpp"), "-o", exe], check=True)
    for i, s in enumerate(mc.all_scenarios()):
        p = s["p"]
        units = tm.units_of(len(s["seqs"]), s["mode"])
        path = tmp_path / ("units_%d.txt" % i)
        with open(path, "wb") as f:
            for rds in units:
                for r in rds:
                    f.write(b"=" + s["seqs"][r] + b"\n" + (b"-" if s["quals"] is None else b"=" + s["quals"][r]) + b"\n")
        nw = 8 if s["max_read_len"] <= 256 else 32
        args = [exe, str(path), str(nw), str(p["min_overlap"]), str(p["max_mismatch_pct"]), str(p["qual_base"]), str(p["qual_cap"])]
        r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)   # (run directly: nothing preloaded)
        lines = r.stdout.decode(errors="replace").splitlines()
        assert r.returncode == 0, "\n".join(lines[-5:])
        rows, moff, mseq, mqual, t = mc.expected(i)
        want = []
        for u in range(len(units)):
            want.append("row %d %d %d %d" % tuple(rows[u]))
            want.append("seq " + mseq[moff[u]:moff[u + 1]].hex())
            want.append("qual " + (mqual[moff[u]:moff[u + 1]].hex() if mqual is not None else "-"))
        want += ["took %d %d %d" % (t["took_mate1"], t["took_mate2"], t["ties"]), "tail clean"]
        assert lines == want, "%s: first difference at line %d" % (s["name"], next(n for n, (a, b) in enumerate(zip(lines + [None], want + [None])) if a != b))


def test_the_batches_hit_the_edges_they_are_named_for():
    S = {s["name"]: i for i, s in enumerate(mc.all_scenarios())}
    for i in S.values():
        mc.expected(i)                  # (asserts the lengths, the winners and the read-through count each batch names)
    rows, moff, mseq, mqual, t = mc.expected(S["offsets mode 2"])
    assert rows[:, 1].tolist() == [-20, 0, 30, 20, 50, 20, -30, 0, 0, 0, 0, 0, 30, 0] and (t["merged"], t["unmerged"]) == (8, 6) and t["len_hist"][0] == 6
    assert moff[-1] == len(mseq) == len(mqual) == sum(rows[:, 0]) + 14 and mseq.count(b"\0") == 14
    h = mc.expected(S["offsets mode 1"])
    assert np.array_equal(h[0], rows) and np.array_equal(h[1], moff) and h[2] == mseq and mm.tally_equal(h[4], t)      # (the modes: one merged arena)
    assert h[3] != mqual                                                                                             # (... of other random qualities)
    assert mc.expected(S["offsets without qualities"])[2] == mseq and mc.expected(S["offsets without qualities"])[3] is None
    rows = mc.expected(S["two mates of 1023 bases overlapping by min_overlap"])[0]
    assert rows[0].tolist() == [2016, 993, 30, 0]
    # the narrow instance looks at 256 bases of a longer mate: another offset, the same fragment
    assert mc.expected(S["a mate of 300 bases under max_read_len 256: the narrow instance's cut"])[0][0].tolist() == [400, 144, 112, 0]
    assert mc.expected(S["a mate of 300 bases under max_read_len 300"])[0][0].tolist() == [400, 100, 200, 0]
    q = mc.expected(S["agreement below, at and above qual_cap"])[3]
    assert q[40:80] == bytes([33 + 40] * 10 + [33 + 41] * 20 + [33 + 20] * 10) and q[:40] == bytes([33 + 20]) * 40 and q[80:120] == bytes([33 + 30]) * 40
    q = mc.expected(S["agreement, qual_cap 93 and phred 64"])[3]
    assert q[40:80] == bytes([64 + 40] * 10 + [64 + 41] * 10 + [64 + 42] * 10 + [64 + 20] * 10)
    rows, _, s, q, t = mc.expected(S["disagreements: mate 1 wins, mate 2 wins, a tie, the floor of 2"])
    a = mc.all_scenarios()[S["disagreements: mate 1 wins, mate 2 wins, a tie, the floor of 2"]]["seqs"][0]
    assert [s[i] == a[i] for i in (45, 55, 65, 75, 85)] == [True, False, True, True, False]
    assert [q[i] - 33 for i in (45, 55, 65, 75, 85)] == [25, 25, 2, 2, 40] and q[50] == 33 + 30 and q[52] == 33 + 30 and rows[0].tolist() == [140, 40, 60, 5]
    rows, _, s, q, t = mc.expected(S["N against a base, N against N, lower case"])
    sc = mc.all_scenarios()[S["N against a base, N against N, lower case"]]
    a, qa = sc["seqs"][0], sc["quals"][0]
    assert rows[0].tolist() == [140, 40, 60 - 8, 0] and s[70:71] == b"N" and q[70] == qa[70] and s[50:51] in b"ACGT" and s[60] == a[60] and q[60] == qa[60]
    assert s[80:83] == a[80:83].upper() and s[85:87] == a[85:87] and s[5:6] == b"n" and s[135:136] == b"-"


def test_the_header_parses_as_c_with_the_new_declaration(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "rcorrector_amd.h"\n'
                   "int (*merge)(rc_ctx *, const uint8_t *, const uint8_t *, const uint32_t *, uint32_t, uint64_t, int32_t, int32_t, const rc_merge_params *,\n"
                   "             rc_read_merge *, uint8_t *, uint8_t *, uint32_t *, uint64_t, rc_merge_tally *) = rc_read_merge_device;\n"
                   "_Static_assert(sizeof(rc_read_merge) == 16, \"16 bytes per unit\");\n"
                   "_Static_assert(sizeof(rc_merge_params) == 16, \"the parameters\");\n"
                   "_Static_assert(sizeof(rc_merge_tally) == (9 + 2048) * 8, \"the tally\");\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    import rcorrector_amd
    from rcorrector_amd import binding as b
    assert "rc_read_merge_device" in rcorrector_amd.ABI_SYMBOLS
    assert callable(getattr(rcorrector_amd.Context, "read_merge_device", None))
    assert b.READ_MERGE_DTYPE.itemsize == 16 and b.READ_MERGE_DTYPE.names == ("merged_len", "d", "v", "m")
    assert ctypes.sizeof(b._MergeParams) == 16 and b.MERGE_TALLY_DTYPE.itemsize == 2057 * 8 == 8 * b.MERGE_TALLY_WORDS
    assert [n for n, _ in b._MergeParams._fields_] == ["min_overlap", "max_mismatch_pct", "qual_base", "qual_cap"]
    assert b.MERGE_TALLY_DTYPE.names == mm.TALLY_KEYS
    p = b.merge_params()
    assert (p.min_overlap, p.max_mismatch_pct, p.qual_base, p.qual_cap) == (30, 10, 33, 41) == tuple(mm.DEFAULTS[k] for k in ("min_overlap", "max_mismatch_pct", "qual_base", "qual_cap"))
    t = b.merge_tally_dict(np.arange(b.MERGE_TALLY_WORDS, dtype=np.uint64))
    assert [t[k] for k in mm.TALLY_KEYS[:9]] == list(range(9)) and t["len_hist"][0] == 9 and t["len_hist"][2047] == b.MERGE_TALLY_WORDS - 1
    with pytest.raises(ValueError, match="2057 64-bit words"):
        b.merge_tally_dict(np.zeros(5, np.uint64))


def test_the_library_exports_the_entry_point_and_is_built_from_the_new_units():
    import rcorrector_amd
    lib = rcorrector_amd.load_library()
    assert hasattr(lib, "rc_read_merge_device")
    mk = open(os.path.join(ROOT, "rcorrector_amd", "csrc", "Makefile")).read()
    assert " rc_merge.o" in mk and " rc_api_merge.o" in mk and " rc_merge.h" in mk
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import build_provenance
    src = build_provenance.snapshot()[0]
    assert {"rcorrector_amd/csrc/rc_merge.h", "rcorrector_amd/csrc/rc_merge.hip", "rcorrector_amd/csrc/rc_api_merge.hip"} <= set(src)


# ---- the tool's command line -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    loader = importlib.machinery.SourceFileLoader("read_merge", TOOL)
    spec = importlib.util.spec_from_loader("read_merge", loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


BAD_ARGS = [
    ([], "the reads: give one of"),
    (["-p", LEFT, RIGHT, "-i", RIGHT], "the reads: give one of"),
    (["-r", LEFT], "-r: single reads have no mate to merge with"),
    (["-p", LEFT], "-p takes files two at a time"),
    (["-p", LEFT, RIGHT, LEFT], "-p takes files two at a time"),
    (["-i", "/nonexistent/reads.fq"], "cannot read /nonexistent/reads.fq"),
    (["-p", LEFT, RIGHT, "-overlap-min", "0"], "-overlap-min must be 1..1023"),
    (["-p", LEFT, RIGHT, "-overlap-min", "1024"], "-overlap-min must be 1..1023"),
    (["-p", LEFT, RIGHT, "-overlap-mm", "-1"], "-overlap-mm must be 0..50"),
    (["-p", LEFT, RIGHT, "-overlap-mm", "51"], "-overlap-mm must be 0..50"),
    (["-i", LEFT, "-qual-base", "125"], "-qual-base must be 0..124"),
    (["-i", LEFT, "-qual-cap", "1"], "-qual-cap must be 2..93"),
    (["-i", LEFT, "-qual-cap", "94"], "-qual-cap must be 2..93"),
    (["-i", LEFT, "-qual-base", "64", "-qual-cap", "63"], "-qual-base \\+ -qual-cap must be at most 126"),
    (["-i", LEFT, "-batch", "0"], "-batch must be at least 1"),
    (["-i", LEFT, os.path.join(FX, "ref", "..", "reads_1.fq")], "two input files would both be written to reads_1.unmerged.fq"),
    (["-i", LEFT, "-frobnicate", "1"], "unknown option -frobnicate"),
    (["-i", LEFT, "-o"], "-o needs a value"),
    (["-i", LEFT, "-o", "a", "-o", "b"], "-o given twice"),
    (["-i", LEFT, "-qual-cap", "x"], "-qual-cap needs an integer, got x"),
]


@pytest.mark.parametrize("args,text", BAD_ARGS, ids=["%d %s" % (i, t) for i, (_, t) in enumerate(BAD_ARGS)])
def test_usage_errors(tool, args, text):
    with pytest.raises(tool.UsageError, match=text):
        tool.parse_args(args)


def test_usage_errors_are_one_line_and_exit_status_2():
    for args, text in (BAD_ARGS[0], BAD_ARGS[2], BAD_ARGS[3], BAD_ARGS[6], BAD_ARGS[16]):
        p = subprocess.run([sys.executable, TOOL] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        err = p.stderr.decode()
        assert p.returncode == 2 and p.stdout == b"" and err.count("\n") == 1 and text in err and "usage: read_merge (-p LEFT RIGHT ..." in err


def test_defaults_output_names_and_the_merged_record(tool):
    o = tool.parse_args(["-p", LEFT, RIGHT])
    assert (o["overlap_min"], o["overlap_mm"], o["qual_base"], o["qual_cap"], o["batch"], o["od"], o["out"], o["list"]) == (30, 10, 33, 41, 1 << 19, ".", None, None)
    o = tool.parse_args(["-i", LEFT, RIGHT, "-qual-base", "64", "-qual-cap", "62", "-od", "d"])
    assert o["i"] == [LEFT, RIGHT] and (o["qual_base"], o["qual_cap"], o["od"]) == (64, 62, "d")
    name = tool.output_name
    assert name("/a/b/X.fq", "merged") == "X.merged.fq" and name("X.fq.gz", "unmerged") == "X.unmerged.fq" and name("X.fa", "merged") == "X.merged.fa"
    assert name("s_1.cor.fq", "merged") == "s_1.cor.merged.fq" and name("X.fastq.gz", "merged") == "X.merged.fq" and name("reads", "unmerged", fastq=False) == "reads.unmerged.fa"
    assert tool.merged_record(b"@r1/1 first\r\nACGT\r\n+r1\nIIII\n", b"ACGTAC", b"IIJJII") == b"@r1/1 first\r\nACGTAC\n+\nIIJJII\n"
    assert tool.merged_record(b">s1 some words\nACGT\n", b"ACGTAC", None) == b">s1 some words\nACGTAC\n"
