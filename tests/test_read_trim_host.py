"""CPU: the trimming contract (rcorrector_amd/csrc/rc_trim.h, what k_read_trim runs per unit) as a host program against
tests/trim_model.py -- tests/hostmath/read_trim.cpp runs the word and lane arithmetic one lane after another over the batches
of tests/trim_cases.py and prints every read's row and every unit's outcome.  Built and run twice: plain, and with
AddressSanitizer + UndefinedBehaviorSanitizer, directly, nothing preloaded.  Then the feature's public surface -- the header as
C, the struct sizes, ABI_SYMBOLS, the binding -- and the usage errors of tools/read_trim, which need no GPU."""
import ctypes
import importlib.machinery
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import trim_cases as tc
import trim_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "read_trim")
FX = os.path.join(ROOT, "tests", "golden", "fx_pe_k23")
LEFT, RIGHT = os.path.join(FX, "reads_1.fq"), os.path.join(FX, "reads_2.fq")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_the_header_equals_the_model_line_by_line(flags, tmp_path):
    exe = str(tmp_path / "read_trim")
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I", os.path.join(ROOT, "rcorrector_amd", "csrc"),
                                                             os.path.join(ROOT, "tests", "hostmath", "read_trim.cpp"), "-o", exe], check=True)
    seen_cuts = set()
    for i, s in enumerate(tc.all_scenarios()):
        p, mates = s["p"], 1 if s["mode"] == 0 else 2
        units = tm.units_of(len(s["seqs"]), s["mode"])
        path = tmp_path / ("units_%d.txt" % i)
        with open(path, "wb") as f:
            for rds in units:
                for r in rds:
                    f.write(b"=" + s["seqs"][r] + b"\n" + (b"-" if s["quals"] is None else b"=" + s["quals"][r]) + b"\n")
        nw = 8 if s["max_read_len"] <= 256 else 32
        args = [exe, str(path), str(nw), str(mates), str(p["qual_min"]), str(p["qual_base"]), p["adapter1"].decode() or "-", p["adapter2"].decode() or "-",
                str(p["adapter_min"]), str(p["adapter_mm_pct"]), str(int(p["pair_overlap"])), str(p["pair_min_overlap"]), str(p["pair_mm_pct"]), str(p["min_len"])]
        r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)   # (run directly: nothing preloaded)
        lines = r.stdout.decode(errors="replace").splitlines()
        assert r.returncode == 0, "\n".join(lines[-5:])
        rows, keep, tally = tc.expected(i)
        want = []
        ovl = 0
        for u, rds in enumerate(units):
            want += ["%d %d %d %d" % tuple(rows[r]) for r in rds]
            o = int(tm.trim_unit([s["seqs"][r] for r in rds], None, dict(p, qual_min=0, adapter1=b"", adapter2=b""), tc.lmax_of(s["max_read_len"]))[2])
            ovl += o
            want.append("unit %d %d" % (keep[u], o))
        assert ovl == tally["pairs_overlapping"]
        assert lines == want, "%s: first difference at line %d" % (s["name"], next(n for n, (a, b) in enumerate(zip(lines + [None], want + [None])) if a != b))
        for row, sq in zip(rows, s["seqs"]):
            L = min(len(sq), tc.lmax_of(s["max_read_len"]))
            seen_cuts |= {(c, "cut" if row[1 + c] < L else "none") for c in range(3)} | ({"keep 0"} if row[0] == 0 and L else set())
    # the batches still cover what they were written for
    assert seen_cuts == {(c, w) for c in range(3) for w in ("cut", "none")} | {"keep 0"}


def test_the_batches_hit_the_edges_they_are_named_for():
    S = {s["name"]: i for i, s in enumerate(tc.all_scenarios())}
    rows = tc.expected(S["pair offsets interleaved"])[0]
    # (d* < 0, = 0, > 0 with F below, at and above La; mate 2 running through; no overlap; unrelated; short fragment; wide; full length; 29 / 30)
    assert rows[:, 3].tolist() == [60, 60, 80, 80, 100, 80, 100, 80, 90, 90, 150, 150, 100, 77, 40, 40, 300, 257, 1023, 1023, 60, 60, 30, 30]
    assert tc.expected(S["pair offsets interleaved"])[2]["pairs_overlapping"] == 9
    assert np.array_equal(tc.expected(S["pair offsets in halves"])[0][:12], rows[0::2]) and tc.expected(S["pair offsets, the option off"])[2]["pairs_overlapping"] == 0
    assert tc.expected(S["pair mismatches at and past the share"])[0][:, 3].tolist() == [70, 70, 100, 100, 100, 100, 60, 60]
    assert tc.expected(S["adapter offsets"])[0][:, 2].tolist() == [0, 55, 60, 30, 20, 30, 30, 30, 50, 64, 0, 1]
    for n in (1, 32, 33, 64):
        ad = tc.expected(S["adapter of %d bases" % n])[0][:, 2].tolist()
        assert ad[3:5] == [0, n] and (n == 1 or ad[:3] == [20, 31, 62]) and (n == 1 or ad[5:7] == [250, 300])
    assert tc.expected(S["adapter mismatch share at and past 10 %"])[0][:, 2].tolist() == [40, 60, 40]
    assert tc.expected(S["adapter mismatch share 0 %"])[0][:, 2].tolist() == [60, 60, 40]
    assert tc.expected(S["qualities"])[0][:, 1].tolist() == [60, 0, 50, 60, 60, 59, 60, 17, 1000, 48, 0, 0]
    assert tc.expected(S["qualities, none given"])[0][:, 1].tolist() == tc.expected(S["qualities, qual_min 0"])[0][:, 1].tolist() == [60] * 7 + [317, 1023, 65, 0, 1]
    assert tc.expected(S["min_len at and above keep_len, mode 0"])[1].tolist() == [1, 1, 0, 1, 1, 0, 1, 0]
    assert tc.expected(S["min_len at and above keep_len, mode 1"])[1].tolist() == [1, 0, 0, 0] == tc.expected(S["min_len at and above keep_len, mode 2"])[1].tolist()
    # a wrong max_read_len: the narrow instance looks at 256 bases of a longer mate
    assert tc.expected(S["lengths mode 0 max_read_len 256"])[0][13:15, 3].tolist() == [256, 256]
    assert tc.expected(S["lengths mode 0 max_read_len 257"])[0][13:15, 3].tolist() == [257, 1023]


def test_the_header_parses_as_c_with_the_new_declaration(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "rcorrector_amd.h"\n'
                   "int (*trim)(rc_ctx *, const uint8_t *, const uint8_t *, const uint32_t *, uint32_t, uint64_t, int32_t, int32_t, const rc_trim_params *,\n"
                   "            rc_read_trim *, uint8_t *, rc_trim_tally *) = rc_read_trim_device;\n"
                   "_Static_assert(sizeof(rc_read_trim) == 16, \"16 bytes per read\");\n"
                   "_Static_assert(sizeof(rc_trim_params) == 8 * 4 + 2 * 64 + 2 * 4, \"the parameters\");\n"
                   "_Static_assert(sizeof(rc_trim_tally) == (2 + 6 + 2 + 2 + 3 + 2 * 1024) * 8, \"the tally\");\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    import rcorrector_amd
    from rcorrector_amd import binding as b
    assert "rc_read_trim_device" in rcorrector_amd.ABI_SYMBOLS
    assert callable(getattr(rcorrector_amd.Context, "read_trim_device", None))
    assert b.READ_TRIM_DTYPE.itemsize == 16 and b.READ_TRIM_DTYPE.names == ("keep_len", "cut_qual", "cut_adapter", "cut_pair")
    assert ctypes.sizeof(b._TrimParams) == 168 and b.TRIM_TALLY_DTYPE.itemsize == 2063 * 8 == 8 * b.TRIM_TALLY_WORDS
    assert [n for n, _ in b._TrimParams._fields_] == ["qual_min", "qual_base", "adapter_min", "adapter_mm_pct", "pair_overlap", "pair_min_overlap", "pair_mm_pct",
                                                     "min_len", "adapter1", "adapter2", "adapter1_len", "adapter2_len"]
    assert b.TRIM_TALLY_DTYPE.names == ("reads", "cut_reads", "bases_removed", "short_reads", "units", "units_kept", "pairs_overlapping", "keep_hist")
    p = b.trim_params()
    assert (p.qual_min, p.qual_base, p.adapter_min, p.adapter_mm_pct, p.pair_overlap, p.pair_min_overlap, p.pair_mm_pct, p.min_len) == (20, 33, 5, 10, 1, 30, 10, 20)
    assert bytes(p.adapter1)[:13] == bytes(p.adapter2)[:13] == b"AGATCGGAAGAGC" and p.adapter1_len == p.adapter2_len == 13
    t = b.trim_tally_dict(np.arange(b.TRIM_TALLY_WORDS, dtype=np.uint64))
    assert t["reads"].tolist() == [0, 1] and t["cut_reads"].tolist() == [[2, 3, 4], [5, 6, 7]] and (t["units"], t["units_kept"], t["pairs_overlapping"]) == (12, 13, 14)
    assert t["keep_hist"][1, 1023] == b.TRIM_TALLY_WORDS - 1


def test_the_library_exports_the_entry_point_and_is_built_from_the_new_units():
    import rcorrector_amd
    lib = rcorrector_amd.load_library()
    assert hasattr(lib, "rc_read_trim_device")
    mk = open(os.path.join(ROOT, "rcorrector_amd", "csrc", "Makefile")).read()
    assert " rc_trim.o" in mk and " rc_api_trim.o" in mk and " rc_trim.h" in mk and " rc_overlap_stage.h" in mk
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import build_provenance
    src = build_provenance.snapshot()[0]
    assert {"rcorrector_amd/csrc/rc_trim.h", "rcorrector_amd/csrc/rc_trim.hip", "rcorrector_amd/csrc/rc_api_trim.hip", "rcorrector_amd/csrc/rc_overlap_stage.h"} <= set(src)


# ---- the tool's command line -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    loader = importlib.machinery.SourceFileLoader("read_trim", TOOL)
    spec = importlib.util.spec_from_loader("read_trim", loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


BAD_ARGS = [
    ([], "the reads: give one of"),
    (["-r", LEFT, "-i", RIGHT], "the reads: give one of"),
    (["-p", LEFT], "-p takes files two at a time"),
    (["-p", LEFT, RIGHT, LEFT], "-p takes files two at a time"),
    (["-r", "/nonexistent/reads.fq"], "cannot read /nonexistent/reads.fq"),
    (["-r", LEFT, "-q", "-1"], "-q must be 0..93"),
    (["-r", LEFT, "-q", "94"], "-q must be 0..93"),
    (["-r", LEFT, "-qual-base", "256"], "-qual-base must be 0..255"),
    (["-r", LEFT, "-a", "ACGN"], "-a must be 0..64 bases of upper-case ACGT"),
    (["-r", LEFT, "-a", "acgt"], "-a must be 0..64 bases of upper-case ACGT"),
    (["-r", LEFT, "-a2", "A" * 65], "-a2 must be 0..64 bases of upper-case ACGT"),
    (["-r", LEFT, "-adapter-min", "0"], "-adapter-min must be 1..64"),
    (["-r", LEFT, "-adapter-min", "65"], "-adapter-min must be 1..64"),
    (["-r", LEFT, "-adapter-mm", "51"], "-adapter-mm must be 0..50"),
    (["-p", LEFT, RIGHT, "-overlap-min", "0"], "-overlap-min must be 1..1023"),
    (["-p", LEFT, RIGHT, "-overlap-mm", "-1"], "-overlap-mm must be 0..50"),
    (["-r", LEFT, "-min-len", "1024"], "-min-len must be 0..1023"),
    (["-r", LEFT, "-batch", "0"], "-batch must be at least 1"),
    (["-r", LEFT, os.path.join(FX, "ref", "..", "reads_1.fq")], "two input files would both be written to reads_1.trim.fq"),
    (["-r", LEFT, "-frobnicate", "1"], "unknown option -frobnicate"),
    (["-r", LEFT, "-o"], "-o needs a value"),
    (["-r", LEFT, "-o", "a", "-o", "b"], "-o given twice"),
    (["-r", LEFT, "-q", "x"], "-q needs an integer, got x"),
]


@pytest.mark.parametrize("args,text", BAD_ARGS, ids=["%d %s" % (i, t) for i, (_, t) in enumerate(BAD_ARGS)])
def test_usage_errors(tool, args, text):
    with pytest.raises(tool.UsageError, match=text):
        tool.parse_args(args)


def test_usage_errors_are_one_line_and_exit_status_2():
    for args, text in (BAD_ARGS[0], BAD_ARGS[2], BAD_ARGS[5], BAD_ARGS[8], BAD_ARGS[19]):
        p = subprocess.run([sys.executable, TOOL] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        err = p.stderr.decode()
        assert p.returncode == 2 and p.stdout == b"" and err.count("\n") == 1 and text in err and "usage: read_trim (-r FILE ..." in err


def test_defaults_and_output_names(tool):
    o = tool.parse_args(["-p", LEFT, RIGHT])
    assert (o["q"], o["qual_base"], o["a"], o["a2"], o["adapter_min"], o["adapter_mm"], o["pair_overlap"], o["overlap_min"], o["overlap_mm"], o["min_len"], o["od"]) == \
        (20, 33, b"AGATCGGAAGAGC", b"AGATCGGAAGAGC", 5, 10, True, 30, 10, 20, ".")
    o = tool.parse_args(["-i", LEFT, "-a", "", "-no-pair-overlap", "-a2", "ACGT"])
    assert o["a"] == b"" and o["a2"] == b"ACGT" and o["pair_overlap"] is False
    assert tool.parse_args(["-r", LEFT, "-a", "GATTACA"])["a2"] == b"GATTACA" and tool.parse_args(["-r", LEFT, "-a", ""])["a2"] == b""
    name = tool.output_name
    assert name("/a/b/X.fq") == "X.trim.fq" and name("X.fq.gz") == "X.trim.fq" and name("X.fa") == "X.trim.fa" and name("d/X.fa.gz") == "X.trim.fa"
    assert name("s_1.cor.fq") == "s_1.cor.trim.fq" and name("X.fastq.gz") == "X.trim.fq" and name("reads", fastq=False) == "reads.trim.fa"


def test_cut_record_cuts_the_sequence_and_the_quality_line_and_nothing_else(tool):
    assert tool.cut_record(b"@r1 first\nACGTAC\n+r1\nIIIIII\n", 4) == b"@r1 first\nACGT\n+r1\nIIII\n"
    assert tool.cut_record(b"@r1\nACGTAC\r\n+\nIIIIII\r\n", 6) == b"@r1\nACGTAC\r\n+\nIIIIII\r\n"
    assert tool.cut_record(b"@r1\nACGTAC\r\n+\nIIIIII\r\n", 0) == b"@r1\n\r\n+\n\r\n"
    assert tool.cut_record(b">s1 some words\nACGTAC\n", 2) == b">s1 some words\nAC\n" and tool.cut_record(b">s1\n\n", 0) == b">s1\n\n"
