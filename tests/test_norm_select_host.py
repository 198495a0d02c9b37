"""CPU: the normalisation contract (rcorrector_amd/csrc/rc_norm.h, what k_norm_select runs per unit) as a host program against
tests/norm_model.py -- tests/hostmath/norm_select.cpp prints what the header makes of a vector set: D of 0, 1, min_cov - 1,
min_cov, target, target + 1 and 2^31 - 1, targets of 1 and 2^31 - 1, indices of 2^32 and above, mates with and without valid
windows in all four combinations, m1 + m2 + 1 = 2^32 - 1, bins on both sides of max_bin, and 2000 seeded random vectors.
Built and run twice: plain, and with AddressSanitizer + UndefinedBehaviorSanitizer, directly, nothing preloaded.  Then the
feature's public surface -- the header as C, ABI_SYMBOLS, the binding, the timer list -- and the usage errors of
tools/read_normalize, which need no GPU."""
import importlib.machinery
import importlib.util
import os
import subprocess
import sys

import pytest

import norm_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "read_normalize")
FX = os.path.join(ROOT, "tests", "golden", "fx_pe_k23")
LEFT, RIGHT, DUMP = os.path.join(FX, "reads_1.fq"), os.path.join(FX, "reads_2.fq"), os.path.join(FX, "dump.jf")
TOP = (1 << 31) - 1


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_the_header_equals_the_model_line_by_line(flags, tmp_path):
    exe = str(tmp_path / "norm_select")
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I", os.path.join(ROOT, "rcorrector_amd", "csrc"),
                                                             os.path.join(ROOT, "tests", "hostmath", "norm_select.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)   # (run directly: nothing preloaded)
    lines = p.stdout.decode().splitlines()
    assert p.returncode == 0 and lines[-1] == "ok %d" % (len(lines) - 1), "\n".join(lines[-5:])
    seen = {"D": set(), "valid": set(), "target": set(), "outcome": set(), "bin_side": set()}
    big_index = wrap = 0
    for ln in lines[:-1]:
        given, got = ln.split(" : ")
        v1, m1, v2, m2, index, seed, target, min_cov, max_bin = (int(x) for x in given.split())
        has, depth, r, outcome, bin_ = (int(x) for x in got.split())
        d = nm.unit_depth([(v1, 0, m1, 0), (v2, 0, m2, 0)])
        want = (int(d is not None), d or 0, nm.draw(seed, index), nm.outcome(d, nm.draw(seed, index), target, min_cov), min(d or 0, max_bin))
        assert (has, depth, r, outcome, bin_) == want, ln
        seen["valid"].add((v1 > 0, v2 > 0))
        seen["target"].add(target)
        seen["outcome"].add(outcome)
        big_index += index >= 1 << 32
        wrap += v1 > 0 and v2 > 0 and m1 + m2 + 1 == (1 << 32) - 1
        if d is not None:
            seen["bin_side"].add((d > max_bin) - (d < max_bin))
            for what, x in (("0", 0), ("1", 1), ("min_cov-1", min_cov - 1), ("min_cov", min_cov), ("target", target), ("target+1", target + 1), ("top", TOP)):
                if d == x:
                    seen["D"].add(what)
    # the vector set still covers what it was written for
    assert seen["D"] == {"0", "1", "min_cov-1", "min_cov", "target", "target+1", "top"}
    assert seen["valid"] == {(False, False), (False, True), (True, False), (True, True)} and {1, TOP} <= seen["target"]
    assert seen["outcome"] == {nm.OVER, nm.KEPT, nm.LOW, nm.NOVALID} and seen["bin_side"] == {-1, 0, 1} and big_index > 100 and wrap >= 1


def test_the_header_parses_as_c_with_the_new_declaration(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "rcorrector_amd.h"\n'
                   "int (*sel)(rc_ctx *, const rc_read_depth *, uint32_t, int, uint64_t, uint32_t, uint32_t, uint64_t, uint32_t, uint8_t *, uint64_t *)\n"
                   "    = rc_norm_select_device;\n"
                   "_Static_assert(RC_NORM_OVER == 0 && RC_NORM_KEPT == 1 && RC_NORM_LOW == 2 && RC_NORM_NOVALID == 3, \"outcome values\");\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    import rcorrector_amd
    assert "rc_norm_select_device" in rcorrector_amd.ABI_SYMBOLS
    assert callable(getattr(rcorrector_amd.Context, "norm_select_device", None))
    h = open(os.path.join(ROOT, "include", "rcorrector_amd.h")).read()
    assert "9 = normalisation's unit selection" in h        # the kernel-timer index follows the last one the header listed
    assert "7 = per-read k-mer depth, 8 = per-read screen against a second k-mer set" in h       # the earlier entries as they were
    # the contract's constants are the same in the two headers
    c = open(os.path.join(ROOT, "rcorrector_amd", "csrc", "rc_norm.h")).read()
    for name, value in (("OVER", nm.OVER), ("KEPT", nm.KEPT), ("LOW", nm.LOW), ("NOVALID", nm.NOVALID)):
        assert "#define RC_NORM_%s %d\n" % (name, value) in h and "#define RC_NORM_%s %d\n" % (name, value) in c


def test_the_library_exports_the_entry_point_and_is_built_from_the_new_units():
    import rcorrector_amd
    lib = rcorrector_amd.load_library()
    assert hasattr(lib, "rc_norm_select_device")
    mk = open(os.path.join(ROOT, "rcorrector_amd", "csrc", "Makefile")).read()
    assert " rc_norm.o" in mk and " rc_api_norm.o" in mk and " rc_norm.h" in mk
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import build_provenance
    src = build_provenance.snapshot()[0]
    assert {"rcorrector_amd/csrc/rc_norm.h", "rcorrector_amd/csrc/rc_norm.hip", "rcorrector_amd/csrc/rc_api_norm.hip"} <= set(src)


# ---- the tool's command line -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    loader = importlib.machinery.SourceFileLoader("read_normalize", TOOL)
    spec = importlib.util.spec_from_loader("read_normalize", loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


BASE = ["-k", "23", "-target", "30"]
BAD_ARGS = [
    ([], "-k is required"),
    (["-k", "40", "-target", "30", "-r", LEFT], "-k must be 1..32"),
    (["-k", "23", "-r", LEFT], "-target is required"),
    (["-k", "23", "-target", "0", "-r", LEFT], "-target must be 1..2147483647"),
    (["-k", "23", "-target", str(1 << 31), "-r", LEFT], "-target must be 1..2147483647"),
    (BASE, "the reads: give one of"),
    (BASE + ["-r", LEFT, "-i", RIGHT], "the reads: give one of"),
    (BASE + ["-p", LEFT], "-p takes files two at a time"),
    (BASE + ["-p", LEFT, RIGHT, LEFT], "-p takes files two at a time"),
    (BASE + ["-r", "/nonexistent/reads.fq"], "cannot read /nonexistent/reads.fq"),
    (BASE + ["-r", LEFT, "-c", "/nonexistent/dump.jf"], "cannot read /nonexistent/dump.jf"),
    (BASE + ["-r", LEFT, "-min-cov", "-1"], "-min-cov must be 0..4294967295"),
    (BASE + ["-r", LEFT, "-seed", "-1"], "-seed must be 0..18446744073709551615"),
    (BASE + ["-r", LEFT, "-seed", str(1 << 64)], "-seed must be 0..18446744073709551615"),
    (BASE + ["-r", LEFT, "-min-count", "0"], "-min-count must be at least 1"),
    (BASE + ["-r", LEFT, "-c", DUMP, "-min-count", "2"], "-min-count is the counted table's bound"),
    (BASE + ["-r", LEFT, "-depth-max", "0"], "-depth-max must be 1..65535"),
    (BASE + ["-r", LEFT, "-depth-max", "65536"], "-depth-max must be 1..65535"),
    (BASE + ["-r", LEFT, "-batch", "0"], "-batch must be at least 1"),
    (BASE + ["-r", LEFT, os.path.join(FX, "ref", "..", "reads_1.fq")], "two input files would both be written to reads_1.norm.fq"),
    (BASE + ["-r", LEFT, "-frobnicate", "1"], "unknown option -frobnicate"),
    (BASE + ["-r", LEFT, "-o"], "-o needs a value"),
    (BASE + ["-r", LEFT, "-o", "a", "-o", "b"], "-o given twice"),
    (BASE + ["-r", LEFT, "-seed", "x"], "-seed needs an integer, got x"),
]


@pytest.mark.parametrize("args,text", BAD_ARGS, ids=["%d %s" % (i, t) for i, (_, t) in enumerate(BAD_ARGS)])
def test_usage_errors(tool, args, text):
    with pytest.raises(tool.UsageError, match=text):
        tool.parse_args(args)


def test_usage_errors_are_one_line_and_exit_status_2():
    for args, text in (BAD_ARGS[0], BAD_ARGS[3], BAD_ARGS[7], BAD_ARGS[16]):
        p = subprocess.run([sys.executable, TOOL] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        err = p.stderr.decode()
        assert p.returncode == 2 and p.stdout == b"" and err.count("\n") == 1 and text in err and "usage: read_normalize -k INT -target INT" in err


def test_defaults_and_output_names(tool):
    o = tool.parse_args(BASE + ["-p", LEFT, RIGHT])
    assert (o["min_cov"], o["seed"], o["min_count"], o["depth_max"], o["od"], o["c"]) == (0, 0, 1, 10000, ".", None)
    assert tool.parse_args(BASE + ["-r", LEFT, "-seed", str((1 << 64) - 1), "-target", str(TOP)])["seed"] == (1 << 64) - 1
    name = tool.output_name
    assert name("/a/b/X.fq") == "X.norm.fq" and name("X.fq.gz") == "X.norm.fq" and name("X.fa") == "X.norm.fa" and name("d/X.fa.gz") == "X.norm.fa"
    assert name("s_1.cor.fq") == "s_1.cor.norm.fq" and name("X.fastq.gz") == "X.norm.fq" and name("X.fasta") == "X.norm.fa"
    assert name("reads") == "reads.norm.fq" and name("reads", fastq=False) == "reads.norm.fa" and name("X.fq", fastq=False) == "X.norm.fa"


def test_the_raw_record_reader_gives_back_what_it_read(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gzip
    import kmer_sets
    fq = b"@r1 first\nACGT\n+\nIIII\n@r2\nNNNN\n+r2\n!!!!"          # (the last line without its line end)
    (tmp_path / "a.fq").write_bytes(fq)
    recs = list(kmer_sets.read_raw_records(str(tmp_path / "a.fq")))
    assert [(n, s) for n, s, _ in recs] == list(kmer_sets.read_records(str(tmp_path / "a.fq"))) == [(b"r1", b"ACGT"), (b"r2", b"NNNN")]
    assert b"".join(t for _, _, t in recs) == fq + b"\n"
    fa = b">s1 some words\nACGT\nAC\n>s2\n\n>s3\nGG\n"
    with gzip.open(str(tmp_path / "b.fa.gz"), "wb") as f:
        f.write(fa)
    recs = list(kmer_sets.read_raw_records(str(tmp_path / "b.fa.gz")))
    assert [(n, s) for n, s, _ in recs] == list(kmer_sets.read_records(str(tmp_path / "b.fa.gz"))) == [(b"s1", b"ACGTAC"), (b"s2", b""), (b"s3", b"GG")]
    assert [t for _, _, t in recs] == [b">s1 some words\nACGTAC\n", b">s2\n\n", b">s3\nGG\n"]
    (tmp_path / "empty.fq").write_bytes(b"")
    assert list(kmer_sets.read_raw_records(str(tmp_path / "empty.fq"))) == []
    (tmp_path / "bad.txt").write_bytes(b"hello\n")
    with pytest.raises(ValueError, match="neither FASTA nor FASTQ"):
        list(kmer_sets.read_raw_records(str(tmp_path / "bad.txt")))
