"""tools/kmer_compare: the command over Context.table_compare.  CPU: argument errors, the formatter, the chunker against a
naive count of the uncut sequences.  GPU: two golden dumps against the model applied to the dumps parsed here, and the
tool's own counting (-a-seq) against the dump `rcorrector -write-dump` writes from the same reads."""
import collections
import gzip
import importlib.machinery
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import compare_model as cm
import golden_util as gu

TOOL = os.path.join(gu.ROOT, "tools", "kmer_compare")
CLI = os.path.join(gu.ROOT, "rcorrector_amd", "rcorrector")
DUMP_A = os.path.join(gu.GOLDEN, "fx_se_k23", "dump.jf")
DUMP_B = os.path.join(gu.GOLDEN, "fx_pe_k23", "dump.jf")


@pytest.fixture(scope="module")
def tool():
    loader = importlib.machinery.SourceFileLoader("kmer_compare", TOOL)
    spec = importlib.util.spec_from_loader("kmer_compare", loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


def run_tool(args, cwd=None):
    return subprocess.run([sys.executable, TOOL] + list(args), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


# ---- CPU -------------------------------------------------------------------------------------------------------------------

BAD_ARGS = [
    ([], "-k is required"),
    (["-k", "23", "-a", DUMP_A], "side b: give either"),
    (["-k", "23", "-a", DUMP_A, "-a-seq", DUMP_A, "-b", DUMP_B], "side a: give either"),
    (["-k", "0", "-a", DUMP_A, "-b", DUMP_B], "-k must be 1..32"),
    (["-k", "33", "-a", DUMP_A, "-b", DUMP_B], "-k must be 1..32"),
    (["-k", "x", "-a", DUMP_A, "-b", DUMP_B], "-k needs an integer"),
    (["-k", "23", "-a", DUMP_A, "-b", DUMP_B, "-max-bin", "0"], "-max-bin must be 1..1023"),
    (["-k", "23", "-a", DUMP_A, "-b", DUMP_B, "-max-bin", "1024"], "-max-bin must be 1..1023"),
    (["-k", "23", "-a", DUMP_A, "-b", DUMP_B, "-min-count", "0"], "-min-count must be at least 1"),
    (["-k", "23", "-a", DUMP_A, "-b", "/nonexistent/dump.jf"], "cannot read /nonexistent/dump.jf"),
    (["-k", "23", "-a", DUMP_A, "-a", DUMP_A, "-b", DUMP_B], "-a given twice"),
    (["-k", "23", "-a", DUMP_A, "-b", DUMP_B, "-frobnicate", "1"], "unknown option -frobnicate"),
    (["-k", "23", "-a", DUMP_A, "-b", DUMP_B, "-o"], "-o needs a value"),
]


@pytest.mark.parametrize("args,text", BAD_ARGS, ids=[t for _, t in BAD_ARGS])
def test_usage_errors_exit_1_with_one_line(tool, args, text):
    with pytest.raises(tool.UsageError, match=text.replace("(", r"\(").replace(")", r"\)")):
        tool.parse_args(args)


def test_usage_error_from_the_command_line_touches_no_gpu(tmp_path):
    """status 1, one line on stderr, nothing on stdout -- in a process that cannot see a GPU at all"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, TOOL, "-k", "23", "-a", DUMP_A], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=60)
    assert p.returncode == 1 and p.stdout == b""
    err = p.stderr.decode()
    assert err.count("\n") == 1 and err.startswith("kmer_compare: side b: give either") and "usage: kmer_compare -k INT" in err


def test_defaults_and_repeated_sequence_files(tool):
    o = tool.parse_args(["-k", "23", "-a-seq", DUMP_A, "-a-seq", DUMP_B, "-b", DUMP_B])
    assert o == {"k": 23, "a": None, "a_seq": [DUMP_A, DUMP_B], "b": DUMP_B, "b_seq": [], "min_count": 1, "max_bin": 255, "out": None}


def test_formatter_from_a_given_matrix(tool):
    cells = np.zeros((4, 4), np.uint64)
    cells[0, 2], cells[1, 0], cells[1, 1], cells[3, 3], cells[2, 3] = 5, 7, 11, 2, 1
    res = {"cells": cells, "distinct_a": 21, "distinct_b": 19, "shared": 14, "mass_a": 1 << 40, "mass_b": 77, "shared_mass_a": (1 << 40) - 7,
           "shared_mass_b": 60, "max_count_a": 1 << 31, "max_count_b": 9}
    assert tool.format_result(23, 3, res) == (
        "k\t23\nmax_bin\t3\ndistinct\ta\t21\ndistinct\tb\t19\nshared\t14\nonly\ta\t7\nonly\tb\t5\n"
        "mass\ta\t1099511627776\nmass\tb\t77\nshared_mass\ta\t1099511627769\nshared_mass\tb\t60\n"
        "cell\t0\t2\t5\ncell\t1\t0\t7\ncell\t1\t1\t11\ncell\t2\t3\t1\ncell\t3\t3\t2\n")
    line = tool.summary_line(res)
    assert "\n" not in line and "14 shared of 21 (a) and 19 (b)" in line and "Jaccard 0.5385" in line and "77.92 % of b's" in line
    empty = dict(res, cells=np.zeros((2, 2), np.uint64), distinct_a=0, distinct_b=0, shared=0, mass_a=0, mass_b=0, shared_mass_a=0, shared_mass_b=0)
    assert "Jaccard 0.0000" in tool.summary_line(empty)


def naive_kmers(seqs, k):
    """every window of k upper-case ACGT letters, canonical, as text -- what the counter counts"""
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    out = collections.Counter()
    for s in seqs:
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if w.strip(b"ACGT"):
                continue
            out[min(w, w.translate(comp)[::-1])] += 1
    return out


def test_chunker_counts_every_window_once(tool, tmp_path):
    """A multi-line FASTA (plain and .gz), with runs of N, lower case and sequences shorter than k, cut at several chunk
    sizes: the pieces hold the same multiset of k-mers as the uncut sequences."""
    k = 11
    rng = np.random.default_rng(12)
    seqs = []
    for n in (5000, 3, 10, 11, 12, 700, 2047, 2048, 2049, 0):
        s = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes())
        for _ in range(n // 400):
            at = int(rng.integers(0, n))
            run = int(rng.integers(1, 30))
            s[at:at + run] = b"N" * len(s[at:at + run])
        if n == 700:
            s[100:160] = bytes(s[100:160]).lower()
        seqs.append(bytes(s)[:n])
    fa = tmp_path / "contigs.fa"
    with open(fa, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">c%d some text\n" % i + b"".join(s[j:j + 60] + b"\n" for j in range(0, len(s), 60)))
    with gzip.open(str(fa) + ".gz", "wb") as f:
        f.write(open(fa, "rb").read())
    fq = tmp_path / "reads.fq"
    with open(fq, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
    for path in (fa, str(fa) + ".gz", fq):
        assert list(tool.read_sequences(str(path))) == seqs
    want = naive_kmers(seqs, k)
    assert sum(want.values()) > 9000 and len(naive_kmers([seqs[5]], k)) < 700 - k + 1 - 60    # the lower-case stretch is skipped
    for chunk in (2 * k, 23, 64, 1000, 2048, 2049, 1 << 20):
        arenas = list(tool.chunk_arenas(iter(seqs), k, chunk))
        assert all(0 < len(a) <= chunk and a.endswith(b"\0") for a in arenas)
        pieces = [p for a in arenas for p in a[:-1].split(b"\0")]
        assert all(len(p) >= k for p in pieces)
        assert naive_kmers(pieces, k) == want, "chunks of %d bytes" % chunk
    assert len(list(tool.chunk_arenas(iter(seqs), k, 1 << 20))) == 1
    with pytest.raises(ValueError):
        list(tool.chunk_arenas(iter(seqs), k, 2 * k - 1))


# ---- GPU -------------------------------------------------------------------------------------------------------------------

def parse_dump(path, k):
    """(codes, counts) of a `jellyfish dump` text file as the table load takes it: counts of 0 and 1 dropped"""
    tok = open(path, "rb").read().split()
    counts = np.array([int(t[1:]) for t in tok[0::2]], dtype=np.int64)
    val = np.zeros(256, np.uint64)
    val[ord("C")], val[ord("G")], val[ord("T")] = 1, 2, 3
    text = np.frombuffer(b"".join(tok[1::2]), np.uint8).reshape(-1, k)
    codes = np.zeros(len(text), np.uint64)
    for j in range(k):
        codes = (codes << np.uint64(2)) | val[text[:, j]]
    keep = counts >= 2
    return codes[keep], counts[keep]


def parse_output(text):
    lines = [l.split("\t") for l in text.splitlines()]
    head = {tuple(l[:-1]): int(l[-1]) for l in lines if l[0] != "cell"}
    cells = [(int(l[1]), int(l[2]), int(l[3])) for l in lines if l[0] == "cell"]
    return head, cells


@pytest.mark.gpu
def test_two_golden_dumps_equal_the_model(tool, tmp_path):
    out = str(tmp_path / "cmp.tsv")
    p = run_tool(["-k", "23", "-a", DUMP_A, "-b", DUMP_B, "-max-bin", "63", "-o", out])
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout == b""
    want = cm.compare(parse_dump(DUMP_A, 23), parse_dump(DUMP_B, 23), 23, 63)
    assert want["distinct_a"] > 1000 and want["distinct_b"] > 1000
    assert open(out).read() == tool.format_result(23, 63, want)
    assert p.stderr.decode().splitlines()[-1] == tool.summary_line(want)


@pytest.mark.gpu
def test_the_tools_counting_equals_the_binarys_dump(tool, tmp_path):
    """-a-seq on a golden read file with -min-count 2 against -b on the dump `rcorrector -write-dump` writes from the same
    reads: the same k-mers with the same counts -- everything on the diagonal, nothing on one side only."""
    d = os.path.join(gu.GOLDEN, "fx_se_k23")
    dump = str(tmp_path / "counted.jf")
    od = tmp_path / "out"
    od.mkdir()
    r = subprocess.run([CLI, "-r", os.path.join(d, "reads.fq"), "-k", "23", "-write-dump", dump, "-od", str(od)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    p = run_tool(["-k", "23", "-a-seq", os.path.join(d, "reads.fq"), "-min-count", "2", "-b", dump, "-max-bin", "1023"])
    assert p.returncode == 0, p.stderr.decode()
    head, cells = parse_output(p.stdout.decode())
    assert head[("k",)] == 23 and head[("max_bin",)] == 1023
    assert head[("only", "a")] == head[("only", "b")] == 0
    assert head[("distinct", "a")] == head[("distinct", "b")] == head[("shared",)] == sum(n for _, _, n in cells) > 1000
    assert head[("mass", "a")] == head[("mass", "b")] == head[("shared_mass", "a")] == head[("shared_mass", "b")]
    assert cells and all(i == j and i >= 2 for i, j, _ in cells)
