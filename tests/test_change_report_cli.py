"""GPU: `rcorrector -report FILE` -- the correction report as tab-separated text.

For the golden fixtures below, the `cmd.txt` command plus `-report` must write the file that the numpy model of
tests/test_change_report.py gives for the fixture's input reads against the REFERENCE's own `ref/*.cor.f[aq]` (which reads
are unfixable: the reference's header mark; which qualities are low: the character in `ref/stderr.txt`'s "Bad quality
threshold is" line), while the outputs and stderr stay the goldens byte for byte.  One paired fixture is repeated on two
contexts, in many small batches with four in flight (byte and packed transport, lanes on and off), and without -c (the
one-pass resident transport: there the expectation comes from that run's own corrected files against its input).
"""
import os
import re
import subprocess

import numpy as np
import pytest

import golden_util as gu
from test_change_report import MAX_PER_READ, SHAPES, add_reports, consistent, model, zero_report

pytestmark = pytest.mark.gpu
CLI = os.path.join(gu.ROOT, "rcorrector_amd", "rcorrector")
PAIRED = "fx_pe_k23"
NAMES = ["fx_pe_k23", "fx_se_k23", "fx_il_k23", "fa_se_k23", "fx_sample", "fx_k31_mc8"]


def fixture_args(name):
    return open(os.path.join(gu.GOLDEN, name, "cmd.txt")).read().split()


def records(path):
    """(headers, arena of the sequences, arena of the qualities or None, offsets) of a FASTQ / FASTA file"""
    lines = open(path, "rb").read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    fastq = lines[0].startswith(b"@")
    step = 4 if fastq else 2
    assert len(lines) % step == 0
    heads, seqs = lines[0::step], lines[1::step]
    off = np.concatenate([[0], np.cumsum([len(s) + 1 for s in seqs])]).astype(np.uint32)
    arena = np.frombuffer(b"".join(s + b"\0" for s in seqs), dtype=np.uint8)
    qual = None
    if fastq:
        quals = lines[3::step]
        assert all(len(q) == len(s) for q, s in zip(quals, seqs))
        qual = np.frombuffer(b"".join(q + b"\0" for q in quals), dtype=np.uint8)
    return heads, arena, qual, off


def inputs_of(args):
    """[(input file, output file name, mate rule)] of a command line"""
    out = []
    for i, a in enumerate(args):
        if a == "-r":
            out.append((args[i + 1], 0))
        elif a == "-p":
            out += [(args[i + 1], 0), (args[i + 2], 1)]
        elif a == "-i":
            out.append((args[i + 1], 2))
    res = []
    for f, rule in out:
        stem, ext = os.path.splitext(os.path.basename(f))
        res.append((f, stem + ".cor" + ext, rule))
    return res


def expected(name, cor_dir=None, bad_q=None, args=None):
    d = os.path.join(gu.GOLDEN, name)
    args = fixture_args(name) if args is None else args
    cor_dir = os.path.join(d, "ref") if cor_dir is None else cor_dir
    if bad_q is None:
        bad_q = re.search(rb"Bad quality threshold is '(.)'", open(os.path.join(d, "ref", "stderr.txt"), "rb").read(), re.S).group(1)
    R, two = zero_report(), False
    for f, cor, rule in inputs_of(args):
        _, orig, qual, off = records(os.path.join(d, f))
        heads, corr, _, off_c = records(os.path.join(cor_dir, cor))
        assert np.array_equal(off, off_c)          # substitutions only
        ret = np.array([-1 if h.endswith(b"unfixable_error") else 0 for h in heads])
        two = two or rule != 0
        mate_of = (lambda r: r & 1) if rule == 2 else (lambda r, rule=rule: rule)
        R = add_reports(R, model(orig, corr, off, ret, qual, mate_of, bad_q))
    assert consistent(R) > 0 and int(R["reads_unfixable"].sum()) > 0
    return R, two


def report_text(R, two_mates):
    mates = (0, 1) if two_mates else (0,)
    out = []
    for m in mates:
        out.append("reads\t%d\t%d\t%d\t%d" % (m + 1, R["reads"][m], R["reads_changed"][m], R["reads_unfixable"][m]))
    for m in mates:
        out.append("changes\t%d\t%d" % (m + 1, R["changes"][m]))
    longest = [int(np.nonzero(R["len_hist"][m])[0].max()) if R["len_hist"][m].any() else 0 for m in (0, 1)]
    for m in mates:
        for p in range(1, longest[m] + 1):
            out.append("pos5\t%d\t%d\t%d\t%d" % (m + 1, p, R["by_pos5"][m][p - 1], R["len_hist"][m][p:].sum()))
    for m in mates:
        for p in range(1, longest[m] + 1):
            out.append("pos3\t%d\t%d\t%d" % (m + 1, p, R["by_pos3"][m][p - 1]))
    for a in range(5):
        for b in range(4):
            out.append("subst\t%s\t%s\t%d" % ("ACGTN"[a], "ACGT"[b], R["subst"][a][b]))
    for q, what in enumerate(("low", "high", "none")):
        out.append("qual\t%s\t%d" % (what, R["by_qual"][q]))
    for c in range(MAX_PER_READ + 1):
        if R["per_read"][c]:
            out.append("perread\t%s\t%d" % ("%d+" % c if c == MAX_PER_READ else str(c), R["per_read"][c]))
    return ("\n".join(out) + "\n").encode()


def parse_report(text):
    """the file back into the model's arrays (what a user's plotting script would do): checks the format line by line"""
    R = zero_report()
    for ln in text.decode().splitlines():
        f = ln.split("\t")
        if f[0] == "reads":
            m = int(f[1]) - 1
            R["reads"][m], R["reads_changed"][m], R["reads_unfixable"][m] = int(f[2]), int(f[3]), int(f[4])
        elif f[0] == "changes":
            R["changes"][int(f[1]) - 1] = int(f[2])
        elif f[0] == "pos5":
            R["by_pos5"][int(f[1]) - 1][int(f[2]) - 1] = int(f[3])
        elif f[0] == "pos3":
            R["by_pos3"][int(f[1]) - 1][int(f[2]) - 1] = int(f[3])
        elif f[0] == "subst":
            R["subst"]["ACGTN".index(f[1])]["ACGT".index(f[2])] = int(f[3])
        elif f[0] == "qual":
            R["by_qual"][("low", "high", "none").index(f[1])] = int(f[2])
        elif f[0] == "perread":
            R["per_read"][int(f[1].rstrip("+"))] = int(f[2])
        else:
            raise AssertionError("unknown section in %r" % ln)
    return R


def run(name, outdir, extra=(), env=None, args=None):
    d = os.path.join(gu.GOLDEN, name)
    p = subprocess.run([CLI] + list(fixture_args(name) if args is None else args) + ["-od", str(outdir)] + list(extra), cwd=d,
                       env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    return p


def outputs(outdir):
    return {f: open(os.path.join(str(outdir), f), "rb").read() for f in sorted(os.listdir(str(outdir)))}


@pytest.mark.parametrize("name", NAMES)
def test_report_of_a_golden_fixture(name, tmp_path):
    want, two = expected(name)
    rep = str(tmp_path / "report.tsv")
    od, od0 = tmp_path / "with", tmp_path / "without"
    p = run(name, od, ["-report", rep])
    got = open(rep, "rb").read()
    assert got == report_text(want, two)
    back = parse_report(got)
    for key in ("reads", "reads_changed", "reads_unfixable", "changes", "by_pos5", "by_pos3", "subst", "by_qual", "per_read"):
        assert np.array_equal(back[key], want[key]), key
    per_mate = [ln.split(b"\t") for ln in got.splitlines() if ln.split(b"\t")[0] in (b"reads", b"changes", b"pos5", b"pos3")]
    assert {f[1] for f in per_mate} == ({b"1", b"2"} if two else {b"1"})     # mate 2 only for paired / interleaved input
    if name == "fa_se_k23":
        assert want["by_qual"][2] == want["changes"].sum()
    # outputs and stderr are the reference's, and those of a run without the flag
    golden = open(os.path.join(gu.GOLDEN, name, "ref", "stderr.txt"), "rb").read()
    gu.assert_same_as_reference(name, od, None, check_stderr=False)
    assert p.stderr == golden
    p0 = run(name, od0)
    assert p0.stderr == p.stderr and p0.stdout == p.stdout and outputs(od0) == outputs(od)


VARIANTS = {
    "two_contexts": (["-gpus", "2", "-batch", "64", "-inflight", "2"], {"RC_SHARED_GPU": "1"}),
    "two_contexts_packed": (["-gpus", "2", "-batch", "64", "-packed"], {"RC_SHARED_GPU": "1"}),
    "small_batches": (["-batch", "60", "-inflight", "4"], {}),
    "small_batches_lanes_off": (["-batch", "60", "-inflight", "4"], {"RC_SLOT_LANES": "0"}),
    "small_batches_packed": (["-packed", "-batch", "60", "-inflight", "4"], {}),
    "small_batches_packed_lanes_off": (["-packed", "-batch", "60", "-inflight", "4"], {"RC_SLOT_LANES": "0"}),
    "with_histo_after": (["-batch", "100", "-histo-after", "after.histo"], {}),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_report_does_not_depend_on_contexts_batching_or_transport(variant, tmp_path):
    extra, env = VARIANTS[variant]
    extra = [str(tmp_path / a) if a.endswith(".histo") else a for a in extra]
    want, two = expected(PAIRED)
    n_reads = len(open(os.path.join(gu.GOLDEN, PAIRED, "reads_1.fq"), "rb").read().split(b"\n")) // 4
    assert n_reads * 2 >= 5 * 64   # (-batch counts reads: at least five batches)
    rep = str(tmp_path / "report.tsv")
    od, od0 = tmp_path / "with", tmp_path / "without"
    p = run(PAIRED, od, extra + ["-report", rep], env)
    assert open(rep, "rb").read() == report_text(want, two)
    p0 = run(PAIRED, od0, extra, env)
    assert p0.stderr == p.stderr and outputs(od0) == outputs(od)
    gu.assert_same_as_reference(PAIRED, od, None, check_stderr=False)


@pytest.mark.parametrize("env", [{"RC_RESIDENT": "1"}, {"RC_RESIDENT": "0"}, {"RC_RESIDENT": "1", "RC_SHARED_GPU": "1"}], ids=["one_pass", "two_pass", "two_ctx"])
def test_report_without_a_dump(env, tmp_path):
    """no -c: the k-mers are counted here and (RC_RESIDENT=1) the reads corrected where the counter kept them -- the expectation is
    the model's over the run's own corrected files against its input, unfixable reads by the run's own header marks"""
    args = fixture_args(PAIRED)
    i = args.index("-c")
    del args[i:i + 2]
    extra = ["-batch", "100"] + (["-gpus", "2"] if "RC_SHARED_GPU" in env else [])
    rep = str(tmp_path / "report.tsv")
    od, od0 = tmp_path / "with", tmp_path / "without"
    p = run(PAIRED, od, extra + ["-report", rep], env, args)
    p0 = run(PAIRED, od0, extra, env, args)
    assert p0.stderr == p.stderr and outputs(od0) == outputs(od)
    bad_q = re.search(rb"Bad quality threshold is '(.)'", p.stderr, re.S).group(1)
    want, two = expected(PAIRED, cor_dir=str(od), bad_q=bad_q, args=args)
    assert open(rep, "rb").read() == report_text(want, two)
    assert int(re.search(rb"Corrected (\d+) bases", p.stderr).group(1)) == int(want["changes"].sum())
