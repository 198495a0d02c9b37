"""GPU: `rcorrector -trust-by-pos FILE [-weak-min INT]` -- the k-mer trust profile of a run by read position, before and after
correction, and the line on stderr that gives the weak share of the valid windows.

For a paired, an interleaved, a FASTA and a .gz fixture the file must equal the one formatted here from the pure-Python
restatement (tests/test_trust_profile.py) -- `before` over the sequences of the fixture's input files, `after` over those of the
REFERENCE's own ref/*.cor.f[aq] --, the outputs and every other stderr line are byte for byte those of the run without the
flag, two contexts give the same file, and -verbose refuses the flag."""
import gzip
import os
import shutil
import subprocess

import pytest

import golden_util as gu
from test_recount_cli import fixture_args, sequences
from test_trust_profile import FIELDS, MAX_LEN, restate_reads
from test_weak_profile_cli import dump_dict, outputs, run

pytestmark = pytest.mark.gpu
PAIRED = "fx_pe_k23"
_want = {}


def seqs(path):
    return sequences(path).split(b"\0")[:-1]


def versions_of(name):
    """(mode, [reads before, reads after]) in the order the library sees them: mode 1 = mates 1, then mates 2"""
    d, args = os.path.join(gu.GOLDEN, name), fixture_args(name)
    ref = lambda n: os.path.join(d, "ref", "%s.cor%s" % os.path.splitext(n))   # noqa: E731
    if "-p" in args:
        i = args.index("-p")
        names, mode = [args[i + 1], args[i + 2]], 1
    else:
        flag = "-i" if "-i" in args else "-r"
        names, mode = [args[args.index(flag) + 1]], 2 if flag == "-i" else 0
    return mode, [sum((seqs(os.path.join(d, n)) for n in names), []), sum((seqs(ref(n)) for n in names), [])]


def expected(name, min_count=1):
    """(the file's text, the stderr line) from the restatement"""
    if (name, min_count) in _want:
        return _want[name, min_count]
    args = fixture_args(name)
    k = int(args[args.index("-k") + 1])
    counts = dump_dict(os.path.join(gu.GOLDEN, name, "dump.jf"))
    mode, versions = versions_of(name)
    memo = {}
    c = [restate_reads(v, mode, k, counts, min_count, memo) for v in versions]
    mates = 1 if mode == 0 else 2
    n = len(versions[0])
    reads = [n, 0] if mode == 0 else [n // 2, n // 2]
    text = "k\t%d\nmin_count\t%d\n" % (k, min_count)
    text += "".join("reads\t%d\t%d\n" % (m + 1, reads[m]) for m in range(mates))
    tags = ("before", "after")
    for v in range(2):
        for m in range(mates):
            w, s, x = (int(c[v][f][m].sum()) for f in ("windows", "solid5", "weak5"))
            text += "total\t%s\t%d\t%d\t%d\t%d\t%d\n" % (tags[v], m + 1, w, s, x, w - s - x)
    for end in ("5", "3"):
        for v in range(2):
            for m in range(mates):
                for p in range(MAX_LEN):
                    w, s, x = (int(c[v][f][m][p]) for f in ("windows", "solid" + end, "weak" + end))
                    if w:
                        text += "pos%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (end, tags[v], m + 1, p, w, s, x, w - s - x)
    weak = [int(c[v]["weak5"].sum()) for v in range(2)]
    valid = [weak[v] + int(c[v]["solid5"].sum()) for v in range(2)]
    assert valid[0] > weak[0] > weak[1] > 0 and set(FIELDS) == set(c[0])
    line = "Trust by position (k-mers counted below %d are weak): %d of %d valid k-mer windows weak before correction (%.4f), %d of %d after (%.4f)\n" % (
        min_count, weak[0], valid[0], weak[0] / valid[0], weak[1], valid[1], weak[1] / valid[1])
    _want[name, min_count] = (text.encode(), line.encode())
    return _want[name, min_count]


@pytest.mark.parametrize("name", ["fx_pe_k23", "fx_il_k23", "fa_se_k23"])
def test_trust_by_pos_file_and_nothing_else(name, tmp_path):
    min_count = 3 if name == "fx_il_k23" else 1
    want = expected(name, min_count)
    out = str(tmp_path / "trust.tsv")
    args = fixture_args(name)
    p = run(name, tmp_path / "with", args, ["-batch", "100", "-trust-by-pos", out] + (["-weak-min", "3"] if min_count == 3 else []))
    p0 = run(name, tmp_path / "without", args, ["-batch", "100"])
    assert open(out, "rb").read() == want[0]
    assert p.stderr == p0.stderr + want[1] and p.stdout == p0.stdout
    got, plain = outputs(tmp_path / "with"), outputs(tmp_path / "without")
    assert got == plain and len(got) > 0
    for f in got:
        assert got[f] == open(os.path.join(gu.GOLDEN, name, "ref", f), "rb").read(), f
    assert (b"reads\t2\t" in want[0]) == (name != "fa_se_k23")                       # mate-2 lines only for paired / interleaved input


def test_trust_by_pos_from_gz_input_packed_and_to_stdout(tmp_path):
    src = os.path.join(gu.GOLDEN, PAIRED)
    want = expected(PAIRED)
    work = tmp_path / "in"
    work.mkdir()
    for n in ("reads_1.fq", "reads_2.fq"):
        with open(os.path.join(src, n), "rb") as f, gzip.open(work / (n + ".gz"), "wb") as g:
            shutil.copyfileobj(f, g)
    out = str(tmp_path / "gz.tsv")
    args = ["-p", str(work / "reads_1.fq.gz"), str(work / "reads_2.fq.gz"), "-k", "23", "-c", os.path.join(src, "dump.jf"), "-batch", "100"]
    p = run(PAIRED, tmp_path / "gz", args, ["-trust-by-pos", out])
    p0 = run(PAIRED, tmp_path / "gz0", args)
    for n in ("reads_1", "reads_2"):
        assert gzip.open(tmp_path / "gz" / (n + ".cor.fq.gz"), "rb").read() == open(os.path.join(src, "ref", n + ".cor.fq"), "rb").read()
    assert open(out, "rb").read() == want[0] and p.stderr == p0.stderr + want[1]
    # -packed, lanes off, four batches in flight
    out = str(tmp_path / "packed.tsv")
    p = run(PAIRED, tmp_path / "pk", fixture_args(PAIRED), ["-packed", "-batch", "60", "-inflight", "4", "-trust-by-pos", out], {"RC_SLOT_LANES": "0"})
    assert open(out, "rb").read() == want[0] and p.stderr.endswith(want[1])
    # -stdout: the records go to stdout as without the flag, the profile to its file
    out = str(tmp_path / "stdout.tsv")
    plain = run(PAIRED, tmp_path / "s0", fixture_args(PAIRED), ["-stdout"])
    p = run(PAIRED, tmp_path / "s1", fixture_args(PAIRED), ["-stdout", "-trust-by-pos", out])
    assert p.stdout == plain.stdout and len(p.stdout) > 0
    assert open(out, "rb").read() == want[0] and p.stderr == plain.stderr + want[1]


def test_two_contexts_give_the_same_file(tmp_path):
    want = expected(PAIRED)
    out = str(tmp_path / "two.tsv")
    p = run(PAIRED, tmp_path / "two", fixture_args(PAIRED), ["-gpus", "2", "-batch", "64", "-inflight", "2", "-trust-by-pos", out], {"RC_SHARED_GPU": "1"})
    gu.assert_same_as_reference(PAIRED, tmp_path / "two", None, check_stderr=False)
    assert open(out, "rb").read() == want[0] and p.stderr.endswith(want[1])


def test_trust_by_pos_with_verbose_is_refused(tmp_path):
    out = str(tmp_path / "t.tsv")
    p = run(PAIRED, tmp_path, fixture_args(PAIRED), ["-trust-by-pos", out, "-verbose"], ok=False)
    assert p.returncode != 0 and b"-trust-by-pos cannot be combined with -verbose" in p.stderr
    assert not os.path.exists(out)
    p = subprocess.run([os.path.join(gu.ROOT, "rcorrector_amd", "rcorrector"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.stderr.index(b"\t-dups-max INT:") < p.stderr.index(b"\t-trust-by-pos STRING:") < p.stderr.index(b"\t-verbose-iter INT:")
