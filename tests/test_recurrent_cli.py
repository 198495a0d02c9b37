"""GPU: `rcorrector -recurrent FILE` -- the recurrent-correction census of a run: the sites (29 corrected bases around a change,
and the letter it was corrected from) at which one fix was made in many reads, and the line on stderr that sums it up.

For every golden fixture the `cmd.txt` command plus `-recurrent` must leave every output file and every stderr line the
reference wrote unchanged, add one line to stderr, and write the file the pure-Python model (tests/recur_model.py) computes
from the fixture's input reads and the REFERENCE's own `ref/*.cor.f[aq]` reads.  One paired fixture is repeated with -packed, in
many small batches with four in flight, on two contexts, from .gz input and to stdout; -recurrent-min / -top / -max run on the
data set of tests/recur_data.py, where sites do recur, against the model over the reads the run itself wrote.
"""
import gzip
import os
import shutil
import subprocess

import pytest

import golden_util as gu
import recur_model as rm
from test_recount_cli import VARIANTS, fixture_args, sequences

pytestmark = pytest.mark.gpu
CLI = os.path.join(gu.ROOT, "rcorrector_amd", "rcorrector")
PAIRED = "fx_pe_k23"


def seqs(path):
    return sequences(path).split(b"\0")[:-1]


def reads_of(name, ref):
    """the fixture's reads in file order, from its inputs (ref = False) or from the reference's corrected files"""
    d = os.path.join(gu.GOLDEN, name)
    args = fixture_args(name)

    def f(n):
        return os.path.join(d, "ref", "%s.cor%s" % os.path.splitext(n)) if ref else os.path.join(d, n)

    out = []
    for i, a in enumerate(args):
        if a == "-p":
            out += seqs(f(args[i + 1])) + seqs(f(args[i + 2]))
        elif a in ("-i", "-r"):
            out += seqs(f(args[i + 1]))
    return out


def expected(name, **kw):
    """(the file's text, the stderr line) from the model"""
    before, after = reads_of(name, False), reads_of(name, True)
    assert len(before) == len(after) > 0
    c = rm.Census().add(before, after)
    return c.file_text(**kw).encode(), (c.stderr_line(kw.get("min_count", 5)) + "\n").encode(), c


def check_run(p, path, want, golden_stderr):
    assert open(path, "rb").read() == want[0]
    assert p.stderr == golden_stderr + want[1]


@pytest.mark.parametrize("name", gu.FIXTURES + ["fa_se_k23"])
def test_recurrent_of_every_golden_fixture(name, tmp_path):
    want = expected(name)
    out, od = str(tmp_path / "recur.tsv"), tmp_path / "od"
    p = gu.run_fixture(CLI, name, od, extra=["-recurrent", out])
    gu.assert_same_as_reference(name, od, None, check_stderr=False)
    check_run(p, out, want, open(os.path.join(gu.GOLDEN, name, "ref", "stderr.txt"), "rb").read())


def test_the_fixtures_cover_pairs_interleaved_single_and_fasta():
    kinds = {a for n in gu.FIXTURES + ["fa_se_k23"] for a in fixture_args(n) if a in ("-p", "-i", "-r")}
    assert kinds == {"-p", "-i", "-r"}
    assert any(x.endswith(".fa") for x in fixture_args("fa_se_k23"))
    assert expected(PAIRED)[2].contexted > 0


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_recurrent_does_not_depend_on_transport_batching_or_contexts(variant, tmp_path):
    extra, env = VARIANTS[variant]
    d = os.path.join(gu.GOLDEN, PAIRED)
    out = str(tmp_path / "recur.tsv")
    od = tmp_path / "out"
    p = subprocess.run([CLI] + fixture_args(PAIRED) + ["-od", str(od), "-recurrent", out] + extra, cwd=d, env=dict(os.environ, **env),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    gu.assert_same_as_reference(PAIRED, od, None, check_stderr=False)
    check_run(p, out, expected(PAIRED), open(os.path.join(d, "ref", "stderr.txt"), "rb").read())


def test_recurrent_from_gz_input_and_to_stdout(tmp_path):
    src = os.path.join(gu.GOLDEN, PAIRED)
    golden = open(os.path.join(src, "ref", "stderr.txt"), "rb").read()
    work = tmp_path / "in"
    work.mkdir()
    for n in ("reads_1.fq", "reads_2.fq"):
        with open(os.path.join(src, n), "rb") as f, gzip.open(work / (n + ".gz"), "wb") as g:
            shutil.copyfileobj(f, g)
    od = tmp_path / "out"
    out = str(tmp_path / "gz.tsv")
    p = gu.run_fixture(CLI, PAIRED, od, args_override=["-p", str(work / "reads_1.fq.gz"), str(work / "reads_2.fq.gz"), "-k", "23", "-c",
                                                       os.path.join(src, "dump.jf"), "-batch", "100", "-recurrent", out])
    for n in ("reads_1", "reads_2"):
        assert gzip.open(od / (n + ".cor.fq.gz"), "rb").read() == open(os.path.join(src, "ref", n + ".cor.fq"), "rb").read()
    check_run(p, out, expected(PAIRED), golden)
    # -stdout: the records go to stdout as without the flag, the census to its file
    out = str(tmp_path / "stdout.tsv")
    plain = gu.run_fixture(CLI, PAIRED, tmp_path / "s0", extra=["-stdout"])
    p = gu.run_fixture(CLI, PAIRED, tmp_path / "s1", extra=["-stdout", "-recurrent", out])
    assert p.stdout == plain.stdout
    check_run(p, out, expected(PAIRED), plain.stderr)


@pytest.mark.parametrize("mode", [0, 1])
def test_recurrent_min_top_and_max_where_sites_recur(mode, tmp_path):
    import datasets
    import recur_data
    d = recur_data.make(mode)
    work = tmp_path / "in"
    work.mkdir()
    args = datasets.write_cli_case(d, str(work))

    def run(od, extra):
        p = subprocess.run([CLI] + args + ["-od", str(od)] + extra, cwd=str(work), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()
        return p

    plain = run(tmp_path / "plain", [])
    out = str(tmp_path / "recur.tsv")
    p = run(tmp_path / "od", ["-recurrent", out, "-recurrent-min", "2", "-recurrent-top", "5", "-recurrent-max", "3", "-batch", "500"])
    names = ["reads_1.cor.fq", "reads_2.cor.fq"] if mode == 1 else ["reads.cor.fq"]
    after = []
    for n in names:
        assert open(tmp_path / "od" / n, "rb").read() == open(tmp_path / "plain" / n, "rb").read()
        after += seqs(str(tmp_path / "od" / n))
    c = rm.Census().add(recur_data.all_reads(d), after)
    # (sites do recur here: the list is truncated, and the last recur line folds)
    assert sum(1 for v in c.keys.values() if v >= 2) > 5 and max(c.keys.values()) > 3
    assert open(out, "rb").read() == c.file_text(max_bin=3, min_count=2, max_sites=5).encode()
    assert p.stderr == plain.stderr + (c.stderr_line(2) + "\n").encode()
    text = open(out).read().splitlines()
    assert sum(1 for ln in text if ln.startswith("site\t")) == 5 and [ln for ln in text if ln.startswith("recur\t")][-1].startswith("recur\t3\t")


def test_recurrent_usage_errors(tmp_path):
    d = os.path.join(gu.GOLDEN, PAIRED)
    out = str(tmp_path / "r.tsv")

    def run(extra):
        return subprocess.run([CLI] + fixture_args(PAIRED) + ["-od", str(tmp_path)] + extra, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)

    p = run(["-recurrent", out, "-verbose"])
    assert p.returncode != 0 and b"-recurrent cannot be combined with -verbose" in p.stderr
    assert not os.path.exists(out)
    p = run(["-recurrent", out, "-recurrent-max", "0"])
    assert p.returncode != 0 and b"-recurrent-max" in p.stderr
    p = run(["-recurrent", out, "-recurrent-min", "0"])
    assert p.returncode != 0 and b"-recurrent-min" in p.stderr and not os.path.exists(out)
    # without -recurrent the three bounds are ignored, as -dups-max is without -dups
    p = run(["-recurrent-min", "0", "-recurrent-top", "3", "-recurrent-max", "0"])
    assert p.returncode == 0 and p.stderr == open(os.path.join(d, "ref", "stderr.txt"), "rb").read()
