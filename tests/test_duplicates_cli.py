"""GPU: `rcorrector -dups FILE` -- the duplicate census of a run: how many reads (pairs, for -p and -i input) are exact copies of
one another, as they were read and as they were corrected, and the line on stderr that gives the duplicate fractions.

For every golden fixture the `cmd.txt` command plus `-dups` must leave every output file and every stderr line the reference
wrote unchanged, add one line to stderr, and write the file a collections.Counter computes: `before` from the sequences of the
fixture's input files, `after` from those of the REFERENCE's own `ref/*.cor.f[aq]`.  One paired fixture is repeated with
-packed, in many small batches with four in flight, on two contexts, from .gz input, to stdout and with a small -dups-max.
"""
import collections
import gzip
import os
import shutil
import subprocess

import pytest

import golden_util as gu
from test_recount_cli import VARIANTS, fixture_args, sequences

pytestmark = pytest.mark.gpu
CLI = os.path.join(gu.ROOT, "rcorrector_amd", "rcorrector")
PAIRED = "fx_pe_k23"


def seqs(path):
    return sequences(path).split(b"\0")[:-1]


def units_of(name, ref):
    """the fixture's units, from its inputs (ref = False) or from the reference's corrected files: (list, "reads" | "pairs")"""
    d = os.path.join(gu.GOLDEN, name)
    args = fixture_args(name)

    def f(n):
        return os.path.join(d, "ref", "%s.cor%s" % os.path.splitext(n)) if ref else os.path.join(d, n)

    if "-p" in args:
        i = args.index("-p")
        return list(zip(seqs(f(args[i + 1])), seqs(f(args[i + 2])))), "pairs"
    if "-i" in args:
        s = seqs(f(args[args.index("-i") + 1]))
        return list(zip(s[0::2], s[1::2])), "pairs"
    return seqs(f(args[args.index("-r") + 1])), "reads"


def expected(name, max_bin=10000):
    """(the file's text, the stderr line) from two Counters"""
    (before, unit), (after, _) = units_of(name, False), units_of(name, True)
    assert len(before) == len(after) > 0
    rows, distinct = {}, []
    for col, units in enumerate((before, after)):
        c = collections.Counter(units)
        distinct.append(len(c))
        for v in c.values():
            rows.setdefault(min(v, max_bin), [0, 0])[col] += 1
    n = len(before)
    text = "units\t%d\t%s\ndistinct\tbefore\t%d\ndistinct\tafter\t%d\n" % (n, unit, distinct[0], distinct[1])
    text += "".join("copies\t%d\t%d\t%d\n" % (c, rows[c][0], rows[c][1]) for c in sorted(rows))
    line = "Duplicates: %d %s, %d distinct before correction (duplicate fraction %.4f), %d after (%.4f)\n" % (
        n, unit, distinct[0], 1.0 - distinct[0] / n, distinct[1], 1.0 - distinct[1] / n)
    return text.encode(), line.encode()


def check_run(p, path, want, golden_stderr):
    assert open(path, "rb").read() == want[0]
    assert p.stderr == golden_stderr + want[1]


@pytest.mark.parametrize("name", gu.FIXTURES + ["fa_se_k23"])
def test_dups_of_every_golden_fixture(name, tmp_path):
    want = expected(name)
    out, od = str(tmp_path / "dups.tsv"), tmp_path / "od"
    p = gu.run_fixture(CLI, name, od, extra=["-dups", out])
    gu.assert_same_as_reference(name, od, None, check_stderr=False)
    check_run(p, out, want, open(os.path.join(gu.GOLDEN, name, "ref", "stderr.txt"), "rb").read())


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_dups_do_not_depend_on_transport_batching_or_contexts(variant, tmp_path):
    extra, env = VARIANTS[variant]
    d = os.path.join(gu.GOLDEN, PAIRED)
    out = str(tmp_path / "dups.tsv")
    od = tmp_path / "out"
    p = subprocess.run([CLI] + fixture_args(PAIRED) + ["-od", str(od), "-dups", out] + extra, cwd=d, env=dict(os.environ, **env),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    gu.assert_same_as_reference(PAIRED, od, None, check_stderr=False)
    check_run(p, out, expected(PAIRED), open(os.path.join(d, "ref", "stderr.txt"), "rb").read())


def test_dups_from_gz_input_to_stdout_and_with_a_small_bound(tmp_path):
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
                                                       os.path.join(src, "dump.jf"), "-batch", "100", "-dups", out])
    for n in ("reads_1", "reads_2"):
        assert gzip.open(od / (n + ".cor.fq.gz"), "rb").read() == open(os.path.join(src, "ref", n + ".cor.fq"), "rb").read()
    check_run(p, out, expected(PAIRED), golden)
    # -stdout: the records go to stdout as without the flag, the census to its file
    out = str(tmp_path / "stdout.tsv")
    plain = gu.run_fixture(CLI, PAIRED, tmp_path / "s0", extra=["-stdout"])
    p = gu.run_fixture(CLI, PAIRED, tmp_path / "s1", extra=["-stdout", "-dups", out])
    assert p.stdout == plain.stdout
    check_run(p, out, expected(PAIRED), plain.stderr)
    # -dups-max 1: every distinct unit in the one line; the counts of distinct units and the stderr line do not change
    out = str(tmp_path / "max1.tsv")
    p = gu.run_fixture(CLI, PAIRED, tmp_path / "m1", extra=["-dups", out, "-dups-max", "1"])
    want = expected(PAIRED, 1)
    assert len(want[0].splitlines()) == 4 and want[1] == expected(PAIRED)[1]
    check_run(p, out, want, golden)


def test_dups_with_verbose_is_refused(tmp_path):
    d = os.path.join(gu.GOLDEN, PAIRED)
    p = subprocess.run([CLI] + fixture_args(PAIRED) + ["-od", str(tmp_path), "-dups", str(tmp_path / "d.tsv"), "-verbose"], cwd=d,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"-dups cannot be combined with -verbose" in p.stderr
    assert not os.path.exists(str(tmp_path / "d.tsv"))
    p = subprocess.run([CLI] + fixture_args(PAIRED) + ["-od", str(tmp_path), "-dups", str(tmp_path / "d.tsv"), "-dups-max", "0"], cwd=d,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"-dups-max" in p.stderr
    # reads and pairs in one census: refused before anything runs
    p = subprocess.run([CLI] + fixture_args(PAIRED) + ["-r", "reads_1.fq", "-od", str(tmp_path), "-dups", str(tmp_path / "d.tsv")], cwd=d,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"not a mix" in p.stderr and not os.path.exists(str(tmp_path / "d.tsv"))
