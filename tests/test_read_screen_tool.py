"""tools/read_screen: the command over Context.read_screen_device.  fx_pe_k23's ref/*.cor.fq as the reads, a multi-line FASTA
written here from some of them (-s-seq) or a dump written here (-s) as the screen set; every line of the report, the per-read
file and the flagged list against the restatement of tests/test_read_screen.py and a Python tally of its rows."""
import importlib.machinery
import importlib.util
import os
import subprocess
import sys

import pytest

import golden_util as gu
from seam_arena import canonical
from test_read_screen import counts_of_reads, restate
from test_weak_profile import fastx_seqs

TOOL = os.path.join(gu.ROOT, "tools", "read_screen")
FX = os.path.join(gu.GOLDEN, "fx_pe_k23")
LEFT, RIGHT = os.path.join(FX, "ref", "reads_1.cor.fq"), os.path.join(FX, "ref", "reads_2.cor.fq")
K = 23


@pytest.fixture(scope="module")
def tool():
    loader = importlib.machinery.SourceFileLoader("read_screen", TOOL)
    spec = importlib.util.spec_from_loader("read_screen", loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


def run_tool(args):
    return subprocess.run([sys.executable, TOOL] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def names_of(path):
    return [ln.split()[0][1:] for ln in open(path, "rb").read().split(b"\n")[0::4] if ln]


def expected(units, counts, min_count, min_pct, screen_kmers):
    """(report, per-read file, flagged file, stderr line) for units of (name, sequence) mates, from the restatement"""
    mates = len(units[0])
    rows = [[restate(seq, K, counts, min_count) for _, seq in u] for u in units]
    per_read = b"".join(name + b"\t" + ("%d\t%d\t%d\t%d\n" % r).encode() for u, rs in zip(units, rows) for (name, _), r in zip(u, rs))
    tot = lambda f: [sum(f(rs[m]) for rs in rows) for m in range(mates)]   # noqa: E731
    pct_of = lambda r: 100 * r[1] // r[0]   # noqa: E731
    flag = lambda r: r[0] > 0 and pct_of(r) >= min_pct   # noqa: E731
    lines = ["k\t%d" % K, "min_count\t%d" % min_count, "min_pct\t%d" % min_pct, "screen_kmers\t%d" % screen_kmers]
    for key, f in (("reads", lambda r: 1), ("novalid", lambda r: r[0] == 0), ("hitreads", lambda r: r[1] > 0), ("flagged", flag)):
        lines += ["%s\t%d\t%d" % (key, m + 1, n) for m, n in enumerate(tot(f))]
    ps = sorted({pct_of(r) for rs in rows for r in rs if r[0] > 0})
    lines += ["pct\t%d\t%s" % (p, "\t".join("%d" % n for n in tot(lambda r: r[0] > 0 and pct_of(r) == p))) for p in ps]
    flagged = [u[0][0] for u, rs in zip(units, rows) if any(flag(r) for r in rs)]
    if mates == 2:
        best = [max(pct_of(r) for r in rs if r[0] > 0) for rs in rows if any(r[0] > 0 for r in rs)]
        lines += ["pairs\t%d" % len(units), "pairs_flagged\t%d" % len(flagged)]
        lines += ["pairmax\t%d\t%d" % (p, best.count(p)) for p in sorted(set(best))]
    n_reads, n_hit = mates * len(units), sum(r[1] > 0 for rs in rows for r in rs)
    err = "read_screen: %d reads, %d with a hit; %d of %d %s flagged (%.2f %%)" % (
        n_reads, n_hit, len(flagged), len(units), "pairs" if mates == 2 else "reads", 100.0 * len(flagged) / len(units))
    return "\n".join(lines) + "\n", per_read, b"".join(n + b"\n" for n in flagged), err


def check_run(args, units, counts, min_count, min_pct, tmp_path, tag):
    out, per, fl = (str(tmp_path / ("%s.%s" % (tag, x))) for x in ("report", "per_read", "flagged"))
    p = run_tool(args + ["-o", out, "-per-read", per, "-flagged", fl])
    assert p.returncode == 0, p.stderr.decode()
    report, per_read, flagged, err = expected(units, counts, min_count, min_pct, len(counts))
    assert open(out).read() == report
    assert open(per, "rb").read() == per_read
    assert open(fl, "rb").read() == flagged
    assert p.stderr.decode().splitlines()[-1] == err and p.stdout == b""
    return report, flagged


# ---- CPU -------------------------------------------------------------------------------------------------------------------
DUMP = os.path.join(FX, "dump.jf")
BAD_ARGS = [
    ([], "-k is required"),
    (["-k", "23", "-r", LEFT], "the screen set: give either"),
    (["-k", "23", "-s", DUMP, "-s-seq", LEFT, "-r", LEFT], "the screen set: give either"),
    (["-k", "23", "-s", DUMP], "the reads: give one of"),
    (["-k", "23", "-s", DUMP, "-r", LEFT, "-i", LEFT], "the reads: give one of"),
    (["-k", "23", "-s", DUMP, "-p", LEFT], "-p takes files two at a time"),
    (["-k", "23", "-s", DUMP, "-p", LEFT, RIGHT, LEFT], "-p takes files two at a time"),
    (["-k", "23", "-s", DUMP, "-r", LEFT, "-min-pct", "101"], "-min-pct must be 0..100"),
    (["-k", "23", "-s", DUMP, "-r", LEFT, "-min-pct", "-1"], "-min-pct must be 0..100"),
    (["-k", "23", "-s", DUMP, "-r", LEFT, "-min-count", "0"], "-min-count must be at least 1"),
    (["-k", "23", "-s", DUMP, "-r", LEFT, "-batch", "0"], "-batch must be at least 1"),
    (["-k", "40", "-s", DUMP, "-r", LEFT], "-k must be 1..32"),
    (["-k", "23", "-s", DUMP, "-r", "/nonexistent/reads.fq"], "cannot read /nonexistent/reads.fq"),
    (["-k", "23", "-s", DUMP, "-r", LEFT, "-frobnicate", "1"], "unknown option -frobnicate"),
    (["-k", "23", "-s", DUMP, "-r", LEFT, "-o"], "-o needs a value"),
]


@pytest.mark.parametrize("args,text", BAD_ARGS, ids=["%d %s" % (i, t) for i, (_, t) in enumerate(BAD_ARGS)])
def test_usage_errors(tool, args, text):
    with pytest.raises(tool.UsageError, match=text):
        tool.parse_args(args)


def test_usage_errors_exit_non_zero_with_one_line():
    for args, text in (BAD_ARGS[0], BAD_ARGS[5], BAD_ARGS[7]):
        p = run_tool(args)
        err = p.stderr.decode()
        assert p.returncode != 0 and p.stdout == b"" and err.count("\n") == 1 and text in err and "usage: read_screen -k INT" in err


def test_the_tally_of_hand_made_rows(tool):
    t = tool.Tally(2, 50)
    assert t.add([(10, 5, 30, 3), (0, 0, 0, 0)]) and not t.add([(10, 4, 30, 3), (9, 0, 0, 0)]) and not t.add([(0, 0, 0, 0), (0, 0, 0, 0)])
    assert t.report(23, 1, 7) == ("k\t23\nmin_count\t1\nmin_pct\t50\nscreen_kmers\t7\nreads\t1\t3\nreads\t2\t3\nnovalid\t1\t1\nnovalid\t2\t2\n"
                                  "hitreads\t1\t2\nhitreads\t2\t0\nflagged\t1\t1\nflagged\t2\t0\npct\t0\t0\t1\npct\t40\t1\t0\npct\t50\t1\t0\n"
                                  "pairs\t3\npairs_flagged\t1\npairmax\t40\t1\npairmax\t50\t1\n")
    assert t.summary_line() == "read_screen: 6 reads, 2 with a hit; 1 of 3 pairs flagged (33.33 %)"


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_paired_and_single_end_runs_equal_the_restatement(tmp_path):
    seqs1, seqs2 = fastx_seqs(LEFT)[0], fastx_seqs(RIGHT)[0]
    names1, names2 = names_of(LEFT), names_of(RIGHT)
    pairs = [((a, s), (b, t)) for a, s, b, t in zip(names1, seqs1, names2, seqs2)]
    # the screen set: every fifth first mate as multi-line FASTA wrapped at 60, one record with an N in it
    picked = [bytes(s) for s in seqs1[::5]]
    picked[3] = picked[3][:40] + b"N" + picked[3][41:]
    fasta = tmp_path / "screen.fa"
    with open(fasta, "wb") as f:
        for i, s in enumerate(picked):
            f.write(b">set%d some words\n" % i + b"".join(s[j:j + 60] + b"\n" for j in range(0, len(s), 60)))
    counts = counts_of_reads(picked, K)
    assert max(len(s) for s in picked) > 60
    report, flagged = check_run(["-k", str(K), "-s-seq", str(fasta), "-p", LEFT, RIGHT, "-batch", "128"], pairs, counts, 1, 50, tmp_path, "pe")
    assert 0 < len(flagged.split()) < len(pairs) and "\npct\t100\t" in report and "\npct\t0\t" in report and len(pairs) * 2 > 3 * 128
    # the same through a dump (counts of 2 and more), single-end, other thresholds, a batch size that does not divide the file
    kept = {c: n for c, n in counts.items() if n >= 2}
    assert 0 < len(kept) < len(counts)
    dump = tmp_path / "screen.jf"
    text = {}
    for s in picked:
        for i in range(len(s) - K + 1):
            w = s[i:i + K]
            if b"N" not in w and canonical(w) in kept:
                text[canonical(w)] = w
    with open(dump, "wb") as f:
        for c in sorted(text):
            f.write(b">%d\n%s\n" % (kept[c], text[c]))
    singles = [((a, s),) for a, s in zip(names2, seqs2)]
    report, flagged = check_run(["-k", str(K), "-s", str(dump), "-r", RIGHT, "-batch", "77", "-min-count", "3", "-min-pct", "10"], singles, kept, 3, 10,
                                tmp_path, "se")
    assert 0 < len(flagged.split()) < len(singles)
    p = run_tool(["-k", str(K), "-s", str(dump), "-r", RIGHT, "-min-pct", "0"])           # the report on stdout; p >= 0: every read with a valid window
    assert p.returncode == 0 and p.stdout.decode() == expected(singles, kept, 1, 0, len(kept))[0]
