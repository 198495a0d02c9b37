"""GPU: tools/read_trim end to end on small generated files -- -r, -p and -i, FASTQ and FASTA, plain and .gz, -batch below and
above the input's size: the output files, the report and the -list lines equal, byte for byte, what the cuts of
tests/trim_model.py give."""
import gzip
import importlib.machinery
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import trim_cases as tc
import trim_model as tm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "read_trim")
N_PAIRS = 150


@pytest.fixture(scope="module")
def tool():
    loader = importlib.machinery.SourceFileLoader("read_trim", TOOL)
    spec = importlib.util.spec_from_loader("read_trim", loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


def make_pairs():
    """(name line, sequence, + line, quality) of both mates of N_PAIRS pairs: fragments shorter and longer than the mates, the
    adapter behind a fragment that is run through, noisy 3' qualities, an N and a lower-case base here and there"""
    rng = np.random.default_rng(17)
    out = []
    for n in range(N_PAIRS):
        La, Lb = (int(x) for x in rng.integers(30, 121, 2))
        F = int(rng.integers(20, 200))
        a, b = tc.pair_of(rng, F, La, Lb, tail=tc.AD + b"CTAGGCATTACG")
        if n % 7 == 0:
            a = a[:11] + b"N" + a[12:]
        if n % 11 == 0:
            b = b[:5] + b[5:8].lower() + b[8:]
        qa = tc.rand_qual(rng, La, 20, 41)[:La - La // 4] + tc.rand_qual(rng, La // 4, 2, 35)
        qb = tc.rand_qual(rng, Lb, 2, 41)
        out.append(((b"@p%d/1 left of %d\n" % (n, n), a, b"+\n", qa), (b"@p%d/2\n" % n, b, b"+p%d/2\n" % n, qb)))
    return out


@pytest.fixture(scope="module")
def pairs():
    return make_pairs()


def fastq(recs):
    return b"".join(h + s + b"\n" + plus + q + b"\n" for h, s, plus, q in recs)


def fasta(recs, width=50):
    return b"".join(b">" + h[1:] + b"".join(s[i:i + width] + b"\n" for i in range(0, len(s), width)) for h, s, _, _ in recs)


def write(path, data):
    with (gzip.open(path, "wb") if str(path).endswith(".gz") else open(path, "wb")) as f:
        f.write(data)
    return str(path)


def expected(units, fq, o):
    """the output text per mate, the report and the list lines of `units` (tuples of records) by the model"""
    p = tm.params(qual_min=o.get("q", 20), adapter1=o.get("a", tc.AD), adapter2=o.get("a2"), pair_overlap=o.get("pair", True), min_len=o.get("min_len", 20),
                  adapter_min=o.get("adapter_min", 5))
    mates = len(units[0])
    seqs = [r[1] for u in units for r in u]
    quals = [r[3] for u in units for r in u] if fq else None
    rows, keep, t = tm.trim_batch(seqs, quals, 0 if mates == 1 else 2, p)
    texts, listing = [b""] * mates, b""
    for n, u in enumerate(units):
        for j, (h, s, plus, q) in enumerate(u):
            kl = int(rows[mates * n + j][0])
            listing += h[1:].split()[0] + (" %d %d %d %d %d\n" % ((len(s),) + tuple(rows[mates * n + j]))).encode()
            if keep[n]:
                texts[j] += (h + s[:kl] + b"\n" + plus + q[:kl] + b"\n") if fq else (b">" + h[1:] + s[:kl] + b"\n")
    rep = [("q", p["qual_min"]), ("qual_base", 33), ("adapter1", p["adapter1"].decode()), ("adapter2", p["adapter2"].decode()), ("adapter_min", p["adapter_min"]),
           ("adapter_mm", 10), ("pair_overlap", int(p["pair_overlap"] and mates == 2)), ("overlap_min", 30), ("overlap_mm", 10), ("min_len", p["min_len"]),
           ("units", len(units), "pairs" if mates == 2 else "reads"), ("kept", int(keep.sum())), ("short", len(units) - int(keep.sum()))]
    for m in range(mates):
        rep += [("reads", m + 1, t["reads"][m])] + [("cut", m + 1, c, t["cut_reads"][m][x]) for x, c in enumerate(("quality", "adapter", "pair"))]
        rep.append(("bases_removed", m + 1, t["bases_removed"][m]))
    rep.append(("pairs_overlapping", t["pairs_overlapping"]))
    for m in range(mates):
        rep += [("len", m + 1, n, t["keep_hist"][m][n]) for n in range(1024) if t["keep_hist"][m][n]]
    return texts, "".join("\t".join(str(x) for x in line) + "\n" for line in rep), listing, t


def run_tool(tool, args, od, capsys):
    rep, lst = os.path.join(od, "report.txt"), os.path.join(od, "list.txt")
    assert tool.main(args + ["-od", od, "-o", rep, "-list", lst]) == 0
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and err.startswith("read_trim: ")
    return open(rep).read(), open(lst, "rb").read(), err


@pytest.mark.parametrize("kind", ["fq", "fq.gz", "fa", "fa.gz"])
def test_single_paired_and_interleaved_input_equal_the_model(tool, pairs, kind, tmp_path, capsys):
    fq = kind.startswith("fq")
    text = fastq if fq else fasta
    left, right = [p[0] for p in pairs], [p[1] for p in pairs]
    inter = [m for p in pairs for m in p]
    f1, f2 = write(tmp_path / ("s_1." + kind), text(left)), write(tmp_path / ("s_2." + kind), text(right))
    fi = write(tmp_path / ("both." + kind), text(inter))
    ext = ".trim.fq" if fq else ".trim.fa"
    # -p, with a batch smaller than the input and one larger
    want_texts, want_rep, want_list, t = expected(pairs, fq, {})
    outs = []
    for batch in (37, 1000):
        od = str(tmp_path / ("p%d" % batch))
        rep, lst, err = run_tool(tool, ["-p", f1, f2, "-batch", str(batch)], od, capsys)
        got = [open(os.path.join(od, "s_%d%s" % (m, ext)), "rb").read() for m in (1, 2)]
        assert got == want_texts and rep == want_rep and lst == want_list
        assert got[0].count(b"\n") == got[1].count(b"\n") == (4 if fq else 2) * t["units_kept"]          # the files stay in step
        assert "%d pairs, %d kept" % (N_PAIRS, t["units_kept"]) in err
        outs.append((got, rep, lst))
    assert outs[0] == outs[1]
    assert 0 < t["units_kept"] and (t["units_kept"] < N_PAIRS or not fq) and t["pairs_overlapping"] > 20 and (t["cut_reads"][:, 1:] > 0).all() and (not fq or (t["cut_reads"][:, 0] > 0).all())
    # -i: the same pairs in one file
    od = str(tmp_path / "i")
    rep, lst, _ = run_tool(tool, ["-i", fi, "-batch", "64"], od, capsys)
    rec = (lambda h, s, plus, q, kl: h + s[:kl] + b"\n" + plus + q[:kl] + b"\n") if fq else (lambda h, s, plus, q, kl: b">" + h[1:] + s[:kl] + b"\n")
    rows, keep, _ = tm.trim_batch([m[1] for m in inter], [m[3] for m in inter] if fq else None, 2, tm.params())
    want_i = b"".join(rec(*m, int(rows[2 * n + j][0])) for n, p in enumerate(pairs) if keep[n] for j, m in enumerate(p))
    assert open(os.path.join(od, "both" + ext), "rb").read() == want_i and rep == want_rep and lst == want_list
    # -r over both files: single reads, no pair cut, a short mate drops nobody else; its own adapter for every read
    units = [(m,) for m in left + right]
    want_texts, want_rep, want_list, t = expected(units, fq, {"a": b"AGATCGGAAG", "min_len": 31, "q": 25})
    od = str(tmp_path / "r")
    rep, lst, _ = run_tool(tool, ["-r", f1, f2, "-batch", "100", "-a", "AGATCGGAAG", "-min-len", "31", "-q", "25"], od, capsys)
    got = b"".join(open(os.path.join(od, "s_%d%s" % (m, ext)), "rb").read() for m in (1, 2))
    assert got == want_texts[0] and rep == want_rep and lst == want_list and t["pairs_overlapping"] == 0


def test_every_cut_switched_off_returns_the_records_unchanged(tool, pairs, tmp_path, capsys):
    left, right = [p[0] for p in pairs], [p[1] for p in pairs]
    f1, f2 = write(tmp_path / "s_1.fq", fastq(left)), write(tmp_path / "s_2.fq.gz", fastq(right))
    od = str(tmp_path / "off")
    rep, lst, _ = run_tool(tool, ["-p", f1, f2, "-a", "", "-q", "0", "-no-pair-overlap", "-min-len", "0"], od, capsys)
    assert open(os.path.join(od, "s_1.trim.fq"), "rb").read() == fastq(left) and open(os.path.join(od, "s_2.trim.fq"), "rb").read() == fastq(right)
    assert "kept\t%d\n" % N_PAIRS in rep and "short\t0\n" in rep and "adapter1\t\n" in rep and "pair_overlap\t0\n" in rep
    assert all(ln.split()[1] == ln.split()[2] == ln.split()[3] == ln.split()[4] == ln.split()[5] for ln in lst.decode().splitlines())


def test_the_command_itself_and_a_read_that_is_too_long(pairs, tmp_path):
    f1 = write(tmp_path / "one.fq", fastq([pairs[0][0], pairs[1][0]]))
    p = subprocess.run([sys.executable, TOOL, "-r", f1, "-od", str(tmp_path / "o")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    own = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("read_trim: ")]       # (the GPU runtime may write lines of its own)
    assert p.returncode == 0 and len(own) == 1 and own[0].startswith("read_trim: 2 reads, ") and p.stderr.decode().endswith(own[0] + "\n")
    assert p.stdout.decode().startswith("q\t20\nqual_base\t33\nadapter1\tAGATCGGAAGAGC\n") and "units\t2\treads\n" in p.stdout.decode()
    assert os.path.isfile(str(tmp_path / "o" / "one.trim.fq"))
    f2 = write(tmp_path / "long.fa", b">fine\nACGT\n>toolong\n" + b"A" * 1024 + b"\n")
    p = subprocess.run([sys.executable, TOOL, "-r", f2, "-od", str(tmp_path / "o")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    own = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("read_trim: ")]
    assert p.returncode == 1 and p.stdout == b"" and own == ["read_trim: read toolong of 1024 bases exceeds the library's 1023"]
