"""GPU: tools/read_merge end to end on tests/golden/fx_pe_k23 and on a small overlapping set written here -- -p and -i, FASTQ and
FASTA, plain and .gz, -batch below and above the input's size: the merged and unmerged files, the report and the -list lines
equal, byte for byte, what tests/merge_model.py gives."""
import gzip
import importlib.machinery
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import merge_model as mm
import trim_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "read_merge")
FX = os.path.join(ROOT, "tests", "golden", "fx_pe_k23")
N_PAIRS = 150


@pytest.fixture(scope="module")
def tool():
    loader = importlib.machinery.SourceFileLoader("read_merge", TOOL)
    spec = importlib.util.spec_from_loader("read_merge", loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


def make_pairs():
    """(name line, sequence, + line, quality) of both mates of N_PAIRS pairs: fragments shorter and longer than the mates and too
    long to overlap, a few disagreements in mate 1, an N and a lower-case base here and there, noisy qualities"""
    rng = np.random.default_rng(23)
    out = []
    for n in range(N_PAIRS):
        La, Lb = (int(x) for x in rng.integers(40, 121, 2))
        F = int(rng.integers(30, 260))
        a, b = tc.pair_of(rng, F, La, Lb, tail=tc.AD + b"CTAGGCATTACG")
        a = bytearray(a)
        for j in set(rng.integers(0, La, int(rng.integers(0, 3))).tolist()):
            a[j] = b"ACGT"[(b"ACGT".index(a[j]) + 1) % 4]
        a = bytes(a)
        if n % 7 == 0:
            a = a[:11] + b"N" + a[12:]
        if n % 11 == 0:
            b = b[:5] + b[5:8].lower() + b[8:]
        out.append(((b"@p%d/1 left of %d\n" % (n, n), a, b"+\n", tc.rand_qual(rng, La, 2, 41)), (b"@p%d/2\n" % n, b, b"+p%d/2\n" % n, tc.rand_qual(rng, Lb, 2, 41))))
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


def expected(pairs, fq, **kw):
    """the merged text, the unmerged text per mate, the report and the list lines of `pairs` by the model; FASTA records come
    back out with their sequence on one line"""
    p = mm.params(**kw)
    seqs = [m[1] for pr in pairs for m in pr]
    quals = [m[3] for pr in pairs for m in pr] if fq else None
    rows, moff, mseq, mqual, t = mm.merge_batch(seqs, quals, 2, p)
    merged, un, listing = b"", [b"", b""], b""
    rec = (lambda h, s, plus, q: h + s + b"\n" + plus + q + b"\n") if fq else (lambda h, s, plus, q: b">" + h[1:] + s + b"\n")
    for u, pr in enumerate(pairs):
        F, d, v, m = (int(x) for x in rows[u])
        listing += pr[0][0][1:].split()[0] + (" %d %d %d %d %d %d\n" % (len(pr[0][1]), len(pr[1][1]), d, v, m, F)).encode()
        if F:
            s = mseq[moff[u]:moff[u + 1] - 1]
            merged += (pr[0][0] + s + b"\n+\n" + mqual[moff[u]:moff[u + 1] - 1] + b"\n") if fq else (b">" + pr[0][0][1:] + s + b"\n")
        else:
            un = [un[j] + rec(*pr[j]) for j in range(2)]
    rep = [("overlap_min", p["min_overlap"]), ("overlap_mm", p["max_mismatch_pct"]), ("qual_base", p["qual_base"]), ("qual_cap", p["qual_cap"])]
    rep += [(k, t[k]) for k in ("pairs", "merged", "unmerged", "readthrough", "compared", "mismatches")]
    rep += [("took", 1, t["took_mate1"]), ("took", 2, t["took_mate2"]), ("took", "tie", t["ties"])]
    rep += [("len", n, t["len_hist"][n]) for n in range(mm.LEN_BINS) if t["len_hist"][n]]
    return merged, un, "".join("\t".join(str(x) for x in line) + "\n" for line in rep), listing, t


def run_tool(tool, args, od, capsys):
    rep, lst = os.path.join(od, "report.txt"), os.path.join(od, "list.txt")
    assert tool.main(args + ["-od", od, "-o", rep, "-list", lst]) == 0
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and err.startswith("read_merge: ")
    return open(rep).read(), open(lst, "rb").read(), err


def read(od, name):
    return open(os.path.join(od, name), "rb").read()


@pytest.mark.parametrize("kind", ["fq", "fq.gz", "fa", "fa.gz"])
def test_paired_and_interleaved_input_equal_the_model(tool, pairs, kind, tmp_path, capsys):
    fq = kind.startswith("fq")
    text = fastq if fq else fasta
    left, right = [p[0] for p in pairs], [p[1] for p in pairs]
    f1, f2 = write(tmp_path / ("s_1." + kind), text(left)), write(tmp_path / ("s_2." + kind), text(right))
    fi = write(tmp_path / ("both." + kind), text([m for p in pairs for m in p]))
    ext = ".fq" if fq else ".fa"
    want_m, want_un, want_rep, want_list, t = expected(pairs, fq)
    assert 30 < t["merged"] < N_PAIRS - 30 and t["readthrough"] > 10 and t["mismatches"] > 10 and (not fq or (t["took_mate1"] and t["took_mate2"])) and (fq or t["ties"])
    outs = []
    for batch in (37, 1000):       # -p, with a batch smaller than the input and one larger
        od = str(tmp_path / ("p%d" % batch))
        rep, lst, err = run_tool(tool, ["-p", f1, f2, "-batch", str(batch)], od, capsys)
        got = (read(od, "s_1.merged" + ext), read(od, "s_1.unmerged" + ext), read(od, "s_2.unmerged" + ext))
        assert got == (want_m, want_un[0], want_un[1]) and rep == want_rep and lst == want_list
        assert not os.path.exists(os.path.join(od, "s_2.merged" + ext)) and "%d pairs, %d merged" % (N_PAIRS, t["merged"]) in err
        outs.append((got, rep, lst))
    assert outs[0] == outs[1]
    # -i: the same pairs in one file; the unmerged file keeps both mates
    od = str(tmp_path / "i")
    rep, lst, _ = run_tool(tool, ["-i", fi, "-batch", "64"], od, capsys)
    rec = (lambda h, s, plus, q: h + s + b"\n" + plus + q + b"\n") if fq else (lambda h, s, plus, q: b">" + h[1:] + s + b"\n")
    rows = mm.merge_batch([m[1] for p in pairs for m in p], [m[3] for p in pairs for m in p] if fq else None, 2, mm.params())[0]
    want_i = b"".join(rec(*m) for n, p in enumerate(pairs) if rows[n][0] == 0 for m in p)
    assert read(od, "both.merged" + ext) == want_m and read(od, "both.unmerged" + ext) == want_i and rep == want_rep and lst == want_list
    # other parameters
    want_m, want_un, want_rep, want_list, t2 = expected(pairs, fq, min_overlap=15, max_mismatch_pct=2, qual_cap=60)
    od = str(tmp_path / "q")
    rep, lst, _ = run_tool(tool, ["-p", f1, f2, "-overlap-min", "15", "-overlap-mm", "2", "-qual-cap", "60"], od, capsys)
    assert (read(od, "s_1.merged" + ext), read(od, "s_1.unmerged" + ext), read(od, "s_2.unmerged" + ext)) == (want_m, want_un[0], want_un[1])
    assert rep == want_rep and lst == want_list and t2["merged"] != t["merged"]


def test_the_golden_pairs_and_the_command_itself(tmp_path):
    """tests/golden/fx_pe_k23 through the command: the report on stdout, one line of the tool's own on stderr"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kmer_sets import read_raw_records
    left, right = os.path.join(FX, "reads_1.fq"), os.path.join(FX, "reads_2.fq")
    recs = list(zip(read_raw_records(left), read_raw_records(right)))
    quals = [m[2].split(b"\n")[3] for pr in recs for m in pr]
    p = mm.params(min_overlap=20)
    rows, moff, mseq, mqual, t = mm.merge_batch([m[1] for pr in recs for m in pr], quals, 2, p)
    od = str(tmp_path / "o")
    r = subprocess.run([sys.executable, TOOL, "-p", left, right, "-overlap-min", "20", "-od", od, "-list", str(tmp_path / "l.txt")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    own = [ln for ln in r.stderr.decode().splitlines() if ln.startswith("read_merge: ")]       # (the GPU runtime may write lines of its own)
    assert r.returncode == 0 and len(own) == 1 and own[0].startswith("read_merge: %d pairs, %d merged" % (len(recs), t["merged"]))
    out = r.stdout.decode()
    assert out.startswith("overlap_min\t20\noverlap_mm\t10\nqual_base\t33\nqual_cap\t41\npairs\t%d\nmerged\t%d\nunmerged\t%d\n" % (len(recs), t["merged"], t["unmerged"]))
    assert "took\t1\t%d\ntook\t2\t%d\ntook\ttie\t%d\n" % (t["took_mate1"], t["took_mate2"], t["ties"]) in out
    want_m = b"".join(pr[0][2][:pr[0][2].index(b"\n") + 1] + mseq[moff[u]:moff[u + 1] - 1] + b"\n+\n" + mqual[moff[u]:moff[u + 1] - 1] + b"\n"
                      for u, pr in enumerate(recs) if rows[u][0])
    assert read(od, "reads_1.merged.fq") == want_m
    assert read(od, "reads_1.unmerged.fq") == b"".join(pr[0][2] for u, pr in enumerate(recs) if not rows[u][0])
    assert read(od, "reads_2.unmerged.fq") == b"".join(pr[1][2] for u, pr in enumerate(recs) if not rows[u][0])
    assert t["pairs"] == len(recs) > 100 and t["merged"] + t["unmerged"] == t["pairs"]
    print("fx_pe_k23: %d pairs, %d merged, %d read through, %d mismatches" % (t["pairs"], t["merged"], t["readthrough"], t["mismatches"]))
    # a read that is too long is refused by name
    f = write(tmp_path / "long.fa", b">fine\nACGT\n>toolong\n" + b"A" * 1024 + b"\n")
    r = subprocess.run([sys.executable, TOOL, "-i", f, "-od", od], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    own = [ln for ln in r.stderr.decode().splitlines() if ln.startswith("read_merge: ")]
    assert r.returncode == 1 and r.stdout == b"" and own == ["read_merge: read toolong of 1024 bases exceeds the library's 1023"]
