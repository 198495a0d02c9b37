"""GPU: the k-mer count spectrum (`jellyfish histo` of the counts) -- rc_table_count_spectrum / rc_table_spectrum, the
binding's count_spectrum / kmer_spectrum, and `rcorrector -histo`.

  * counted: every canonical k-mer the counter saw, those below min_count (the count-1 bin) included, in one pass, in
    tens of passes, with arrays regrown at every pass and sharded over several contexts == numpy's np.unique counts
  * table: the live entries of every kind of table (counted, a loaded dump, WIDE / PACKED, remainder bits above the
    count, the overflow prefix, the absence filter, shared, replicated) == bincount of rc_table_export's counts
  * the bins above max_bin fold into the last one; the statistics are exact whatever max_bin is
  * `rcorrector -histo` writes "<count> <frequency>" lines and changes no other byte of the run
Expectations come from numpy over the reads or over the exported table; nothing here reads the reference.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import synth

pytestmark = pytest.mark.gpu
CLI = os.path.join(gu.ROOT, "rcorrector_amd", "rcorrector")
EXACT_DUMP_FIXTURES = ["fx_sample", "fx_se_k23", "fx_pe_k23", "fx_il_k23", "fx_k31_mc8", "fx_skew", "fx_k32", "fx_k15", "fx_varlen_n"]
MAX_BINS = [1, 2, 7, 10000, 1 << 20]


@pytest.fixture(scope="module")
def rc():
    import rcorrector_amd
    return rcorrector_amd


def spectrum(counts, max_bin):
    """freq[max_bin + 1] and the four statistics of a list of per-k-mer counts"""
    c = np.asarray(counts, dtype=np.int64)
    f = np.bincount(np.minimum(c, max_bin), minlength=max_bin + 1).astype(np.uint64)
    f[0] = 0
    st = {"distinct": len(c), "total": int(c.sum()), "unique": int((c == 1).sum()), "max_count": int(c.max()) if len(c) else 0}
    return f, st


def assert_spectrum(got, counts, max_bin):
    f, st = spectrum(counts, max_bin)
    assert got[0].dtype == np.uint64 and len(got[0]) == max_bin + 1
    assert np.array_equal(got[0], f), "bins differ at %s" % np.nonzero(got[0] != f)[0][:10]
    assert got[1] == st


def arena_of(rows):
    return b"".join(bytes(r) + b"\0" for r in rows)


def all_counts(codes):
    return np.unique(np.asarray(codes, dtype=np.uint64), return_counts=True)[1]


def reads_with_a_deep_kmer(seed, k):
    """ragged reads with N, plus 200 poly-A reads: one k-mer counted > 16384 times (the bins beyond what LDS holds)"""
    s1, _, s2, _, lens = synth.make_reads(seed, 3000, 120, n_tx=8, l_tx=600, e=0.01, p_n=0.003, paired=True, var_len=True)
    rows = [s1[i, :lens[i]] for i in range(len(s1))] + [s2[i, :lens[i]] for i in range(len(s2))]
    polya = np.full((200, 120), ord("A"), dtype=np.uint8)
    rows += [polya[i] for i in range(len(polya))]
    codes = np.concatenate([synth.canonical_codes(s1, k, lens), synth.canonical_codes(s2, k, lens), synth.canonical_codes(polya, k)])
    return rows, all_counts(codes)


def count_in_pieces(ctx, rows, min_count):
    """count_begin, ragged host and device arenas (one empty), count_finish"""
    import torch
    ctx.count_begin()
    cuts = [0, 1, 1, 700, 2500, 2501, len(rows)]
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        ar = arena_of(rows[a:b])
        if i % 2:
            t = torch.frombuffer(bytearray(ar), dtype=torch.uint8).cuda() if ar else torch.zeros(0, dtype=torch.uint8, device="cuda")
            ctx.count_add_device(t, len(ar))
            torch.cuda.synchronize()
        else:
            ctx.count_add(ar)
    return ctx.count_finish(min_count)


@pytest.mark.parametrize("k", [15, 23, 31, 32])
def test_counted_spectrum_equals_numpy(rc, k):
    rows, cnt = reads_with_a_deep_kmer(500 + k, k)
    assert (cnt == 1).sum() > 1000 and cnt.max() > 16384
    ctx = rc.Context(k=k)
    for i, mb in enumerate(MAX_BINS):
        min_count = 2 if i % 2 else 5
        ctx.count_spectrum(mb)
        n = count_in_pieces(ctx, rows, min_count)
        assert n == (cnt >= min_count).sum()
        assert_spectrum(ctx.kmer_spectrum("counted", mb), cnt, mb)
    for mb in MAX_BINS:   # the last count was armed with 1 << 20: every lower bound folds from it
        assert_spectrum(ctx.kmer_spectrum("counted", mb), cnt, mb)
    # the table holds the counts >= min_count: its spectrum is the counted one with the lower bins zeroed
    t = ctx.kmer_spectrum("table", 10000)
    want = ctx.kmer_spectrum("counted", 10000)[0].copy()
    want[:min_count] = 0
    assert np.array_equal(t[0], want)
    assert_spectrum(t, ctx.table_export()[1], 10000)
    ctx.close()


@pytest.mark.parametrize("env", [{"RC_COUNT_MEM_MB": "1"}, {"RC_COUNT_MEM_MB": "1", "RC_COUNT_TIGHT": "1"}, {"RC_COUNT_TIGHT": "1"}])
def test_counted_spectrum_over_many_passes(rc, env, monkeypatch):
    k = 31
    s1, _, _, _, _ = synth.make_reads(4100, 10000, 150, n_tx=6, l_tx=900, e=0.05)
    cnt = all_counts(synth.canonical_codes(s1, k))
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    ctx = rc.Context(k=k)
    ctx.count_spectrum(10000)
    ctx.count_begin()
    rows = [s1[i] for i in range(len(s1))]
    for lo in range(0, len(rows), 2500):
        ctx.count_add(arena_of(rows[lo:lo + 2500]))
    ctx.count_finish(2)
    assert_spectrum(ctx.kmer_spectrum("counted", 10000), cnt, 10000)
    assert_spectrum(ctx.kmer_spectrum("counted", 7), cnt, 7)
    ctx.close()


@pytest.mark.parametrize("n_ctx,mem_mb", [(2, None), (3, 1), (8, 1)])
def test_sharded_counted_spectrum_equals_one_context(rc, n_ctx, mem_mb, monkeypatch):
    k = 31
    s1, _, _, _, _ = synth.make_reads(4200, 9000, 150, n_tx=6, l_tx=900, e=0.03)
    cnt = all_counts(synth.canonical_codes(s1, k))
    if mem_mb is not None:
        monkeypatch.setenv("RC_COUNT_MEM_MB", str(mem_mb))
    rows = [s1[i] for i in range(len(s1))]
    pieces = [arena_of(rows[lo:lo + 1000]) for lo in range(0, len(rows), 1000)]
    one = rc.Context(k=k)
    one.count_spectrum(10000)
    one.count_begin()
    for a in pieces:
        one.count_add(a)
    one.count_finish(2)
    ctxs = [rc.Context(k=k) for _ in range(n_ctx)]
    ctxs[0].count_spectrum(10000)   # (ctxs[0]'s setting applies to every context)
    for c in ctxs:
        c.count_begin()
    for i, a in enumerate(pieces):
        ctxs[(i * 3) % n_ctx if n_ctx < 8 else i % (n_ctx - 1)].count_add(a)
    ctxs[0].count_finish_sharded(ctxs[1:])
    got = ctxs[0].kmer_spectrum("counted", 10000)
    want = one.kmer_spectrum("counted", 10000)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    assert_spectrum(got, cnt, 10000)
    for c in ctxs + [one]:
        c.close()


def table_spectrum_equals_export(ctx, max_bins=(2, 7, 10000, 1 << 20)):
    counts = ctx.table_export()[1]
    for mb in max_bins:
        assert_spectrum(ctx.kmer_spectrum("table", mb), counts, mb)
    return counts


@pytest.mark.parametrize("name", [n for n in gu.FIXTURES if os.path.exists(os.path.join(gu.GOLDEN, n, "dump.jf"))])
def test_table_spectrum_of_golden_dumps(rc, name):
    d = os.path.join(gu.GOLDEN, name)
    args = open(os.path.join(d, "cmd.txt")).read().split()
    ctx = rc.Context(k=int(args[args.index("-k") + 1]))
    ctx.load_jfdump(os.path.join(d, "dump.jf"))
    table_spectrum_equals_export(ctx, (2, 10000))
    ctx.close()


def skewed_table(k, n, seed, big=()):
    rng = np.random.default_rng(seed)
    codes = np.unique(rng.integers(0, 1 << min(2 * k, 63), size=n, dtype=np.uint64))
    counts = np.minimum(2 + rng.zipf(1.6, size=len(codes)), 400000).astype(np.int32)
    for i, c in enumerate(big):
        counts[i] = c
    return codes, counts


@pytest.mark.parametrize("k,n,load,layout,filt", [(23, 200000, None, "wide", None), (23, 200000, None, "packed", None),
                                                  (31, 1200000, "0.06", "packed", None), (31, 200000, None, "wide", None),
                                                  (23, 200000, None, "packed", "force"), (32, 4200000, "0.06", "packed", "force")])
def test_table_spectrum_of_built_tables(rc, k, n, load, layout, filt, monkeypatch):
    """WIDE and PACKED slots; k = 31 / 32 with 8 remainder bits above the count (ext > 0, at a low load: the smallest
    table that keeps PACKED), so counts from 2^19 up go to the overflow prefix, as 2^27 + 5 does at ext = 0; the absence
    filter behind the buckets; duplicate keys (the later Put wins)"""
    if layout == "wide":
        monkeypatch.setenv("RC_TABLE_LAYOUT", "wide")
    if filt:
        monkeypatch.setenv("RC_TABLE_FILTER", filt)
    if load:
        monkeypatch.setenv("RC_TABLE_LOAD", load)
    codes, counts = skewed_table(k, n, k, big=(3_000_000, (1 << 27) + 5, 600_000, 20000))
    dup = codes[1000:1500]   # Put again with other counts: the table holds the later ones
    ctx = rc.Context(k=k)
    ctx.table_build(np.concatenate([codes, dup]), np.concatenate([counts, np.full(len(dup), 9, np.int32)]))
    assert ctx.table_layout() == (0 if layout == "wide" else 1)
    want = counts.copy()
    want[1000:1500] = 9
    got = table_spectrum_equals_export(ctx)
    assert np.array_equal(np.sort(got), np.sort(want))
    assert_spectrum(ctx.kmer_spectrum("table", 1 << 20), want, 1 << 20)
    ctx.close()


def test_table_spectrum_of_shared_and_replicated_tables(rc):
    k = 23
    codes, counts = skewed_table(k, 100000, 7)
    src = rc.Context(k=k)
    src.table_build(codes, counts)
    shared, repl = rc.Context(k=k), rc.Context(k=k)
    shared.share_table_of(src)
    repl.replicate_table_of(src)
    for c in (src, shared, repl):
        assert_spectrum(c.kmer_spectrum("table", 10000), counts, 10000)
    for c in (shared, repl, src):
        c.close()


def test_spectrum_errors_and_empty_table(rc):
    ctx = rc.Context(k=23)
    with pytest.raises(rc.RcorrectorError, match="no k-mer table"):
        ctx.kmer_spectrum("table")
    with pytest.raises(rc.RcorrectorError, match="no counted spectrum"):
        ctx.kmer_spectrum("counted")
    ctx.table_build(np.zeros(0, np.uint64), np.zeros(0, np.int32))
    f, st = ctx.kmer_spectrum("table", 100)
    assert len(f) == 101 and not f.any() and st == {"distinct": 0, "total": 0, "unique": 0, "max_count": 0}
    # counted without arming: nothing to hand out; armed: the bound is the largest max_bin
    ctx.count_begin()
    ctx.count_add(b"ACGTACGTACGTACGTACGTACGTACGT\0")
    ctx.count_finish(2)
    with pytest.raises(rc.RcorrectorError, match="no counted spectrum"):
        ctx.kmer_spectrum("counted")
    ctx.count_spectrum(50)
    ctx.count_begin()
    ctx.count_add(b"ACGTACGTACGTACGTACGTACGTACGT\0")
    ctx.count_finish(2)
    assert ctx.kmer_spectrum("counted", 50)[1]["distinct"] > 0
    with pytest.raises(rc.RcorrectorError, match="above the bound"):
        ctx.kmer_spectrum("counted", 51)
    with pytest.raises(rc.RcorrectorError, match="max_bin"):
        ctx.kmer_spectrum("table", 0)
    with pytest.raises(ValueError):
        ctx.kmer_spectrum("both")
    ctx.count_release()   # (the counted spectrum stays until the next count_begin)
    assert ctx.kmer_spectrum("counted", 50)[1]["distinct"] > 0
    ctx.count_begin()
    with pytest.raises(rc.RcorrectorError, match="no counted spectrum"):
        ctx.kmer_spectrum("counted")
    ctx.close()


# ---- rcorrector -histo ------------------------------------------------------------------------------------------------------------
def fixture_reads(name):
    """the fixture's reads as a padded array (N beyond a read's end) and their lengths"""
    d = os.path.join(gu.GOLDEN, name)
    args = open(os.path.join(d, "cmd.txt")).read().split()
    files = []
    i = 0
    while i < len(args):
        if args[i] in ("-r", "-i"):
            files.append(args[i + 1]); i += 2
        elif args[i] == "-p":
            files += args[i + 1:i + 3]; i += 3
        else:
            i += 1
    seqs = [s for f in files for s in open(os.path.join(d, f), "rb").read().split(b"\n")[1::4]]
    L = max(len(s) for s in seqs)
    a = np.full((len(seqs), L), ord("N"), dtype=np.uint8)
    for j, s in enumerate(seqs):
        a[j, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return a, np.array([len(s) for s in seqs]), int(args[args.index("-k") + 1])


def read_histo(path):
    rows = [tuple(int(x) for x in ln.split()) for ln in open(path).read().splitlines()]
    assert rows == sorted(rows) and all(f > 0 for _, f in rows)
    return rows


def histo_rows(freq):
    return [(c, int(freq[c])) for c in range(1, len(freq)) if freq[c]]


def run_cli(name, tmp_path, tag, drop_c, extra=(), env=None):
    d = os.path.join(gu.GOLDEN, name)
    args = open(os.path.join(d, "cmd.txt")).read().split()
    if drop_c:
        i = args.index("-c")
        del args[i:i + 2]
    od = tmp_path / tag
    p = subprocess.run([CLI] + args + ["-od", str(od)] + list(extra), cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr.decode()
    return p, od


@pytest.mark.parametrize("name", EXACT_DUMP_FIXTURES)
def test_cli_histo_without_c_is_the_full_spectrum_of_the_reads(name, tmp_path):
    """The fixture's dump is the exact count of its reads, so the run without -c reproduces the reference's bytes -- with
    -histo as well: the .cor.fq outputs and stderr do not change.  The file is numpy's spectrum of the reads, count 1 included."""
    a, lens, k = fixture_reads(name)
    cnt = all_counts(synth.canonical_codes(a, k, lens))
    h = str(tmp_path / "h.txt")
    p, od = run_cli(name, tmp_path, "o", True, ["-histo", h])
    gu.assert_same_as_reference(name, od, p.stderr)
    assert read_histo(h) == histo_rows(spectrum(cnt, 10000)[0])
    assert read_histo(h)[0][0] == 1


@pytest.mark.parametrize("name", ["fx_pe_k23", "fx_k31_mc8", "fx_varlen_n"])
@pytest.mark.parametrize("resident", [None, "0"])
def test_cli_histo_on_two_gpus_and_histo_max(name, resident, tmp_path):
    """-gpus 2 (both on device 0): one pass counts sharded over the two contexts, two passes on the first; the same file.
    -histo-max 5 folds the higher bins into the fifth."""
    a, lens, k = fixture_reads(name)
    cnt = all_counts(synth.canonical_codes(a, k, lens))
    env = {"RC_SHARED_GPU": "1"}
    if resident is not None:
        env["RC_RESIDENT"] = resident
    h2, h5 = str(tmp_path / "h2.txt"), str(tmp_path / "h5.txt")
    p, od = run_cli(name, tmp_path, "g2", True, ["-histo", h2, "-gpus", "2"], env)
    gu.assert_same_as_reference(name, od, b"", check_stderr=False)
    assert read_histo(h2) == histo_rows(spectrum(cnt, 10000)[0])
    p, od = run_cli(name, tmp_path, "m5", True, ["-histo", h5, "-histo-max", "5"], env)
    assert read_histo(h5) == histo_rows(spectrum(cnt, 5)[0])


@pytest.mark.parametrize("name", EXACT_DUMP_FIXTURES)
def test_cli_histo_with_c_is_the_dump_spectrum(name, tmp_path):
    toks = open(os.path.join(gu.GOLDEN, name, "dump.jf"), "rb").read().split()
    dump_counts = np.array([int(t[1:]) for t in toks[0::2]], dtype=np.int64)
    assert (dump_counts >= 2).all()
    h = str(tmp_path / "h.txt")
    p, od = run_cli(name, tmp_path, "o", False, ["-histo", h])
    gu.assert_same_as_reference(name, od, p.stderr)
    assert read_histo(h) == histo_rows(spectrum(dump_counts, 10000)[0])


def test_wrapper_passes_histo_through(tmp_path):
    name = "fx_se_k23"
    d = os.path.join(gu.GOLDEN, name)
    a, lens, k = fixture_reads(name)
    cnt = all_counts(synth.canonical_codes(a, k, lens))
    tmpd = tmp_path / "tmp"
    tmpd.mkdir()
    h = str(tmp_path / "h.txt")
    wrapper = os.path.join(gu.ROOT, "tools", "run_rcorrector_gpu")
    p = subprocess.run([sys.executable, wrapper, "-s", "reads.fq", "-k", "23", "-od", str(tmp_path / "o"), "-tmpd", str(tmpd),
                        "-histo", h, "-histo-max", "7"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    gu.assert_same_as_reference(name, tmp_path / "o", b"", check_stderr=False)
    assert read_histo(h) == histo_rows(spectrum(cnt, 7)[0])
