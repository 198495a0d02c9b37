"""GPU: rc_table_compare / Context.table_compare -- two k-mer tables side by side -- against the numpy model of
tests/compare_model.py.  The tables are built with table_build from seeded arrays, so the model has the truth without
reading a table back; every case asserts the layout it means to test.

What the shapes are for (rc_compare.hip): the kernel keeps the 32 x 32 low corner of the matrix in LDS (RC_CMP_CORNER),
sends the other cells to the device array, and lets the first live lane of a wavefront add for every lane that shares its
cell -- so counts of 31 / 32 / 33 on either side, tables that fall into one cell inside and outside the corner, and
counts around max_bin are what can go wrong; a wavefront's step covers 128 buckets, so a table of 64 home buckets and
tables whose bucket count is no multiple of 128 are the scan's edges."""
import os

import numpy as np
import pytest

import compare_model as cm
import datasets
import golden_util as gu

pytestmark = pytest.mark.gpu
CORNER = 32          # RC_CMP_CORNER
WAVE_SPAN = 128      # buckets a wavefront takes per step: 64 lanes x RC_CMP_UNROLL


@pytest.fixture(scope="module")
def rc():
    import rcorrector_amd
    return rcorrector_amd


def random_codes(seed, k, n):
    """about n distinct canonical codes of k bases (a few more are drawn than asked for: some draws repeat)"""
    rng = np.random.default_rng(seed)
    n += n // 8 + 8
    codes = rng.integers(0, 1 << (2 * k), size=n, dtype=np.uint64, endpoint=False) if k < 32 else rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    return np.unique(np.minimum(codes, datasets.revcomp_codes(codes, k)))


def mixed_counts(seed, n, max_bin):
    """a Zipf-like bulk; one k-mer in eight takes a count from either side of the LDS corner's edge, of max_bin, or far beyond"""
    rng = np.random.default_rng(seed)
    c = np.minimum(rng.zipf(1.5, size=n), 100000).astype(np.int64)
    edge = np.array([1, 2, CORNER - 1, CORNER, CORNER + 1, max(1, max_bin - 1), max_bin, max_bin + 1, 70000], dtype=np.int64)
    pick = rng.random(n) < 0.125
    c[pick] = edge[rng.integers(0, len(edge), size=int(pick.sum()))]
    return c.astype(np.int32)


def make_ctx(rc, k, codes, counts, monkeypatch, env=None):
    for key, v in (env or {}).items():
        monkeypatch.setenv(key, v)
    ctx = rc.Context(k=k)
    ctx.table_build(codes, counts)
    for key in (env or {}):
        monkeypatch.delenv(key)
    return ctx


def assert_layout(ctx, k, n, layout, ext=None, load=0.4):
    """the layout the case is about, and for PACKED the extension bits the build's rule gives a table of n entries"""
    assert ctx.table_layout() == layout, "k = %d, %d entries: layout %d expected" % (k, n, layout)
    if layout == 1 and ext is not None:
        got_ext, home = datasets.packed_rule(k, n, load)
        assert got_ext == ext, "k = %d, %d entries: the rule gives ext %d, the case wants %d" % (k, n, got_ext, ext)
        assert home < ctx.table_stats()["buckets"] <= home + 33


def same_result(got, want, what):
    assert got["cells"].dtype == np.uint64 and got["cells"].shape == want["cells"].shape
    bad = np.argwhere(got["cells"] != want["cells"])
    assert len(bad) == 0, "%s: cells differ at %s (got %s, want %s)" % (
        what, bad[:5].tolist(), [int(got["cells"][i, j]) for i, j in bad[:5]], [int(want["cells"][i, j]) for i, j in bad[:5]])
    for f in cm.STAT_FIELDS:
        assert got[f] == want[f], "%s: %s is %d, expected %d" % (what, f, got[f], want[f])


def check_pair(a, b, set_a, set_b, k, max_bins=(255,)):
    """compare(a, b) against the model, and the invariants every case must keep"""
    dig = (a.table_digest(), b.table_digest())
    for mb in max_bins:
        want = cm.compare(set_a, set_b, k, mb)
        got = a.table_compare(b, mb)
        same_result(got, want, "max_bin %d" % mb)
        assert got["cells"][0, 0] == 0
        for ctx, sums, side in ((a, got["cells"].sum(axis=1), "a"), (b, got["cells"].sum(axis=0), "b")):
            freq, st = ctx.kmer_spectrum("table", mb)
            assert np.array_equal(sums[1:], freq[1:]), "the sums over %s's bins are not its spectrum" % side
            assert (got["distinct_" + side], got["mass_" + side], got["max_count_" + side]) == (st["distinct"], st["total"], st["max_count"])
        same_result(b.table_compare(a, mb), cm.transposed(want), "max_bin %d, b against a" % mb)
    assert (a.table_digest(), b.table_digest()) == dig
    return got


def overlapping_sets(seed, k, n_a, n_b, max_bin=255):
    """two sets that share about a third of their k-mers, counts drawn independently"""
    pool = random_codes(seed, k, n_a + n_b)
    rng = np.random.default_rng(seed + 1)
    pool = pool[rng.permutation(len(pool))]
    assert len(pool) >= n_a + n_b
    s = min(n_a, n_b) // 3
    ka, kb = pool[:n_a], np.sort(np.concatenate([pool[:s], pool[n_a:n_a + n_b - s]]))
    return (ka, mixed_counts(seed + 2, len(ka), max_bin)), (kb, mixed_counts(seed + 3, len(kb), max_bin))


# ---- layouts ---------------------------------------------------------------------------------------------------------------

WIDE = {"RC_TABLE_LAYOUT": "wide"}
LOW_LOAD = {"RC_TABLE_LOAD": "0.06"}
FILTER = {"RC_TABLE_FILTER": "force"}
#           k   n_a      env_a     (layout, ext, load)    n_b      env_b     (layout, ext, load)
PAIRS = [
    (23, 3000, WIDE, (0, None, 0.4), 5000, WIDE, (0, None, 0.4)),
    (23, 30000, None, (1, 0, 0.4), 4000, WIDE, (0, None, 0.4)),
    (23, 4000, WIDE, (0, None, 0.4), 30000, None, (1, 0, 0.4)),
    (23, 30000, None, (1, 0, 0.4), 40000, None, (1, 0, 0.4)),
    (23, 3000, None, (1, 4, 0.4), 30000, None, (1, 0, 0.4)),           # a small table borrows count bits, the large one does not
    (27, 120000, None, (1, 6, 0.4), 400000, None, (1, 5, 0.4)),        # a different ext on the two sides
    (28, 120000, None, (1, 8, 0.4), 120000, WIDE, (0, None, 0.4)),
    (29, 450000, None, (1, 8, 0.4), 20000, None, (0, None, 0.4)),      # (20 000 entries at k = 29 would need 13 bits: WIDE by itself)
    (30, 270000, LOW_LOAD, (1, 8, 0.06), 270000, LOW_LOAD, (1, 8, 0.06)),
    (23, 30000, FILTER, (1, 0, 0.4), 30000, None, (1, 0, 0.4)),        # the absence filter on one side only
    (23, 30000, None, (1, 0, 0.4), 3000, FILTER, (1, 4, 0.4)),
    (11, 20000, None, (1, 0, 0.4), 9000, WIDE, (0, None, 0.4)),
    (32, 5000, None, (0, None, 0.4), 3000, None, (0, None, 0.4)),      # k = 32: WIDE at this size
    (3, 32, None, (1, 0, 0.4), 30, WIDE, (0, None, 0.4)),              # k = 3: 32 canonical codes, the key space nearly full
]


@pytest.mark.parametrize("k,n_a,env_a,lay_a,n_b,env_b,lay_b", PAIRS, ids=["k%d-%d%s-%d%s" % (p[0], p[1], "".join(sorted((p[2] or {}).values())), p[4], "".join(sorted((p[5] or {}).values()))) for p in PAIRS])
def test_layout_pairs_equal_the_model(rc, k, n_a, env_a, lay_a, n_b, env_b, lay_b, monkeypatch):
    if k == 3:   # (all of the key space on one side, all but two codes on the other)
        allc = random_codes(1, 3, 4000)
        assert len(allc) == 32
        set_a, set_b = (allc, mixed_counts(5, 32, 255)), (allc[1:31], mixed_counts(6, 30, 255))
    else:
        set_a, set_b = overlapping_sets(100 + k, k, n_a, n_b)
    a = make_ctx(rc, k, *set_a, monkeypatch, env_a)
    b = make_ctx(rc, k, *set_b, monkeypatch, env_b)
    assert_layout(a, k, len(set_a[0]), *lay_a)
    assert_layout(b, k, len(set_b[0]), *lay_b)
    got = check_pair(a, b, set_a, set_b, k)
    assert 0 < got["shared"] < min(got["distinct_a"], got["distinct_b"]) or k == 3
    a.close()
    b.close()


# ---- overlap shapes --------------------------------------------------------------------------------------------------------

def test_disjoint_identical_subset_and_one_entry(rc, monkeypatch):
    k = 23
    codes = random_codes(7, k, 12000)
    ca, cb = mixed_counts(8, len(codes), 255), mixed_counts(9, len(codes), 255)
    half = len(codes) // 2
    full = make_ctx(rc, k, codes, ca, monkeypatch)
    twin = make_ctx(rc, k, codes, ca, monkeypatch, WIDE)                # the same content in the other layout
    front = make_ctx(rc, k, codes[:half], cb[:half], monkeypatch)
    back = make_ctx(rc, k, codes[half:], cb[half:], monkeypatch)
    one = make_ctx(rc, k, codes[5:6], np.array([CORNER], np.int32), monkeypatch)
    assert (full.table_layout(), twin.table_layout()) == (1, 0) and full.table_digest() == twin.table_digest()
    assert one.table_stats()["buckets"] < WAVE_SPAN                      # fewer buckets than one wavefront's step
    assert full.table_stats()["buckets"] % WAVE_SPAN != 0                # ... and a last step that is not full
    got = check_pair(front, back, (codes[:half], cb[:half]), (codes[half:], cb[half:]), k)          # disjoint
    assert got["shared"] == 0 and got["cells"][1:, 1:].sum() == 0
    got = check_pair(full, twin, (codes, ca), (codes, ca), k)                                        # identical
    assert got["shared"] == len(codes) and np.array_equal(got["cells"], np.diag(np.diag(got["cells"])))
    got = check_pair(front, full, (codes[:half], cb[:half]), (codes, ca), k)                         # a inside b
    assert got["shared"] == got["distinct_a"] == half and got["cells"][1:, 0].sum() == 0 and got["cells"][0, 1:].sum() == len(codes) - half
    got = check_pair(one, full, (codes[5:6], [CORNER]), (codes, ca), k)                              # one entry
    assert got["distinct_a"] == got["shared"] == 1 and got["shared_mass_a"] == CORNER and got["shared_mass_b"] == int(ca[5])
    got = check_pair(one, back, (codes[5:6], [CORNER]), (codes[half:], cb[half:]), k)
    assert got["shared"] == 0 and got["cells"][CORNER, 0] == 1
    for c in (full, twin, front, back, one):
        c.close()


def test_a_table_against_itself_a_borrower_and_a_replica(rc, monkeypatch):
    k = 23
    codes = random_codes(17, k, 30000)
    counts = mixed_counts(18, len(codes), 255)
    src = make_ctx(rc, k, codes, counts, monkeypatch)
    shared, repl = rc.Context(k=k), rc.Context(k=k)
    shared.share_table_of(src)
    repl.replicate_table_of(src)
    for other in (src, shared, repl):
        got = check_pair(src, other, (codes, counts), (codes, counts), k, (7, 255))
        assert np.array_equal(got["cells"], np.diag(np.diag(got["cells"]))) and got["shared"] == len(codes)
        assert got["shared_mass_a"] == got["shared_mass_b"] == got["mass_a"] == int(counts.astype(np.int64).sum())
    for c in (shared, repl, src):
        c.close()


# ---- counts ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_bin", [1, 7, 255, 1023])
def test_counts_around_max_bin_and_the_corner(rc, max_bin, monkeypatch):
    """every pair of counts from {1, 2, 31, 32, 33, max_bin - 1, max_bin, max_bin + 1, 70 000} on the two sides occurs"""
    k = 23
    palette = sorted({1, 2, CORNER - 1, CORNER, CORNER + 1, max(1, max_bin - 1), max_bin, max_bin + 1, 70000})
    grid = np.array([(x, y) for x in palette for y in palette] * 40, dtype=np.int32)
    codes = random_codes(20 + max_bin, k, 40000)[:len(grid) + 2000]
    extra = len(codes) - len(grid)
    set_a = (codes[:len(grid) + extra // 2], np.concatenate([grid[:, 0], mixed_counts(1, extra // 2, max_bin)]))
    set_b = (np.concatenate([codes[:len(grid)], codes[len(grid) + extra // 2:]]), np.concatenate([grid[:, 1], mixed_counts(2, extra - extra // 2, max_bin)]))
    a = make_ctx(rc, k, *set_a, monkeypatch)
    b = make_ctx(rc, k, *set_b, monkeypatch, WIDE)
    assert (a.table_layout(), b.table_layout()) == (1, 0)
    got = check_pair(a, b, set_a, set_b, k, (max_bin,))
    fold = lambda c: min(c, max_bin)
    for x in palette:
        for y in palette:
            assert got["cells"][fold(x), fold(y)] >= 40
    a.close()
    b.close()


@pytest.mark.parametrize("ca,cb", [(1, 1), (CORNER + 8, CORNER - 1), (300, 5)], ids=["cell-1-1", "outside-the-corner", "folded"])
def test_every_kmer_in_one_cell(rc, ca, cb, monkeypatch):
    """contention: all lanes of every wavefront add to the same word -- in LDS, and in the device array"""
    k = 23
    codes = random_codes(31, k, 60000)
    set_a, set_b = (codes, np.full(len(codes), ca, np.int32)), (codes, np.full(len(codes), cb, np.int32))
    a = make_ctx(rc, k, *set_a, monkeypatch)
    b = make_ctx(rc, k, *set_b, monkeypatch)
    assert (a.table_layout(), b.table_layout()) == (1, 1)
    got = check_pair(a, b, set_a, set_b, k)
    assert got["cells"][min(ca, 255), min(cb, 255)] == len(codes) == got["cells"].sum()
    a.close()
    b.close()


@pytest.mark.parametrize("k,n,env,layout,ext", [(23, 30000, None, 1, 0), (28, 120000, None, 1, 8), (23, 6000, WIDE, 0, None)])
def test_counts_too_large_for_a_packed_slot(rc, k, n, env, layout, ext, monkeypatch):
    """Counts at and beyond the PACKED count field (2^(27 - ext) - 1 is the slot's mark: from there on the count lives in the
    table's prefix), up to 2^31 - 1, pinned as datasets.huge_make pins them; the masses are exact 64-bit sums."""
    set_a, set_b = overlapping_sets(400 + k, k, n, n)
    limit = 1 << (27 - (ext or 0))
    pins = np.array([limit - 2, limit - 1, limit, limit + 1, datasets.INT_MAX], dtype=np.int64)
    ca, cb = set_a[1].astype(np.int64), set_b[1].astype(np.int64)
    shared = np.nonzero(np.isin(set_a[0], set_b[0]))[0]
    ca[shared[:5]] = pins                                  # huge in a, whatever b holds
    ca[shared[5:305]] = datasets.INT_MAX - np.arange(300)  # 300 more beyond the field: the prefix is searched, not scanned
    cb[np.searchsorted(set_b[0], set_a[0][shared[3:8]])] = pins[::-1]   # huge on both sides for two of them, in b alone for three
    only_a = np.nonzero(~np.isin(set_a[0], set_b[0]))[0]
    ca[only_a[:5]] = pins
    set_a, set_b = (set_a[0], ca.astype(np.int32)), (set_b[0], cb.astype(np.int32))
    a = make_ctx(rc, k, *set_a, monkeypatch, env)
    b = make_ctx(rc, k, *set_b, monkeypatch)
    assert_layout(a, k, len(set_a[0]), layout, ext)
    assert b.table_layout() == 1
    if layout == 1:
        assert 300 <= datasets.huge_overflowing(ca, ext) <= datasets.RC_PACKED_OVF_MAX
    got = check_pair(a, b, set_a, set_b, k, (255, 1023))
    assert got["max_count_a"] == got["max_count_b"] == datasets.INT_MAX and got["mass_a"] > 300 * (1 << 30)
    a.close()
    b.close()


# ---- duplicate keys --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout_env", [None, WIDE], ids=["packed", "wide"])
def test_repeated_kmers_of_a_quirky_dump_count_once(rc, layout_env, tmp_path, monkeypatch):
    """A dump that repeats k-mers leaves several slots with the same key in the table; the entry rc_table_lookup answers
    with is the one that counts."""
    import io_quirks
    k = 23
    path = str(tmp_path / "quirky.jf")
    io_quirks.make_quirky_dump(77, path, k=k, n=4000)
    for key, v in (layout_env or {}).items():
        monkeypatch.setenv(key, v)
    a = rc.Context(k=k)
    stored = a.load_jfdump(path)
    for key in (layout_env or {}):
        monkeypatch.delenv(key)
    assert a.table_layout() == (0 if layout_env else 1)
    codes = np.unique(a.table_export()[0])
    assert stored > len(codes) > 2000                       # repeated k-mers were stored, and are live once
    set_a = (codes, a.lookup(codes))
    set_b = (codes[::2], mixed_counts(3, len(codes[::2]), 255))
    b = make_ctx(rc, k, *set_b, monkeypatch)
    check_pair(a, b, set_a, set_b, k)
    a.close()
    b.close()


# ---- the contexts afterwards -----------------------------------------------------------------------------------------------

def test_correction_is_byte_equal_after_a_compare(rc, oracle):
    name = "fx_se_k23"
    d = os.path.join(gu.GOLDEN, name)
    lines = open(os.path.join(d, "reads.fq"), "rb").read().split(b"\n")
    n = len(lines) // 4
    seqs, quals = lines[1:4 * n:4], lines[3:4 * n:4]
    ctx, other = rc.Context(k=23), rc.Context(k=23)
    ctx.load_jfdump(os.path.join(d, "dump.jf"))
    ctx.set_run_params(0.01, b"H")
    codes = random_codes(3, 23, 5000)
    other.table_build(codes, mixed_counts(4, len(codes), 255))

    def correct():
        a, off = oracle.pack_reads(seqs)
        q, _ = oracle.pack_reads(quals)
        return ctx.correct_batch(0, a, q, off) + (a,)
    before = correct()
    assert int((before[0] > 0).sum()) > 0
    dig = ctx.table_digest()
    ctx.table_compare(other, 255)
    other.table_compare(ctx, 1023)
    after = correct()
    assert ctx.table_digest() == dig
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    ctx.close()
    other.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_and_their_texts(rc, monkeypatch):
    import torch
    codes = random_codes(5, 23, 2000)
    a = make_ctx(rc, 23, codes, mixed_counts(6, len(codes), 255), monkeypatch)
    empty, other_k = rc.Context(k=23), make_ctx(rc, 21, random_codes(5, 21, 2000)[:1000], np.full(1000, 3, np.int32), monkeypatch)
    L = rc.load_library()
    cells = np.zeros(256 * 256, np.uint64)

    def refused(x, y, max_bin, ptr, status, text):
        assert L.rc_table_compare(x._h, y._h, max_bin, ptr, None) == status
        assert text in L.rc_last_error(x._h).decode(), L.rc_last_error(x._h).decode()

    STATE, ARG = -4, -1
    refused(a, empty, 255, cells.ctypes.data, STATE, "no k-mer table loaded in the second context")
    refused(empty, a, 255, cells.ctypes.data, STATE, "no k-mer table loaded in the first context")
    refused(a, other_k, 255, cells.ctypes.data, ARG, "k = 23 and k = 21")
    refused(a, a, 255, None, ARG, "cells not NULL")
    refused(a, a, 0, cells.ctypes.data, ARG, "max_bin must be 1..1023 (got 0)")
    refused(a, a, 1024, cells.ctypes.data, ARG, "max_bin must be 1..1023 (got 1024)")
    with pytest.raises(rc.RcorrectorError, match="max_bin must be 1..1023"):
        a.table_compare(a, 5000)
    assert a.table_compare(a, 1023)["cells"].shape == (1024, 1024)     # the largest matrix the call takes, stats == NULL above
    if torch.cuda.device_count() >= 2:
        far = rc.Context(k=23, device=1)
        far.replicate_table_of(a)
        refused(a, far, 255, cells.ctypes.data, ARG, "rc_table_replicate")
        far.close()
    for c in (a, empty, other_k):
        c.close()
