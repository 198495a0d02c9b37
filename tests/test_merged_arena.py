"""GPU: the arena rc_read_merge_device leaves in HBM, handed as it lies -- d_mseq / d_mqual / d_moff, units reads, mode 0, nbytes =
d_moff[units], no trip through host memory -- to every per-read entry point (include/rcorrector_amd.h: "an arena every per-read
entry point accepts as it is in mode 0").  The arenas are tests/merged_arena.py's: runs of up to 300 empty reads, 5 000 of them
alone, offsets at every residue of 16, reads of up to 2045 bases, computed qualities.  The merge runs once per arena (module
fixture) and is checked against tests/merge_model.py; every consumer is then compared with the CPU reference its own test file
uses, computed on the MODEL's strings, and with the same strings uploaded from the host through pack_reads.
tests/test_merged_arena_cases.py shows on the CPU that none of these comparisons is an empty one."""
import ctypes

import numpy as np
import pytest

import merged_arena as ma
import recur_model as rm
import rcorrector_amd
import test_trust_profile as ttp
from rcorrector_amd import binding as B
from test_duplicates import dup_key, host_keys  # noqa: F401  (dup_key: the fixture that builds the host program)
from test_high_arena import probe_want
from test_read_depth import restate_all as depth_rows
from test_read_depth import table_of
from test_read_merge import POISON, SLACK, assert_equal, params_of
from test_read_screen import restate_all as screen_rows
from test_recount import canonical_codes
from test_weak_profile import restate_all as weak_rows

pytestmark = pytest.mark.gpu
K = ma.K
RC_STATUS_ARG = -1
ARENAS = ("mixed", "mixed_fasta", "long", "unmerged")


def merge_buffers(name):
    """the pairs of ma.arena(name) uploaded and the output tensors allocated and filled with poison: everything a merge needs in
    HBM, made on torch's stream -- the caller synchronises once before it issues anything on a context's stream"""
    import torch
    a = ma.arena(name)
    arena, off = rcorrector_amd.pack_reads(a["seqs"])
    units = len(a["seqs"]) // 2
    m = {"name": name, "units": units, "in_bytes": int(arena.size),
         "seq": torch.from_numpy(arena).cuda(), "off": torch.from_numpy(off.astype(np.int32)).cuda(), "qual": None, "mqual": None,
         "rows": torch.full((units, 4), -7, dtype=torch.int32, device="cuda"),
         "mseq": torch.full((arena.size + SLACK,), POISON, dtype=torch.uint8, device="cuda"),
         "moff": torch.full((units + 2,), -7, dtype=torch.int32, device="cuda"),
         "tally": torch.zeros(B.MERGE_TALLY_WORDS, dtype=torch.int64, device="cuda")}
    if a["quals"] is not None:
        m["qual"] = torch.from_numpy(rcorrector_amd.pack_reads(a["quals"])[0]).cuda()
        m["mqual"] = torch.full((arena.size + SLACK,), POISON, dtype=torch.uint8, device="cuda")
    return m


def issue_merge(ctx, m):
    """read_merge_device on the buffers of merge_buffers: the call alone, no synchronisation of any kind"""
    a = ma.arena(m["name"])
    ctx.read_merge_device(m["seq"], m["qual"], m["off"], 2 * m["units"], m["in_bytes"], a["max_read_len"], 2, params_of(a["p"]), m["rows"], m["mseq"], m["mqual"],
                          m["moff"], m["in_bytes"], m["tally"])


def merge_on_device(ctx, name):
    """read_merge_device on the pairs of ma.arena(name), uploaded once: the device tensors, kept"""
    import torch
    m = merge_buffers(name)
    torch.cuda.synchronize()
    issue_merge(ctx, m)
    ctx.sync()
    m["total"] = int(m["moff"][m["units"]].item())
    return m


def as_results(m):
    """the device tensors of merge_on_device as the dict test_read_merge.assert_equal takes"""
    units = m["units"]
    moff = m["moff"].cpu().numpy().view(np.uint32)
    total = int(moff[units])
    assert moff[units + 1] == np.uint32(-7 & 0xFFFFFFFF) and total <= m["in_bytes"]
    got = {"rows": m["rows"].cpu().numpy(), "moff": moff[:units + 1], "tally": B.merge_tally_dict(m["tally"].cpu().numpy())}
    for k in ("mseq", "mqual"):
        got[k] = None
        if m[k] is not None:
            assert bool((m[k][total:] == POISON).all()), "%s: a byte at or behind d_moff[units] = %d was written" % (k, total)
            got[k] = m[k][:total].cpu().numpy().tobytes()
    return got


@pytest.fixture(scope="module")
def merged():
    """{name: the merged arena of ma.arena(name) in HBM}, each merged once on a context without a table"""
    ctx = rcorrector_amd.Context(k=K, max_fix_per_k=4, device=0)
    out = {name: merge_on_device(ctx, name) for name in ARENAS}
    yield out
    ctx.close()


def table_ctx(which="all"):
    ctx = rcorrector_amd.Context(k=K, max_fix_per_k=4, device=0)
    ctx.table_build(*ma.table_arrays(which))
    ctx.set_run_params(ma.error_rate(), b"H")
    return ctx


@pytest.fixture(scope="module")
def tctx():
    c = table_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def screen_ctx():
    c = table_ctx("half")
    yield c
    c.close()


def uploaded(name):
    """the model's merged strings through pack_reads: (d_seq, d_qual or zeros, d_off, units, nbytes)"""
    import torch
    a = ma.arena(name)
    arena, off = rcorrector_amd.pack_reads(a["strings"])
    assert arena.tobytes() == a["want"][2] and np.array_equal(off.astype(np.uint32), a["want"][1])
    q = torch.zeros(arena.size, dtype=torch.uint8, device="cuda") if a["qstrings"] is None else torch.from_numpy(rcorrector_amd.pack_reads(a["qstrings"])[0]).cuda()
    return torch.from_numpy(arena).cuda(), q, torch.from_numpy(off.astype(np.int32)).cuda(), len(a["strings"]), int(arena.size)


def on_the_spot(m, copy=False):
    """the merged arena where the merge left it: (d_seq, d_qual or zeros, d_off, units, nbytes); copy: a copy of the bases, for a
    call that corrects in place (at the same alignment: both start on an allocation's first byte)"""
    import torch
    q = m["mqual"] if m["mqual"] is not None else torch.zeros(m["mseq"].numel(), dtype=torch.uint8, device="cuda")
    seq = m["mseq"].clone() if copy else m["mseq"]
    assert seq.data_ptr() % 16 == 0
    return seq, q, m["moff"], m["units"], m["total"]


def rows_of(call, n):
    """call(d_out) with d_out n x 4 int32 preset to -7; the rows after a sync"""
    import torch
    out = torch.full((max(n, 1), 4), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    call(out)
    torch.cuda.synchronize()
    return out.cpu().numpy()[:n]


def differing(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, want %s" % (what, got.shape, want.shape)
    bad = np.nonzero((got != want).reshape(len(want), -1).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d differ, first at %d: got %s, want %s" % (what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


# ---- 0. the merge itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ARENAS)
def test_the_merge_equals_the_model(merged, name):
    assert_equal(as_results(merged[name]), ma.arena(name)["want"], name)
    assert merged[name]["total"] == len(ma.arena(name)["want"][2])


# ---- 1. correct_device and strong_threshold_device -----------------------------------------------------------------------------
def correct(ctx, seq, qual, off, n, nbytes, max_len):
    """correct_device in mode 0: (ret, l, m, h, the arena's bytes afterwards)"""
    import torch
    res = [torch.full((max(n, 1),), -77, dtype=torch.int32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    ctx.correct_device(0, n, nbytes, max_len, seq, qual, off, *res)
    ctx.sync()
    return [r.cpu().numpy()[:n] for r in res] + [seq[:nbytes].cpu().numpy().tobytes()]


def strong_of(ctx, seq, off, n, nbytes, max_len):
    import torch
    out = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.strong_threshold_device(seq, off, n, nbytes, max_len, out)
    ctx.sync()
    return out.cpu().numpy()[:n]


def assert_corrected(got, name, what):
    strong, ret, l, m, h, fixed = ma.oracle_want(name)
    for g, w, f in zip(got[:4], (ret, l, m, h), ("ret", "l", "m", "h")):
        differing(g, w, "%s: %s" % (what, f))
    want = b"".join(s + b"\0" for s in fixed)
    assert got[4] == want, "%s: the corrected bytes differ, first at byte %d" % (what, next(i for i, (x, y) in enumerate(zip(got[4], want)) if x != y))


@pytest.mark.parametrize("locality", ["default", "force"])
@pytest.mark.parametrize("name", ["mixed", "mixed_fasta"])
def test_correct_device_on_the_merged_arena(merged, name, locality, monkeypatch):
    if locality == "force":
        monkeypatch.setenv("RC_LOCALITY", "force")       # (read when the context is made)
    ctx = table_ctx()
    try:
        assert ctx.estimate_error_rate(0.95) == ma.error_rate()
        spot, up = on_the_spot(merged[name], copy=True), uploaded(name)
        strong = ma.oracle_want(name)[0]
        differing(strong_of(ctx, spot[0], spot[2], spot[3], spot[4], 1023), strong, "%s strong, on the spot" % name)
        differing(strong_of(ctx, up[0], up[2], up[3], up[4], 1023), strong, "%s strong, uploaded" % name)
        a = correct(ctx, *spot, 1023)
        assert_corrected(a, name, "%s %s, on the spot" % (name, locality))
        b = correct(ctx, *up, 1023)
        assert_corrected(b, name, "%s %s, uploaded" % (name, locality))
        assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]
    finally:
        ctx.close()


@pytest.mark.parametrize("locality", ["default", "force"])
def test_correct_device_on_nothing_but_empty_reads(merged, locality, monkeypatch):
    from oracle import pyoracle as po
    if locality == "force":
        monkeypatch.setenv("RC_LOCALITY", "force")
    po.build()
    codes, counts = ma.table_arrays()
    T = po.Table(K, len(codes))
    T.put_many(codes, counts)
    P = po.make_params(K, 4, ma.error_rate(), b"H")
    want = (po.error_correction(P, T, b"", b"")[0],) + po.kmer_information(P, T, b"")
    want_strong = po.strong_threshold(P, T, b"")
    n = ma.N_UNMERGED
    ctx = table_ctx()
    try:
        for how, (seq, qual, off, units, nbytes) in (("on the spot", on_the_spot(merged["unmerged"], copy=True)), ("uploaded", uploaded("unmerged"))):
            assert units == nbytes == n
            differing(strong_of(ctx, seq, off, units, nbytes, 0), np.full(n, want_strong, np.int32), "strong, " + how)
            got = correct(ctx, seq, qual, off, units, nbytes, 0)
            for g, w, f in zip(got[:4], want, ("ret", "l", "m", "h")):
                differing(g, np.full(n, w, np.int32), "%s of an empty read, %s" % (f, how))
            assert got[4] == b"\0" * n, "an arena byte is no longer NUL, " + how
    finally:
        ctx.close()


def test_correct_device_refuses_reads_above_1023_bases_and_leaves_the_arena(merged, tctx):
    import torch
    seq, qual, off, units, nbytes = on_the_spot(merged["long"], copy=True)
    before = seq.clone()
    res = [torch.full((units,), -77, dtype=torch.int32, device="cuda") for _ in range(4)]
    b = B._DeviceBatch(0, units, nbytes, 2045, seq.data_ptr(), qual.data_ptr(), off.data_ptr(), *[r.data_ptr() for r in res])
    torch.cuda.synchronize()
    assert tctx._L.rc_correct_device(tctx._h, ctypes.byref(b)) == RC_STATUS_ARG
    err = tctx._L.rc_last_error(tctx._h).decode()
    assert "2045" in err and "1023-base limit" in err, err
    tctx.sync()
    assert torch.equal(seq, before), "a refused batch was corrected in part"
    assert all(bool((r == -77).all()) for r in res)


# ---- 2. the per-read profiles ----------------------------------------------------------------------------------------------------
def profile_want(what, name):
    """the rows of the reference on the model's strings.  To the profiles that stage reads in the probe tile (depth, screen) a
    read of more than 1023 bases is no read: four zeros; the weak profile walks the plane words of a read of any length, so its
    reference is the whole read's"""
    strings = ma.arena(name)["strings"]
    if what == "weak":
        return weak_rows(strings, K, ma.table_counts(), 25)
    rows = depth_rows(strings, K, ma.table_counts()) if what == "depth" else screen_rows(strings, K, ma.table_counts("half"), 1)
    for i, s in enumerate(strings):
        if len(s) > 1023:
            assert rows[i].any()
            rows[i] = 0
    return rows


@pytest.mark.parametrize("name", ["long", "unmerged"])
@pytest.mark.parametrize("what", ["weak", "depth", "screen"])
def test_the_profiles_on_the_merged_arena(merged, tctx, screen_ctx, what, name):
    want = profile_want(what, name)
    lens = np.array([len(s) for s in ma.arena(name)["strings"]])
    assert not want[lens == 0].any() and (name == "unmerged" or (want[(lens >= K) & (lens <= 1023)].any(axis=1)).sum() > 30)
    if name == "long":
        assert want[lens > 1023].any(axis=1).sum() == (3 if what == "weak" else 0)      # (weak: every over-long read has weak windows at 25)
    max_len = 1023 if name == "long" else 0      # (depth and screen promise four zeros for a read max_read_len said not to exist)
    for how, (seq, _, off, n, nbytes) in (("on the spot", on_the_spot(merged[name])), ("uploaded", uploaded(name))):
        if what == "weak":
            got = rows_of(lambda out: tctx.weak_profile_device(seq, off, n, nbytes, max_len, out, 25), n)
        elif what == "depth":
            got = rows_of(lambda out: tctx.read_depth_device(seq, off, n, nbytes, max_len, out), n)
        else:
            got = rows_of(lambda out: tctx.read_screen_device(screen_ctx, seq, off, n, nbytes, max_len, out, min_count=1), n)
        differing(got, want, "%s of %s, %s" % (what, name, how))


@pytest.mark.parametrize("max_len,cap", [(1023, 1024), (259, 256)])
def test_trust_profile_device_counts_a_long_reads_first_windows(merged, tctx, max_len, cap):
    """max_read_len 259 picks the instance that keeps 256 windows a read, 1023 the one that keeps 1024: a longer read -- those of
    2045 bases, and at 259 every read of 279 or more -- has its first `cap` windows counted, p3 from the last of those"""
    import torch
    strings, counts, memo = ma.arena("long")["strings"], ma.table_counts(), {}
    want = ttp.restate([ttp.window_counts(s, K, counts, memo)[:cap] for s in strings], [0] * len(strings), 25)
    assert want["windows"][0, cap - 1] >= 2 and want["weak5"][0].sum() > 100 and want["solid3"][0, 0] > 50
    for how, (seq, _, off, n, nbytes) in (("on the spot", on_the_spot(merged["long"])), ("uploaded", uploaded("long"))):
        out = torch.zeros((5, 2, ttp.MAX_LEN), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        tctx.trust_profile_device(seq, off, n, nbytes, max_len, 0, out, 25)
        tctx.sync()
        ttp.assert_counts(ttp.as_counts(out), want, "max_read_len %d, %s" % (max_len, how))


# ---- 3. the census keys ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "unmerged"])
def test_read_keys_device_on_the_merged_arena(merged, tctx, dup_key, name):  # noqa: F811
    import torch
    strings = ma.arena(name)["strings"]
    want = host_keys(dup_key, strings, 0)
    empty = np.array([not s for s in strings])
    assert len({tuple(k) for k in want[empty].tolist()}) == 1 and len({tuple(k) for k in want[~empty].tolist()}) == (~empty).sum()
    for how, (seq, _, off, n, nbytes) in (("on the spot", on_the_spot(merged[name])), ("uploaded", uploaded(name))):
        out = torch.full((n, 2), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        tctx.read_keys_device(seq, off, n, nbytes, 0, out)
        tctx.sync()
        differing(out.cpu().numpy().view(np.uint64), want, "keys of %s, %s" % (name, how))


@pytest.mark.parametrize("name", ["mixed", "unmerged"])
def test_change_keys_device_between_the_merged_and_the_corrected_arena(merged, tctx, name):
    """before = the arena the merge wrote, after = a copy of it that correct_device corrected: neither has left HBM"""
    import torch
    strings = ma.arena(name)["strings"]
    fixed = ma.oracle_want(name)[5] if name == "mixed" else strings
    want = rm.Census().add(strings, fixed)
    assert (want.contexted > 30 and want.changes >= want.contexted) if name == "mixed" else want.changes == 0
    before, qual, off, n, nbytes = on_the_spot(merged[name])
    after = before.clone()
    got = correct(tctx, after, qual, off, n, nbytes, ma.arena(name)["max_len"])
    assert got[4] == b"".join(s + b"\0" for s in fixed)
    room = want.contexted + 8
    keys = torch.full((room + 4,), -7, dtype=torch.int64, device="cuda")
    counts = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    tctx.change_keys_device(before, after, off, n, nbytes, keys, room, counts)
    tctx.sync()
    k = keys.cpu().numpy()
    assert [int(x) for x in counts.cpu().numpy()] == [want.changes, want.contexted, want.contexted]
    assert sorted(int(x) for x in k[:want.contexted].view(np.uint64)) == want.key_list() and k[room:].tolist() == [-7] * 4


# ---- 4. counting -----------------------------------------------------------------------------------------------------------------
def absent_codes(counts, n):
    rng = np.random.default_rng(ma.SEED + 9)
    out = [c for c in (int(x) for x in rng.integers(0, 1 << 46, 2 * n + 16)) if c not in counts]
    return out[:n]


@pytest.mark.parametrize("name", ["long", "unmerged"])
def test_counting_the_merged_arena(merged, name):
    """count_begin / count_add_device / count_finish and count_reads_device on the arena where it lies: every k-mer of the model's
    strings and as many absent ones against a Python dictionary, the digest against a count of the uploaded strings; then
    probe_device and recount_add_device over the counted table, arena byte by arena byte, the recount's spectrum bin for bin.
    d_counts is preset to -7 and the kernel writes only where a window starts, so "the NUL of a run starts no window" is held by
    the absence of a write: for `unmerged`, probed and recounted over the fragments' table, every byte must still be -7 and the
    recount must have seen no k-mer"""
    import torch
    strings = ma.arena(name)["strings"]
    counts = ma.strings_counts(strings)
    codes = sorted(counts) + absent_codes(counts, max(len(counts), 64))
    want = np.array([counts.get(c, 0) for c in codes], dtype=np.int32)
    seq, _, _, n, nbytes = on_the_spot(merged[name])
    up = uploaded(name)
    made = []
    try:
        for how in ("add_device", "reads_device", "uploaded"):
            c = rcorrector_amd.Context(k=K, device=0)
            made.append(c)
            if how == "reads_device":
                stored = c.count_reads_device(seq, nbytes, 1)
            else:
                c.count_begin()
                c.count_add_device(seq if how == "add_device" else up[0], nbytes)
                stored = c.count_finish(1)
            assert stored == len(counts), how
            differing(c.lookup(np.array(codes, dtype=np.uint64)), want, "lookup after %s" % how)
        assert made[0].table_digest() == made[1].table_digest() == made[2].table_digest()
        if counts:
            ctx = made[0]
        else:                                        # (an empty table: probed and recounted over the fragments' table instead)
            ctx = table_ctx()
            made.append(ctx)
        d_cnt = torch.full((nbytes,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.probe_device(seq, nbytes, d_cnt)
        ctx.sync()
        differing(d_cnt.cpu().numpy(), probe_want(strings, K, counts), "probe counts of %s" % name)      # (-7 where no window starts: not written)
        ctx.recount_begin(100)
        ctx.recount_add_device(seq, nbytes)
        freq, st = ctx.recount_finish()
        occ = canonical_codes(ma.arena(name)["want"][2], K)
        assert (st["distinct"], st["total"], st["absent_distinct"], st["absent_total"]) == (len(counts), len(occ), 0, 0) and len(occ) == sum(counts.values())
        want_freq = np.bincount(np.minimum(np.array(list(counts.values()), dtype=np.int64), 100), minlength=101).astype(np.uint64)
        assert np.array_equal(freq, want_freq), "recount bins differ at %s" % np.nonzero(freq != want_freq)[0][:10]
        assert int(freq.sum()) == len(counts) and st["max_count"] == max(list(counts.values()) + [0])
    finally:
        for c in made:
            c.close()


# ---- 5. the merge's scan and the locality sort share one scratch buffer --------------------------------------------------------
def test_merge_and_correct_back_to_back_with_one_sync(merged, monkeypatch):
    """RC_LOCALITY=force: read_merge_device(unmerged), correct_device(merged mixed), read_merge_device(long) and
    correct_device(merged mixed) again, on one context.  Every buffer the four calls touch is uploaded, allocated and filled
    first, then one device-wide synchronise, then the four entry points with nothing between them -- no torch call, no sync -- and
    one ctx.sync() at the end: every output is what the same calls gave one at a time.  The merge's lengths and scan scratch and
    the locality sort's scratch are the same buffer, ctx->sel_tmp; the calls are ordered by the context's stream alone.  (The first
    merge, 5 001 scan entries, reserves more than the sort over 633 reads or the second merge, 640 entries, asks for, so nothing
    regrows between the calls: what is held here is that each user finds its predecessor done with the bytes, not the regrowth,
    which rc_dbuf_reserve guards by waiting for the stream before it frees.)"""
    import torch
    monkeypatch.setenv("RC_LOCALITY", "force")
    ctx = table_ctx()
    try:
        copies = [on_the_spot(merged["mixed"], copy=True) for _ in range(2)]
        res = [[torch.full((copies[0][3],), -77, dtype=torch.int32, device="cuda") for _ in range(4)] for _ in range(2)]
        m1, m2 = merge_buffers("unmerged"), merge_buffers("long")
        torch.cuda.synchronize()
        # ---- nothing but the four entry points from here to the sync
        issue_merge(ctx, m1)
        ctx.correct_device(0, copies[0][3], copies[0][4], 1023, copies[0][0], copies[0][1], copies[0][2], *res[0])
        issue_merge(ctx, m2)
        ctx.correct_device(0, copies[1][3], copies[1][4], 1023, copies[1][0], copies[1][1], copies[1][2], *res[1])
        ctx.sync()
        for m in (m1, m2):
            assert_equal(as_results(m), ma.arena(m["name"])["want"], "back to back: " + m["name"])
            for k in ("rows", "mseq", "mqual", "moff", "tally"):
                assert torch.equal(m[k], merged[m["name"]][k]), "back to back: %s of %s differs from the call alone" % (k, m["name"])
        for c, r in zip(copies, res):
            got = [x.cpu().numpy() for x in r] + [c[0][:c[4]].cpu().numpy().tobytes()]
            assert_corrected(got, "mixed", "back to back")
    finally:
        ctx.close()
