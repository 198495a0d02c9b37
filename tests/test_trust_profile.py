"""GPU: the k-mer trust profile by read position -- rc_trust_profile_device and the binding's trust_profile_device: per mate and
window position, from the 5' and from the 3' end, the reads that have a window there and those whose window is solid / weak
(include/rcorrector_amd.h: rc_trust_counts).

The yardstick is `restate` below: tests/test_weak_profile.py's window loop, pure Python over a dict {canonical k-mer code:
count} (missing = 0) built from a golden fixture's dump.jf or from the arrays a synthetic table was built from -- never from
the library.  For each read and valid window i it bumps solid5[m][i] and solid3[m][nwin - 1 - i], or the weak pair, and
windows[m][p] for p < nwin.  The corrected reads of the golden fixtures are the REFERENCE's (ref/*.cor.*).  Every comparison is
exact integer equality, and every test ends with a sync of the context.
"""
import numpy as np
import pytest

import rcorrector_amd
from test_weak_profile import _ACGT, canonical, device_profile, fixture, fixture_ctx

pytestmark = pytest.mark.gpu
RC_STATUS_ARG, RC_STATUS_STATE = -1, -4
MAX_LEN = 1024
FIELDS = ("windows", "solid5", "weak5", "solid3", "weak3")
_LETTERS = np.frombuffer(b"ACGT", np.uint8)


# ---- the yardstick -------------------------------------------------------------------------------------------------------------
def window_counts(seq, k, counts, memo):
    """the table's count of every window of one read, -1 for an invalid one (the window loop of test_weak_profile.restate)"""
    out = np.empty(max(0, len(seq) - k + 1), dtype=np.int64)
    for i in range(len(out)):
        w = seq[i:i + k]
        c = memo.get(w)
        if c is None:
            c = counts.get(canonical(w), 0) if _ACGT.issuperset(w) else -1
            memo[w] = c
        out[i] = c
    return out


def mates_of(mode, n):
    if mode == 0:
        return [0] * n
    if mode == 1:
        return [0] * (n // 2) + [1] * (n - n // 2)
    return [i & 1 for i in range(n)]


def empty_counts():
    return {f: np.zeros((2, MAX_LEN), dtype=np.uint64) for f in FIELDS}


def restate(per_read, mates, min_count):
    """the contract for one version of the reads: per_read = window_counts of every read, mates = its mate"""
    out = empty_counts()
    for c, m in zip(per_read, mates):
        nwin = len(c)
        assert nwin <= MAX_LEN
        out["windows"][m, :nwin] += 1
        solid = (c >= min_count).astype(np.uint64)
        weak = ((c >= 0) & (c < min_count)).astype(np.uint64)
        out["solid5"][m, :nwin] += solid
        out["weak5"][m, :nwin] += weak
        out["solid3"][m, :nwin] += solid[::-1]          # window i is p3 = nwin - 1 - i
        out["weak3"][m, :nwin] += weak[::-1]
    return out


def restate_reads(seqs, mode, k, counts, min_count, memo=None):
    memo = {} if memo is None else memo
    return restate([window_counts(s, k, counts, memo) for s in seqs], mates_of(mode, len(seqs)), min_count)


def assert_counts(got, want, what=""):
    for f in FIELDS:
        g, w = got[f], want[f]
        assert g.shape == (2, MAX_LEN) and g.dtype == np.uint64, "%s: %s" % (what, f)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, "%s: %s[%d][%d]: got %d, want %d (%d entries differ)" % (what, f, bad[0][0], bad[0][1], g[tuple(bad[0])], w[tuple(bad[0])], len(bad))


def as_counts(t):
    a = t.cpu().numpy().view(np.uint64).reshape(5, 2, MAX_LEN)
    return {f: a[i].copy() for i, f in enumerate(FIELDS)}


def device_counts(ctx, arena, off, mode, min_count, lead=0, max_len=None, into=None):
    """rc_trust_profile_device on a copy of `arena` that starts `lead` bytes behind a 16-byte boundary of device memory; the bytes
    in front of it and behind it are letters, not NULs: what the kernel may read there must not count.  Returns the tensor."""
    import torch
    n = len(off) - 1
    buf = torch.full((lead + arena.size + 64,), ord("A"), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if arena.size:
        buf[lead:lead + arena.size] = torch.from_numpy(np.ascontiguousarray(arena)).cuda()
    t_off = torch.from_numpy(np.asarray(off).astype(np.int32)).cuda()
    out = torch.zeros((5, 2, MAX_LEN), dtype=torch.int64, device="cuda") if into is None else into
    if max_len is None:
        max_len = int(np.diff(np.asarray(off).astype(np.int64)).max()) - 1 if n else 0
    torch.cuda.synchronize()
    ctx.trust_profile_device(buf.data_ptr() + lead, t_off, n, arena.size, max_len, mode, out, min_count)
    ctx.sync()
    return out


# ---- 1. the device entry point against the restatement, on arenas aimed at the kernel's seams ----------------------------------
def synthetic(k, n, long_reads):
    """n reads (n even) cut from a 3 000-base sequence G whose k-mers are the table, with counts 1 .. 5 in turn (min_count = 3
    makes some of them weak): the lengths k - 1, k, k + 1, k + 62, k + 63, k + 64, k + 126, k + 127, k + 128 -- 0, 1, 2, 63, 64,
    65, 127, 128, 129 windows -- in turn, with long_reads every tenth read 1 023 bases; every seventh read has a substitution
    (a stretch of weak windows), every eleventh an N, every thirteenth a lower-case letter (invalid windows); one read is empty"""
    rng = np.random.default_rng(1000 + k)
    G = rng.choice(_LETTERS, size=3000).tobytes()
    counts = {}
    for i in range(len(G) - k + 1):
        counts.setdefault(canonical(G[i:i + k]), 1 + i % 5)
    lens = [k - 1, k, k + 1, k + 62, k + 63, k + 64, k + 126, k + 127, k + 128]
    reads = []
    for r in range(n):
        L = 1023 if long_reads and r % 10 == 3 else lens[r % len(lens)]
        p = int(rng.integers(0, len(G) - L + 1))
        s = bytearray(G[p:p + L])
        if r % 7 == 0:
            q = int(rng.integers(0, L))
            s[q] = b"ACGT"[(b"ACGT".index(s[q]) + 1) % 4]
        if r % 11 == 0:
            s[int(rng.integers(0, L))] = ord("N")
        if r % 13 == 0:
            q = int(rng.integers(0, L))
            s[q] = s[q] | 0x20
        reads.append(bytes(s))
    reads[5] = b""
    return reads, counts


def group_sums(per_read, min_count):
    """restate() once per (half, parity) group of the reads: every mode's mates are unions of these"""
    n = len(per_read)
    g = {}
    for half in (0, 1):
        for par in (0, 1):
            idx = [i for i in range(n) if (i >= n // 2) == bool(half) and (i & 1) == par]
            g[half, par] = restate([per_read[i] for i in idx], [0] * len(idx), min_count)
    return g


def want_of(groups, mode):
    out = empty_counts()
    for (half, par), c in groups.items():
        m = 0 if mode == 0 else half if mode == 1 else par
        for f in FIELDS:
            out[f][m] += c[f][0]
    return out


@pytest.mark.parametrize("k", [15, 23, 32])
def test_device_profile_equals_the_restatement(k):
    """two arenas: 9 000 reads of at most k + 128 bases (max_read_len <= 259: the four-word instance; more reads than the
    grid has wavefronts, so a wavefront adds up several) and 3 000 with reads of 1 023 (the sixteen-word instance); lead 0, 1
    and 15 with letters around the arena; modes 0, 1, 2; min_count 1 and 3"""
    ctx = rcorrector_amd.Context(k=k, device=0)
    for n, long_reads in ((9000, False), (3000, True)):
        reads, counts = synthetic(k, n, long_reads)
        codes = np.array(sorted(counts), dtype=np.uint64)
        ctx.table_build(codes, np.array([counts[c] for c in codes.tolist()], dtype=np.int32))
        arena, off = rcorrector_amd.pack_reads(reads)
        max_len = max(len(r) for r in reads)
        assert max_len == (1023 if long_reads else k + 128) and (long_reads or max_len <= 259) and b"" in reads
        memo = {}
        per_read = [window_counts(r, k, counts, memo) for r in reads]
        assert {len(c) for c in per_read} >= {0, 1, 2, 63, 64, 65, 127, 128, 129}
        for min_count in (1, 3):
            groups = group_sums(per_read, min_count)
            for mode in (0, 1, 2):
                want = want_of(groups, mode)
                assert want["weak5"].sum() > 0 and want["solid5"].sum() > 0
                assert (want["windows"] - want["solid5"] - want["weak5"]).sum() > 0          # (invalid windows are there too)
                for lead in (0, 1, 15):
                    got = as_counts(device_counts(ctx, arena, off, mode, min_count, lead))
                    assert_counts(got, want, "k %d n %d mode %d min_count %d lead %d" % (k, n, mode, min_count, lead))
    ctx.sync()
    ctx.close()


def test_no_reads_leave_the_counts_alone_and_a_second_call_adds():
    import torch
    k = 23
    reads, counts = synthetic(k, 400, True)
    ctx = rcorrector_amd.Context(k=k, device=0)
    codes = np.array(sorted(counts), dtype=np.uint64)
    ctx.table_build(codes, np.array([counts[c] for c in codes.tolist()], dtype=np.int32))
    arena, off = rcorrector_amd.pack_reads(reads)
    want = restate_reads(reads, 2, k, counts, 1)
    t = device_counts(ctx, arena, off, 2, 1)
    assert_counts(as_counts(t), want, "first call")
    ctx.trust_profile_device(None, None, 0, 0, 0, 2, t, 1)                       # n_reads = 0: untouched
    ctx.sync()
    assert_counts(as_counts(t), want, "n_reads = 0")
    device_counts(ctx, arena, off, 2, 1, lead=3, into=t)                         # a second call adds
    assert_counts(as_counts(t), {f: 2 * want[f] for f in FIELDS}, "second call")
    # a max_read_len that understates the reads picks the four-word instance: the counts of the long reads are cut short, the
    # arrays are never left -- positions 256 and above stay as they were
    z = torch.zeros((5, 2, MAX_LEN), dtype=torch.int64, device="cuda")
    device_counts(ctx, arena, off, 0, 1, max_len=100, into=z)
    assert int(z[:, :, 256:].abs().sum()) == 0 and int(z[0, 0, :256].max()) == len([r for r in reads if len(r) >= k])
    ctx.sync()
    ctx.close()


def test_argument_and_state_errors():
    import torch
    f = fixture("fx_k15")
    L = rcorrector_amd.load_library()
    arena, off = rcorrector_amd.pack_reads(f["seqs1"][:8])
    t_seq, t_off = torch.from_numpy(arena).cuda(), torch.from_numpy(off.astype(np.int32)).cuda()
    t_out = torch.zeros((5, 2, MAX_LEN), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def dev(c, min_count=1, seq=t_seq.data_ptr(), n=8, nbytes=arena.size, max_len=100, mode=0, out=t_out.data_ptr()):
        return L.rc_trust_profile_device(c._h, seq, t_off.data_ptr(), n, nbytes, max_len, mode, min_count, out)

    bare = rcorrector_amd.Context(k=f["k"], device=0)
    assert dev(bare) == RC_STATUS_STATE and b"table" in L.rc_last_error(bare._h)          # no table
    assert L.rc_trust_profile_begin(bare._h, 1) == RC_STATUS_STATE                        # begin needs one too
    assert L.rc_trust_profile_get(bare._h, None) == RC_STATUS_STATE and L.rc_trust_profile_end(bare._h) == RC_STATUS_STATE
    bare.close()
    ctx = fixture_ctx(f)
    assert dev(ctx, 0) == RC_STATUS_ARG and dev(ctx, -3) == RC_STATUS_ARG                 # min_count < 1
    assert dev(ctx, seq=None) == RC_STATUS_ARG and dev(ctx, out=None) == RC_STATUS_ARG    # a null pointer with reads
    assert dev(ctx, mode=3) == RC_STATUS_ARG and dev(ctx, mode=-1) == RC_STATUS_ARG       # a mode outside 0 .. 2
    assert dev(ctx, mode=1, n=7) == RC_STATUS_ARG                                         # mode 1 with an odd n_reads
    assert dev(ctx, max_len=MAX_LEN) == RC_STATUS_ARG and dev(ctx, max_len=MAX_LEN - 1) == 0
    assert dev(ctx, nbytes=1 << 32) == RC_STATUS_ARG
    assert L.rc_trust_profile_device(ctx._h, None, None, 0, 0, 0, 0, 1, None) == 0
    ctx.sync()
    t_out.zero_()
    torch.cuda.synchronize()
    assert dev(ctx, mode=2, n=7) == 0                                                     # mode 2 takes an odd count: the last read is mate 0
    ctx.sync()
    assert_counts(as_counts(t_out), restate_reads(f["seqs1"][:7], 2, f["k"], f["counts_of"], 1), "seven reads, mode 2")
    # begin / get / end: the report's state errors
    assert L.rc_trust_profile_get(ctx._h, None) == RC_STATUS_STATE and L.rc_trust_profile_end(ctx._h) == RC_STATUS_STATE
    assert L.rc_trust_profile_begin(ctx._h, 0) == RC_STATUS_ARG
    ctx.trust_profile_begin(2)
    assert L.rc_trust_profile_begin(ctx._h, 1) == RC_STATUS_STATE and b"open already" in L.rc_last_error(ctx._h)
    assert L.rc_trust_profile_get(ctx._h, None) == RC_STATUS_ARG
    got = ctx.trust_profile()
    assert got["k"] == f["k"] and got["min_count"] == 2 and got["reads"].tolist() == [0, 0]
    assert all(int(got[v][x].sum()) == 0 for v in ("before", "after") for x in FIELDS)
    ctx.trust_profile_end()
    assert L.rc_trust_profile_end(ctx._h) == RC_STATUS_STATE
    ctx.sync()
    ctx.close()


# ---- 2. invariants on the golden fixtures --------------------------------------------------------------------------------------
_restated = {}


def fixture_restated(name, min_count=1):
    """(before, after) of a golden fixture: its reads, and the reference's corrected reads"""
    key = (name, min_count)
    if key not in _restated:
        f = fixture(name)
        memo = {}
        _restated[key] = tuple(restate_reads(s, f["mode"], f["k"], f["counts_of"], min_count, memo)
                               for s in (f["seqs1"] + f["seqs2"], f["cor1"] + f["cor2"]))
    return _restated[key]


@pytest.mark.parametrize("name", ["fx_k15", "fx_pe_k23", "fx_k32", "fx_edge"])
def test_invariants_on_golden_fixtures(name):
    f = fixture(name)
    ctx = fixture_ctx(f)
    want = fixture_restated(name)
    got = []
    for which, seqs in enumerate((f["seqs1"] + f["seqs2"], f["cor1"] + f["cor2"])):
        arena, off = rcorrector_amd.pack_reads(seqs)
        c = as_counts(device_counts(ctx, arena, off, f["mode"], 1))
        assert_counts(c, want[which], "%s version %d" % (name, which))
        for m in (0, 1):
            assert int(c["solid5"][m].sum()) == int(c["solid3"][m].sum()) and int(c["weak5"][m].sum()) == int(c["weak3"][m].sum())
            assert (c["solid5"][m] + c["weak5"][m] <= c["windows"][m]).all() and (c["solid3"][m] + c["weak3"][m] <= c["windows"][m]).all()
        # min_count = 1: the weak windows are those of the per-read profile, and the k-mers a recount finds absent
        weak = int(c["weak5"].sum())
        assert weak == int(device_profile(ctx, arena, off, 1)[:, 0].sum()) > 0
        ctx.recount_begin(100)
        ctx.recount_add(arena)
        assert weak == ctx.recount_finish()[1]["absent_total"]
        got.append(c)
    assert np.array_equal(got[0]["windows"], got[1]["windows"])                            # a correction changes no length
    assert int(got[1]["weak5"].sum()) < int(got[0]["weak5"].sum())                          # (and it did remove weak k-mers)
    assert (f["mode"] != 0) == bool(got[0]["windows"][1].sum())
    ctx.sync()
    ctx.close()
