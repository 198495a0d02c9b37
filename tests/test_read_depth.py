"""GPU: the per-read k-mer depth -- rc_read_depth_device / rc_read_depth_into and the binding's read_depth_* methods: for every
read its valid k-windows and the lower quartile, median and upper quartile of their counts (include/rcorrector_amd.h:
rc_read_depth).

The yardstick is `restate` below, pure Python over a dict {canonical k-mer code: count} (missing = 0) that is built from a
golden fixture's dump.jf, or from the arrays a synthetic table was built from -- never from the library.  The corrected reads of
the golden fixtures are the REFERENCE's (ref/*.cor.fq).  Every comparison is exact equality on all four fields of every read,
and every test ends with a sync of the context.
"""
import numpy as np
import pytest

import datasets
import rcorrector_amd
from seam_arena import canonical, seam_arena
from test_recount import packed, unit_cuts
from test_weak_profile import (RC_STATUS_ARG, RC_STATUS_NOSPACE, RC_STATUS_STATE, device_profile, fixture, fixture_ctx, packed_inputs,
                               single_end)
from test_weak_profile import out_array as weak_out_array

pytestmark = pytest.mark.gpu
_ACGT = frozenset(b"ACGT")
TOP = (1 << 27) - 1


def restate(seq, k, counts):
    """the feature's contract for one read: (valid, q1, median, q3)"""
    c = sorted(counts.get(canonical(seq[i:i + k]), 0) for i in range(len(seq) - k + 1) if _ACGT.issuperset(seq[i:i + k]))
    n = len(c)
    return (n, c[(n - 1) // 4], c[(n - 1) // 2], c[3 * (n - 1) // 4]) if n else (0, 0, 0, 0)


def restate_all(seqs, k, counts):
    return np.array([restate(s, k, counts) for s in seqs], dtype=np.int32).reshape(len(seqs), 4)


def device_depth(ctx, arena, off, lead=0, max_len=None):
    """rc_read_depth_device on a copy of `arena` that starts `lead` bytes behind a 16-byte boundary of device memory; the bytes
    in front of it and behind it are letters, not NULs: what the kernel may read there must not count"""
    import torch
    n = len(off) - 1
    buf = torch.full((lead + arena.size + 64,), ord("A"), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if arena.size:
        buf[lead:lead + arena.size] = torch.from_numpy(np.ascontiguousarray(arena)).cuda()
    t_off = torch.from_numpy(np.asarray(off).astype(np.int32)).cuda()
    out = torch.full((max(n, 1), 4), -7, dtype=torch.int32, device="cuda")
    if max_len is None:
        max_len = int(np.diff(np.asarray(off).astype(np.int64)).max()) - 1 if n else 0
    torch.cuda.synchronize()
    ctx.read_depth_device(buf.data_ptr() + lead, t_off, n, arena.size, max_len, out)
    ctx.sync()
    return out.cpu().numpy()[:n]


def assert_depth(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.int32, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "%s: read %d: got %s, want %s (%d reads differ)" % (what, bad[0], got[bad[0]], want[bad[0]], len(bad))
    assert (got[:, 1] <= got[:, 2]).all() and (got[:, 2] <= got[:, 3]).all()


# ---- 1. the device entry point against the restatement on golden fixtures ------------------------------------------------------
# what each fixture must go on exercising: spread = a read with q1 < median < q3, novalid = a read without a valid window,
# zero = a read with valid windows whose median is 0, parity = the parities of n that occur
FIXTURES = {
    "fx_highcov": dict(spread=True),
    "fx_skew": dict(spread=True),
    "fx_edge": dict(spread=True, novalid=True, zero=True, parity={0, 1}),
    "fx_k15": dict(spread=True, parity={1}),
    "fx_k32": dict(spread=True, parity={1}),
    "fx_pe_k23": dict(spread=True, parity={0}),
    "fx_varlen_n": dict(spread=True, novalid=True, parity={0, 1}),
}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_device_depth_equals_the_restatement_on_golden_fixtures(name):
    f = fixture(name)
    ctx = fixture_ctx(f)
    changed, seen = 0, []
    for which, seqs in (("uncorrected", f["seqs1"] + f["seqs2"]), ("corrected", f["cor1"] + f["cor2"])):
        arena, off = rcorrector_amd.pack_reads(seqs)
        changed += which == "corrected" and seqs != f["seqs1"] + f["seqs2"]
        want = restate_all(seqs, f["k"], f["counts_of"])
        print("%s %s: %d reads, %d without a valid window, %d distinct medians, max count %d" %
              (name, which, len(seqs), int((want[:, 0] == 0).sum()), len(set(want[want[:, 0] > 0, 2].tolist())), int(want[:, 3].max())))
        assert_depth(device_depth(ctx, arena, off), want, "%s %s" % (name, which))
        seen.append(want)
    assert changed == 1
    want, p = np.concatenate(seen), FIXTURES[name]
    # (a regenerated fixture cannot empty the test)
    assert ((want[:, 1] < want[:, 2]) & (want[:, 2] < want[:, 3])).any()
    if p.get("novalid"):
        assert (want[:, 0] == 0).any()
    if p.get("zero"):
        assert ((want[:, 0] > 0) & (want[:, 2] == 0)).any()
    if "parity" in p:
        assert set((want[want[:, 0] > 0, 0] % 2).tolist()) == p["parity"]
    if name == "fx_highcov":
        assert (seen[0][:, 1] < seen[0][:, 3]).all() and len(set(seen[0][:, 2].tolist())) > 100 and seen[0][:, 3].max() > 5000
    ctx.sync()
    ctx.close()


# ---- 2. synthetic arenas over table_build tables -------------------------------------------------------------------------------
def synthetic(k=23):
    """reads and the {code: count} dict of their table: every rank index, the longest read, the extreme counts, letters outside ACGT"""
    rng = np.random.default_rng(20250307)
    letters = np.frombuffer(b"ACGT", np.uint8)
    G = rng.choice(letters, size=1100).tobytes()
    counts = {}
    for i in range(len(G) - k + 1):
        counts.setdefault(canonical(G[i:i + k]), 2 + int(rng.integers(0, 40)) ** 2)
    reads = [G[50:50 + n] for n in (k - 1, k, k + 1, k + 2, k + 3, k + 4)]          # n = 0 .. 5 windows
    reads.append(G[3:3 + 1023])                                                      # the longest read the library takes
    alt = rng.choice(letters, size=300).tobytes()                                    # absent k-mers and 2^27 - 1, window by window
    for i in range(0, len(alt) - k + 1, 2):
        counts[canonical(alt[i:i + k])] = TOP
    reads.append(alt)
    reads.append(b"N" + G[101:160] + b"N" + G[161:200] + b"acgt" + G[204:300] + b"n" + G[301:340] + b"N")
    reads.append(b"NNNN" + G[0:k - 1])                                               # bases, but no valid window
    reads.append(b"")
    reads += [G[j:j + 150] for j in range(0, 900, 7)]                                # more than two workgroups' worth of ordinary reads
    return k, reads, counts


def table_of(ctx, counts):
    codes = np.array(sorted(counts), dtype=np.uint64)
    ctx.table_build(codes, np.array([counts[int(c)] for c in codes], dtype=np.int32))


@pytest.mark.parametrize("lead", range(16))
def test_device_depth_on_a_synthetic_arena_at_every_lead(lead):
    k, reads, counts = synthetic()
    ctx = rcorrector_amd.Context(k=k, device=0)
    table_of(ctx, counts)
    want = restate_all(reads, k, counts)
    assert want[:6, 0].tolist() == [0, 1, 2, 3, 4, 5] and want[6, 0] == 1001
    assert want[7, 1] == 0 and want[7, 3] == TOP and want[7, 2] in (0, TOP)
    assert 0 < want[8, 0] < len(reads[8]) - k + 1 and tuple(want[9]) == (0, 0, 0, 0) and tuple(want[10]) == (0, 0, 0, 0)
    assert len(reads) > 2 * 64 + 1
    arena, off = rcorrector_amd.pack_reads(reads)
    assert_depth(device_depth(ctx, arena, off, lead), want, "lead %d" % lead)
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("lead", [0, 5, 15])
def test_device_depth_at_the_tile_seams(lead):
    k, reads, counts = seam_arena()
    arena, off = rcorrector_amd.pack_reads(reads)
    ctx = rcorrector_amd.Context(k=k, device=0)
    table_of(ctx, counts)
    assert_depth(device_depth(ctx, arena, off, lead), restate_all(reads, k, counts), "lead %d" % lead)
    ctx.sync()
    ctx.close()


def test_read_counts_around_a_workgroup_and_offsets_that_leave_the_arena():
    k, reads, counts = synthetic()
    ctx = rcorrector_amd.Context(k=k, device=0)
    table_of(ctx, counts)
    long_reads = [reads[6]] * 9                                   # 1 023-base reads: a workgroup's 64 reads take many tiles
    for seqs in ([], reads[11:12], reads[11:11 + 64], reads[11:11 + 65], long_reads + reads[11:11 + 60] + long_reads):
        arena, off = rcorrector_amd.pack_reads(seqs)
        assert_depth(device_depth(ctx, arena, off, 3), restate_all(seqs, k, counts), "%d reads" % len(seqs))
    # an offset pair that leaves the arena, or that runs backwards, describes no read; the reads beside it are not disturbed
    seqs = reads[11:11 + 10]
    arena, off = rcorrector_amd.pack_reads(seqs)
    want = restate_all(seqs, k, counts)
    bad = off.astype(np.int64).copy()
    bad[4] = arena.size + 1000                                    # read 3 ends, read 4 starts, outside
    want[3] = want[4] = 0
    assert_depth(device_depth(ctx, arena, bad.astype(np.uint32), 0, max_len=150), want, "offsets outside")
    # a read longer than the limit that max_read_len promised: no read either, whatever the caller said
    seqs = [reads[11], reads[6] + reads[6][:100], reads[12]]
    arena, off = rcorrector_amd.pack_reads(seqs)
    want = restate_all(seqs, k, counts)
    want[1] = 0
    assert_depth(device_depth(ctx, arena, off, 0, max_len=150), want, "a read beyond the limit")
    ctx.sync()
    ctx.close()


def test_device_depth_on_a_table_with_extension_bits():
    d = datasets.k_sweep(27, 0, 120_000)            # as tests/test_k_sweep.py builds its k = 27 case
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    ctx.table_build(d["keys"], d["counts"])
    assert ctx.table_layout() == 1 and ctx.table_stats()["buckets"] < 1 << (2 * d["k"] - 32)   # the remainder borrows count bits
    counts = dict(zip(np.asarray(d["keys"]).tolist(), np.asarray(d["counts"]).tolist()))
    seqs = [bytes(s) for s in list(d["seqs1"]) + list(d["seqs2"] or [])]
    arena, off = rcorrector_amd.pack_reads(seqs)
    want = restate_all(seqs, d["k"], counts)
    assert (want[:, 2] > 0).any()
    assert_depth(device_depth(ctx, arena, off), want, "packed_ext")
    ctx.sync()
    ctx.close()


# ---- 3. slots ------------------------------------------------------------------------------------------------------------------
# Each result must equal rc_read_depth_device on the same corrected reads: the arena a batch leaves behind (a packed / resident
# batch: the caller's arena with the fix list applied), through the entry point that sections 1 and 2 hold to the restatement.
def depth_of(ctx, arena, off):
    return device_depth(ctx, np.ascontiguousarray(arena), off)


def out_array(ctx, slot, total, pinned):
    out = ctx.read_depth_into(slot, total) if pinned else ctx.read_depth_into(slot, total, out=np.zeros((total, 4), dtype=np.int32))
    out[:] = -9
    return out


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "host_array"])
def test_depth_into_through_submit_and_packed_with_the_weak_profile_beside_it(pinned):
    f = fixture("fx_pe_k23")
    ctx = fixture_ctx(f)
    corrected_bases = 0
    for d in (f, single_end(f)):
        for lo, hi in unit_cuts(d, 2):
            a, qa, off, _, args = packed(rcorrector_amd, d, lo, hi)
            total = len(off) - 1
            # rc_submit / rc_wait, slot 0, the weak profile alone: what it must also be with the depth beside it
            weak_alone = weak_out_array(ctx, 0, total, 2, pinned)
            before = a.copy()
            ctx.submit(0, d["mode"], *args)
            ctx.wait(0)
            cor = np.concatenate(args[0::3])
            corrected_bases += int((cor != before).sum())
            want = depth_of(ctx, cor, off)
            assert (want[:, 0] > 0).any() and (weak_alone != -9).all()
            # both registrations on one submit, in a lane
            a, qa, off, _, args = packed(rcorrector_amd, d, lo, hi)
            weak, out = weak_out_array(ctx, 1, total, 2, pinned), out_array(ctx, 1, total, pinned)
            ctx.submit(1, d["mode"], *args)
            ctx.wait(1)
            assert np.array_equal(np.concatenate(args[0::3]), cor)
            assert_depth(out, want, "mode %d submit" % d["mode"])
            assert np.array_equal(weak, weak_alone) and np.array_equal(weak, device_profile(ctx, cor, off, 2))
            # rc_submit_packed / rc_wait_packed
            a, qa, off, _, _ = packed(rcorrector_amd, d, lo, hi)
            arena, bases, exc_pos, exc_chr, qb = packed_inputs(ctx, a, qa, f["bad_q"])
            out = out_array(ctx, 2, total, pinned)
            ctx.submit_packed(2, d["mode"], a.size, off, bases, qb, exc_pos, exc_chr)
            r = ctx.wait_packed(2)
            ctx.apply_fixes(arena, r[4], r[5])
            assert np.array_equal(arena, cor)
            assert_depth(out, want, "mode %d packed" % d["mode"])
    assert corrected_bases > 0
    ctx.sync()
    ctx.close()


def test_depth_into_through_the_resident_transport():
    import os
    import golden_util as gu
    d = fixture("fx_pe_k23")
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    a1, off1 = rcorrector_amd.pack_reads(d["seqs1"])
    a2, off2 = rcorrector_amd.pack_reads(d["seqs2"])
    q = [rcorrector_amd.pack_reads(d["quals1"])[0], rcorrector_amd.pack_reads(d["quals2"])[0]]
    ctx.count_keep(True)
    ctx.count_begin()
    ctx.count_add(a1)
    ctx.count_add(a2)
    off = np.concatenate([off1, (off2[1:].astype(np.int64) + a1.size).astype(np.uint32)])
    ctx.count_finish(2)
    ctx.load_jfdump(os.path.join(gu.GOLDEN, d["name"], "dump.jf"))
    ctx.set_run_params(ctx.estimate_error_rate(0.95), d["bad_q"])
    qb = ctx.host_array((int(off[-1]) + 7) // 8)
    ctx.pack_quality_bits(np.concatenate(q), d["bad_q"], out=qb)
    for slot, pinned in ((0, True), (3, False)):
        out = out_array(ctx, slot, len(off) - 1, pinned)
        ctx.submit_resident(slot, 1, off, qb, arena_a=0, begin_a=0, bytes_a=a1.size, arena_b=1, begin_b=0, bytes_b=a2.size)
        r = ctx.wait_resident(slot)
        host = np.concatenate([a1, a2])
        assert len(r[4]) > 0
        ctx.apply_fixes(host, r[4], r[5])
        assert_depth(out, depth_of(ctx, host, off), "resident slot %d" % slot)
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("lanes", [True, False], ids=["lanes_on", "lanes_off"])
def test_four_slots_in_flight(lanes):
    f = fixture("fx_pe_k23")
    ctx = fixture_ctx(f)
    ctx.set_slot_lanes(lanes)
    outs, keep = [], []
    for s, (lo, hi) in enumerate(unit_cuts(f, 4)):
        a, qa, off, _, args = packed(rcorrector_amd, f, lo, hi)
        keep.append((args, off))
        outs.append(out_array(ctx, s, len(off) - 1, pinned=s < 2))
        ctx.submit(s, f["mode"], *args)
    for s in (3, 1, 0, 2):
        ctx.wait(s)
    for s, (args, off) in enumerate(keep):
        assert_depth(outs[s], depth_of(ctx, np.concatenate(args[0::3]), off), "slot %d, lanes %s" % (s, lanes))
    ctx.sync()
    ctx.close()


def test_a_batch_resubmitted_after_nospace_is_profiled_once_then():
    f = fixture("fx_pe_k23")
    ctx = fixture_ctx(f)
    n = len(f["seqs1"])
    a, qa, off, _, _ = packed(rcorrector_amd, f, 0, n)
    arena, bases, exc_pos, exc_chr, qb = packed_inputs(ctx, a, qa, f["bad_q"])
    L, h = rcorrector_amd.load_library(), ctx._h
    out = out_array(ctx, 1, 2 * n, pinned=False)
    ctx.profile(True)
    ctx.profile_reset()
    ctx.submit_packed(1, f["mode"], a.size, off, bases, qb, exc_pos, exc_chr, fix_pos=np.zeros(0, np.uint32), fix_chr=np.zeros(0, np.uint8))   # fix_cap = 0
    assert L.rc_wait_packed(h, 1) == RC_STATUS_NOSPACE
    ctx._inflight_packed.pop(1)
    assert (out == -9).all()                      # (a pageable array is written by the wait that succeeds, and only by it)
    launches_refused = ctx.profile_get(7)[1]
    # the registration went with that submit: without a new one the resubmitted batch leaves the array alone and launches nothing
    ctx.submit_packed(1, f["mode"], a.size, off, bases, qb, exc_pos, exc_chr)
    ctx.wait_packed(1)
    assert (out == -9).all() and ctx.profile_get(7)[1] == launches_refused == 1
    out = out_array(ctx, 1, 2 * n, pinned=False)
    ctx.submit_packed(1, f["mode"], a.size, off, bases, qb, exc_pos, exc_chr)
    res = ctx.wait_packed(1)
    assert ctx.profile_get(7)[1] == launches_refused + 1
    host = a.copy()
    ctx.apply_fixes(host, res[4], res[5])
    ctx.profile(False)
    assert_depth(out, depth_of(ctx, host, off), "resubmitted")
    ctx.sync()
    ctx.close()


def test_a_registration_changes_nothing_else_is_one_shot_and_can_be_withdrawn():
    f = fixture("fx_pe_k23")
    n = len(f["seqs1"])

    def run(register):
        ctx = fixture_ctx(f)
        digest = ctx.table_digest()
        outs = []
        for slot in (0, 2):
            a, qa, off, _, args = packed(rcorrector_amd, f, 0, n)
            out = out_array(ctx, slot, 2 * n, pinned=slot == 0) if register else None
            ctx.submit(slot, f["mode"], *args)
            res = ctx.wait(slot)
            outs.append((out, [r.copy() for r in res], args[0].copy(), args[3].copy()))
        if register:
            first = outs[0][0].copy()
            assert (first != -9).all()
            a, qa, off, _, args = packed(rcorrector_amd, f, 0, n // 2)   # no registration: the earlier array stays as it is
            ctx.submit(0, f["mode"], *args)
            ctx.wait(0)
            assert np.array_equal(outs[0][0], first)
            withdrawn = out_array(ctx, 0, 2 * n, pinned=True)
            ctx.read_depth_withdraw(0)
            a, qa, off, _, args = packed(rcorrector_amd, f, 0, n // 2)
            ctx.submit(0, f["mode"], *args)
            ctx.wait(0)
            assert np.array_equal(outs[0][0], first) and (withdrawn == -9).all()
        else:
            for _ in range(2):
                a, qa, off, _, args = packed(rcorrector_amd, f, 0, n // 2)
                ctx.submit(0, f["mode"], *args)
                ctx.wait(0)
        state = (ctx.summary(), ctx.table_digest() == digest)
        ctx.sync()
        ctx.close()
        return outs, state

    with_reg, st1 = run(True)
    without, st0 = run(False)
    assert st1 == st0 and st1[1]
    for (out, res, s1, s2), (_, res0, s10, s20) in zip(with_reg, without):
        assert all(np.array_equal(x, y) for x, y in zip(res, res0)) and np.array_equal(s1, s10) and np.array_equal(s2, s20)


# ---- 4. errors -----------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors():
    import torch
    f = fixture("fx_k15")
    L = rcorrector_amd.load_library()
    arena, off = rcorrector_amd.pack_reads(f["seqs1"][:8])
    t_seq, t_off = torch.from_numpy(arena).cuda(), torch.from_numpy(off.astype(np.int32)).cuda()
    t_out = torch.zeros((8, 4), dtype=torch.int32, device="cuda")
    host = np.zeros((8, 4), dtype=np.int32)
    torch.cuda.synchronize()

    def dev(c, seq=t_seq.data_ptr(), off_p=t_off.data_ptr(), out=t_out.data_ptr(), nbytes=arena.size, max_len=100):
        return L.rc_read_depth_device(c._h, seq, off_p, 8, nbytes, max_len, out)

    bare = rcorrector_amd.Context(k=f["k"], device=0)
    assert dev(bare) == RC_STATUS_STATE                                       # no table
    assert L.rc_read_depth_into(bare._h, 0, host.ctypes.data) == RC_STATUS_STATE
    assert b"table" in L.rc_last_error(bare._h)
    assert L.rc_read_depth_into(bare._h, 0, None) == 0                        # withdrawing needs none
    bare.close()
    ctx = fixture_ctx(f)
    assert dev(ctx, seq=None) == RC_STATUS_ARG and dev(ctx, off_p=None) == RC_STATUS_ARG and dev(ctx, out=None) == RC_STATUS_ARG
    assert dev(ctx, nbytes=1 << 32) == RC_STATUS_ARG and b"4 GiB" in L.rc_last_error(ctx._h)
    assert dev(ctx, max_len=1024) == RC_STATUS_ARG and dev(ctx, max_len=1023) == 0   # the library's read limit
    assert L.rc_read_depth_device(ctx._h, None, None, 0, 0, 0, None) == 0
    assert L.rc_read_depth_into(ctx._h, 4, host.ctypes.data) == RC_STATUS_ARG        # slots are 0 .. 3
    assert L.rc_read_depth_into(ctx._h, -1, host.ctypes.data) == RC_STATUS_ARG
    assert dev(ctx) == 0
    ctx.sync()
    assert_depth(t_out.cpu().numpy(), restate_all(f["seqs1"][:8], f["k"], f["counts_of"]))
    ctx.close()
