"""GPU: the per-read weak-k-mer profile -- rc_weak_profile_device / rc_weak_profile_into and the binding's weak_profile_*
methods: for every read its weak windows, bad prefix, bad suffix and uncovered bases (include/rcorrector_amd.h: rc_read_weak).

The yardstick is `restate` below, a dozen lines of pure Python over a dict {canonical k-mer code: count} (missing = 0) that is
built from a golden fixture's dump.jf, or from the arrays a synthetic table was built from -- never from the library.  The
corrected reads of the golden fixtures are the REFERENCE's (ref/*.cor.fq).  Every comparison is exact integer equality, and every
test ends with a sync of the context.
"""
import os
import re

import numpy as np
import pytest

import datasets
import golden_util as gu
import rcorrector_amd
from seam_arena import canonical, seam_arena
from test_recount import packed, unit_cuts

pytestmark = pytest.mark.gpu
RC_STATUS_ARG, RC_STATUS_STATE, RC_STATUS_NOSPACE = -1, -4, -6
_ACGT = frozenset(b"ACGT")


def restate(seq, k, counts, min_count):
    """section 1 of the feature's contract for one read: (weak, bad_prefix, bad_suffix, uncovered)"""
    L, weak, solid = len(seq), 0, []
    for i in range(L - k + 1):
        w = seq[i:i + k]
        if not _ACGT.issuperset(w):
            continue                                   # invalid: neither solid nor weak
        if counts.get(canonical(w), 0) >= min_count:
            solid.append(i)
        else:
            weak += 1
    if not solid:
        return (weak, L, L, L)
    covered = set()
    for i in solid:
        covered.update(range(i, i + k))
    return (weak, solid[0], L - (solid[-1] + k), L - len(covered))


def restate_all(seqs, k, counts, min_count):
    return np.array([restate(s, k, counts, min_count) for s in seqs], dtype=np.int32).reshape(len(seqs), 4)


# ---- golden fixtures: reads, the reference's corrected reads, the dump as a dict ------------------------------------------------
def fastx_seqs(path):
    lines = open(path, "rb").read().split(b"\n")
    step = 4 if lines[0].startswith(b"@") else 2
    n = len(lines) // step
    return [lines[step * i + 1] for i in range(n)], ([lines[step * i + 3] for i in range(n)] if step == 4 else None)


def dump_counts(name):
    d, cnt = {}, 0
    for ln in open(os.path.join(gu.GOLDEN, name, "dump.jf"), "rb").read().split():
        if ln.startswith(b">"):
            cnt = int(ln[1:])
        else:
            d[canonical(ln)] = cnt                       # (a k-mer put twice keeps its last count, Store.h:55)
    return d


_fixture_cache = {}


def fixture(name):
    """a golden fixture as the dict test_recount's batch helpers take, plus the reference's corrected reads and the dump's counts"""
    if name in _fixture_cache:
        return _fixture_cache[name]
    d = os.path.join(gu.GOLDEN, name)
    args = open(os.path.join(d, "cmd.txt")).read().split()
    k = int(args[args.index("-k") + 1])
    f = dict(k=k, mfk=4, name=name, counts_of=dump_counts(name), seqs2=[], quals2=[], cor2=[])
    if "-p" in args:
        i = args.index("-p")
        f["mode"] = 1
        f["seqs1"], f["quals1"] = fastx_seqs(os.path.join(d, args[i + 1]))
        f["seqs2"], f["quals2"] = fastx_seqs(os.path.join(d, args[i + 2]))
        outs = [args[i + 1], args[i + 2]]
    else:
        flag = "-i" if "-i" in args else "-r"
        f["mode"] = 2 if flag == "-i" else 0
        f["seqs1"], f["quals1"] = fastx_seqs(os.path.join(d, args[args.index(flag) + 1]))
        outs = [args[args.index(flag) + 1]]
    cor = [fastx_seqs(os.path.join(d, "ref", "%s.cor%s" % os.path.splitext(o)))[0] for o in outs]
    f["cor1"], f["cor2"] = cor[0], (cor[1] if len(cor) > 1 else [])
    f["bad_q"] = re.search(rb"Bad quality threshold is '(.)'", open(os.path.join(d, "ref", "stderr.txt"), "rb").read(), re.S).group(1)
    _fixture_cache[name] = f
    return f


def fixture_ctx(f):
    ctx = rcorrector_amd.Context(k=f["k"], max_fix_per_k=f["mfk"], device=0)
    ctx.load_jfdump(os.path.join(gu.GOLDEN, f["name"], "dump.jf"))
    f["rate"] = ctx.estimate_error_rate(0.95)
    ctx.set_run_params(f["rate"], f["bad_q"])
    return ctx


def device_profile(ctx, arena, off, min_count, lead=0):
    """rc_weak_profile_device on a copy of `arena` that starts `lead` bytes behind a 16-byte boundary of device memory; the bytes
    in front of it and behind it are letters, not NULs: what the kernel may read there must not count"""
    import torch
    n = len(off) - 1
    buf = torch.full((lead + arena.size + 64,), ord("A"), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if arena.size:
        buf[lead:lead + arena.size] = torch.from_numpy(np.ascontiguousarray(arena)).cuda()
    t_off = torch.from_numpy(np.asarray(off).astype(np.int32)).cuda()
    out = torch.full((max(n, 1), 4), -7, dtype=torch.int32, device="cuda")
    max_len = int(np.diff(np.asarray(off).astype(np.int64)).max()) - 1 if n else 0
    torch.cuda.synchronize()
    ctx.weak_profile_device(buf.data_ptr() + lead, t_off, n, arena.size, max_len, out, min_count)
    ctx.sync()
    return out.cpu().numpy()[:n]


def assert_profile(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.int32, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "%s: read %d: got %s, want %s (%d reads differ)" % (what, bad[0], got[bad[0]], want[bad[0]], len(bad))


# ---- 1. the device entry point against the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fx_k15", "fx_pe_k23", "fx_k32", "fx_edge"])
def test_device_profile_equals_the_restatement_on_golden_fixtures(name):
    f = fixture(name)
    ctx = fixture_ctx(f)
    changed = 0
    for which, seqs in (("uncorrected", f["seqs1"] + f["seqs2"]), ("corrected", f["cor1"] + f["cor2"])):
        arena, off = rcorrector_amd.pack_reads(seqs)
        changed += which == "corrected" and seqs != f["seqs1"] + f["seqs2"]
        for min_count in (1, 3):
            want = restate_all(seqs, f["k"], f["counts_of"], min_count)
            assert_profile(device_profile(ctx, arena, off, min_count), want, "%s %s min_count %d" % (name, which, min_count))
            has = want[:, 1] < np.array([len(s) for s in seqs])      # reads with a solid window: the contract's own invariant
            assert (want[has, 1] + want[has, 2] <= want[has, 3]).all() and (want[:, 3] <= [len(s) for s in seqs]).all()
            assert want[:, 0].sum() > 0 and has.any()                  # (the fixture exercises both kinds of window)
    assert changed == 1
    ctx.sync()
    ctx.close()


# ---- 2. a synthetic arena aimed at the kernel's seams ---------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1, 7, 15])
def test_device_profile_at_the_kernels_seams(lead):
    k, reads, counts = seam_arena()
    arena, off = rcorrector_amd.pack_reads(reads)
    assert arena.size % 16 != 0 and arena.size > 4 * 4096
    starts = set(off[:-1].tolist())
    assert {4096 - 46, 8192 - 46, 2 * 4096 + 4096, 4 * 4096 - 1} <= starts and (3 * 4096 - 1) in set((off[1:] - 1).tolist())
    ctx = rcorrector_amd.Context(k=k, device=0)
    codes = np.array(sorted(counts), dtype=np.uint64)
    ctx.table_build(codes, np.full(len(codes), 5, dtype=np.int32))
    for min_count in (1, 6):
        want = restate_all(reads, k, counts, min_count)
        assert_profile(device_profile(ctx, arena, off, min_count, lead), want, "lead %d min_count %d" % (lead, min_count))
    want = restate_all(reads, k, counts, 1)
    lens = np.array([len(r) for r in reads])
    assert (want[lens < k] == np.stack([np.zeros_like(lens), lens, lens, lens], axis=1)[lens < k]).all()
    gap = reads.index(next(r for r in reads if len(r) == 110))
    assert tuple(want[gap]) == (52, 0, 0, 30)   # (the yardstick itself: 52 windows touch the junk, its 30 bases are uncovered)
    ctx.sync()
    ctx.close()


# ---- 3. table layouts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["wide", "packed", "packed_ext"])
def test_device_profile_on_every_table_layout(layout, monkeypatch):
    if layout == "wide":
        monkeypatch.setenv("RC_TABLE_LAYOUT", "wide")   # (read when the context is made)
        d = datasets.make("pe_k23")
    elif layout == "packed":
        d = datasets.make("k15")
    else:
        d = datasets.k_sweep(27, 0, 120_000)            # as tests/test_k_sweep.py builds its k = 27 case
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    monkeypatch.delenv("RC_TABLE_LAYOUT", raising=False)
    ctx.table_build(d["keys"], d["counts"])
    assert ctx.table_layout() == (0 if layout == "wide" else 1)
    if layout == "packed_ext":
        assert ctx.table_stats()["buckets"] < 1 << (2 * d["k"] - 32)   # the remainder borrows count bits
    elif layout == "packed":
        assert ctx.table_stats()["buckets"] >= 1 << max(0, 2 * d["k"] - 32)
    counts = dict(zip(np.asarray(d["keys"]).tolist(), np.asarray(d["counts"]).tolist()))
    seqs = [bytes(s) for s in list(d["seqs1"]) + list(d["seqs2"] or [])]
    arena, off = rcorrector_amd.pack_reads(seqs)
    for min_count in (1, 3):
        want = restate_all(seqs, d["k"], counts, min_count)
        assert min_count == 1 or (want[:, 0].sum() > 0 and (want[:, 1] == 0).any())
        assert_profile(device_profile(ctx, arena, off, min_count), want, "%s min_count %d" % (layout, min_count))
    ctx.sync()
    ctx.close()


# ---- 4. the census invariant ---------------------------------------------------------------------------------------------------
def test_weak_windows_add_up_to_the_recounts_absent_total():
    f = fixture("fx_pe_k23")
    ctx = fixture_ctx(f)
    arena, off = rcorrector_amd.pack_reads(f["cor1"] + f["cor2"])
    got = device_profile(ctx, arena, off, 1)
    ctx.recount_begin(100)
    ctx.recount_add(arena)
    _, st = ctx.recount_finish()
    assert int(got[:, 0].sum()) == st["absent_total"] > 0
    ctx.sync()
    ctx.close()


# ---- 5. slots ------------------------------------------------------------------------------------------------------------------
# Each result must equal rc_weak_profile_device on the same corrected reads: the arena a batch leaves behind (a packed / resident
# batch: the caller's arena with the fix list applied), profiled by the entry point that section 1 holds to the restatement.
def profile_of(ctx, arena, off, min_count):
    return device_profile(ctx, np.ascontiguousarray(arena), off, min_count)


def out_array(ctx, slot, total, min_count, pinned):
    if pinned:
        out = ctx.weak_profile_into(slot, total, min_count)
    else:
        out = ctx.weak_profile_into(slot, total, min_count, out=np.zeros((total, 4), dtype=np.int32))
    out[:] = -9
    return out


def packed_inputs(ctx, a, qa, bad_q):
    arena = ctx.host_array(a.size)
    arena[:] = a
    bases, exc_pos, exc_chr = ctx.pack_bases(arena, bases=ctx.host_array((a.size + 15) // 16, np.uint32))
    qb = ctx.host_array((a.size + 7) // 8)
    ctx.pack_quality_bits(qa, bad_q, out=qb)
    return arena, bases, exc_pos, exc_chr, qb


def single_end(f):
    """the first mates of a paired fixture as a mode-0 data set"""
    return dict(f, mode=0, seqs2=[], quals2=[])


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "host_array"])
@pytest.mark.parametrize("name", ["fx_pe_k23", "fx_il_k23"])
def test_profile_into_through_correct_batch_submit_and_packed(name, pinned):
    """modes 1 and 2 whole, mode 0 as the first mates alone; two batches each"""
    f = fixture(name)
    ctx = fixture_ctx(f)
    corrected_bases = 0
    for d in ([f, single_end(f)] if name == "fx_pe_k23" else [f]):
        for lo, hi in unit_cuts(d, 2):
            # rc_correct_batch (slot 0)
            a, qa, off, _, args = packed(rcorrector_amd, d, lo, hi)
            total = len(off) - 1
            out = out_array(ctx, 0, total, 1, pinned)
            before = a.copy()                          # (outside mode 1 `a` IS args[0], which the batch corrects in place)
            ctx.correct_batch(d["mode"], *args)
            cor = np.concatenate(args[0::3])
            corrected_bases += int((cor != before).sum())
            want = profile_of(ctx, cor, off, 1)
            assert_profile(out, want, "%s mode %d correct_batch" % (name, d["mode"]))
            # rc_submit / rc_wait in a lane
            a, qa, off, _, args = packed(rcorrector_amd, d, lo, hi)
            out = out_array(ctx, 1, total, 1, pinned)
            ctx.submit(1, d["mode"], *args)
            ctx.wait(1)
            assert np.array_equal(np.concatenate(args[0::3]), cor)
            assert_profile(out, want, "%s mode %d submit" % (name, d["mode"]))
            # rc_submit_packed / rc_wait_packed
            a, qa, off, _, _ = packed(rcorrector_amd, d, lo, hi)
            arena, bases, exc_pos, exc_chr, qb = packed_inputs(ctx, a, qa, f["bad_q"])
            out = out_array(ctx, 2, total, 1, pinned)
            ctx.submit_packed(2, d["mode"], a.size, off, bases, qb, exc_pos, exc_chr)
            r = ctx.wait_packed(2)
            ctx.apply_fixes(arena, r[4], r[5])
            assert np.array_equal(arena, cor)
            assert_profile(out, want, "%s mode %d packed" % (name, d["mode"]))
    assert corrected_bases > 0
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_profile_into_through_the_resident_transport(mode):
    f = fixture("fx_il_k23" if mode == 2 else "fx_pe_k23")
    d = single_end(f) if mode == 0 else f
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    a1, off1 = rcorrector_amd.pack_reads(d["seqs1"])
    q = [rcorrector_amd.pack_reads(d["quals1"])[0]]
    ctx.count_keep(True)
    ctx.count_begin()
    ctx.count_add(a1)
    off, args, arenas = off1, dict(arena_a=0, begin_a=0, bytes_a=a1.size), [a1]
    if mode == 1:
        a2, off2 = rcorrector_amd.pack_reads(d["seqs2"])
        q.append(rcorrector_amd.pack_reads(d["quals2"])[0])
        ctx.count_add(a2)
        off = np.concatenate([off1, (off2[1:].astype(np.int64) + a1.size).astype(np.uint32)])
        args.update(arena_b=1, begin_b=0, bytes_b=a2.size)
        arenas.append(a2)
    ctx.count_finish(2)
    ctx.load_jfdump(os.path.join(gu.GOLDEN, d["name"], "dump.jf"))
    ctx.set_run_params(ctx.estimate_error_rate(0.95), d["bad_q"])
    nbytes = int(off[-1])
    qb = ctx.host_array((nbytes + 7) // 8)
    ctx.pack_quality_bits(np.concatenate(q), d["bad_q"], out=qb)
    for slot, pinned in ((0, True), (3, False)):
        out = out_array(ctx, slot, len(off) - 1, 3, pinned)
        ctx.submit_resident(slot, mode, off, qb, **args)
        r = ctx.wait_resident(slot)
        host = np.concatenate(arenas)
        assert len(r[4]) > 0
        ctx.apply_fixes(host, r[4], r[5])
        assert_profile(out, profile_of(ctx, host, off, 3), "resident mode %d slot %d" % (mode, slot))
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
        outs.append(out_array(ctx, s, len(off) - 1, 1 + s % 2, pinned=s < 2))
        ctx.submit(s, f["mode"], *args)
    for s in (3, 1, 0, 2):
        ctx.wait(s)
    for s, (args, off) in enumerate(keep):
        assert_profile(outs[s], profile_of(ctx, np.concatenate(args[0::3]), off, 1 + s % 2), "slot %d, lanes %s" % (s, lanes))
    ctx.sync()
    ctx.close()


def test_a_batch_resubmitted_after_nospace_registers_again():
    f = fixture("fx_pe_k23")
    ctx = fixture_ctx(f)
    n = len(f["seqs1"])
    a, qa, off, _, _ = packed(rcorrector_amd, f, 0, n)
    arena, bases, exc_pos, exc_chr, qb = packed_inputs(ctx, a, qa, f["bad_q"])
    L, h = rcorrector_amd.load_library(), ctx._h
    out = out_array(ctx, 1, 2 * n, 1, pinned=False)
    ctx.submit_packed(1, f["mode"], a.size, off, bases, qb, exc_pos, exc_chr, fix_pos=np.zeros(0, np.uint32), fix_chr=np.zeros(0, np.uint8))   # fix_cap = 0
    assert L.rc_wait_packed(h, 1) == RC_STATUS_NOSPACE
    ctx._inflight_packed.pop(1)
    assert (out == -9).all()                      # (a pageable array is written by the wait that succeeds, and only by it)
    # the registration went with that submit: without a new one the resubmitted batch leaves the array alone
    ctx.submit_packed(1, f["mode"], a.size, off, bases, qb, exc_pos, exc_chr)
    res_plain = ctx.wait_packed(1)
    assert (out == -9).all()
    out = out_array(ctx, 1, 2 * n, 1, pinned=False)
    ctx.submit_packed(1, f["mode"], a.size, off, bases, qb, exc_pos, exc_chr)
    res = ctx.wait_packed(1)
    for x, y in zip(res_plain[:4], res[:4]):
        assert np.array_equal(x, y)
    assert len(res[4]) > 0 and sorted(res[4].tolist()) == sorted(res_plain[4].tolist())
    host = a.copy()
    ctx.apply_fixes(host, res[4], res[5])
    assert_profile(out, profile_of(ctx, host, off, 1), "resubmitted")
    ctx.sync()
    ctx.close()


def test_a_registration_changes_nothing_else_and_is_one_shot():
    f = fixture("fx_pe_k23")
    n = len(f["seqs1"])

    def run(register):
        ctx = fixture_ctx(f)
        digest = ctx.table_digest()
        outs = []
        for slot in (0, 2):
            a, qa, off, _, args = packed(rcorrector_amd, f, 0, n)
            out = out_array(ctx, slot, 2 * n, 1, pinned=slot == 0) if register else None
            ctx.submit(slot, f["mode"], *args)
            res = ctx.wait(slot)
            outs.append((out, [r.copy() for r in res], args[0].copy(), args[3].copy()))
        if register:
            # a second submit into slot 0 without a registration: the earlier array stays as the first batch left it
            first = outs[0][0].copy()
            assert (first != -9).all()
            a, qa, off, _, args = packed(rcorrector_amd, f, 0, n // 2)
            ctx.submit(0, f["mode"], *args)
            ctx.wait(0)
            assert np.array_equal(outs[0][0], first)
            withdrawn = out_array(ctx, 0, 2 * n, 1, pinned=True)
            ctx.weak_profile_withdraw(0)            # out == NULL withdraws
            a, qa, off, _, args = packed(rcorrector_amd, f, 0, n // 2)
            ctx.correct_batch(f["mode"], *args)
            assert np.array_equal(outs[0][0], first) and (withdrawn == -9).all()
        else:
            for _ in range(2):
                a, qa, off, _, args = packed(rcorrector_amd, f, 0, n // 2)
                ctx.correct_batch(f["mode"], *args)
        state = (ctx.summary(), ctx.table_digest() == digest)
        ctx.sync()
        ctx.close()
        return outs, state

    with_reg, st1 = run(True)
    without, st0 = run(False)
    assert st1 == st0 and st1[1]
    for (out, res, s1, s2), (_, res0, s10, s20) in zip(with_reg, without):
        assert all(np.array_equal(x, y) for x, y in zip(res, res0)) and np.array_equal(s1, s10) and np.array_equal(s2, s20)


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors():
    import torch
    f = fixture("fx_k15")
    L = rcorrector_amd.load_library()
    arena, off = rcorrector_amd.pack_reads(f["seqs1"][:8])
    t_seq, t_off = torch.from_numpy(arena).cuda(), torch.from_numpy(off.astype(np.int32)).cuda()
    t_out = torch.zeros((8, 4), dtype=torch.int32, device="cuda")
    host = np.zeros((8, 4), dtype=np.int32)
    torch.cuda.synchronize()
    dev = lambda c, mc, seq=t_seq.data_ptr(): L.rc_weak_profile_device(c._h, seq, t_off.data_ptr(), 8, arena.size, 100, mc, t_out.data_ptr())   # noqa: E731
    bare = rcorrector_amd.Context(k=f["k"], device=0)
    assert dev(bare, 1) == RC_STATUS_STATE                                    # no table
    assert L.rc_weak_profile_into(bare._h, 0, host.ctypes.data, 1) == RC_STATUS_STATE
    assert b"table" in L.rc_last_error(bare._h)
    bare.close()
    ctx = fixture_ctx(f)
    assert dev(ctx, 0) == RC_STATUS_ARG and dev(ctx, -3) == RC_STATUS_ARG     # min_count < 1
    assert dev(ctx, 1, None) == RC_STATUS_ARG                                 # a null pointer with reads
    assert L.rc_weak_profile_device(ctx._h, None, None, 0, 0, 0, 1, None) == 0
    assert L.rc_weak_profile_into(ctx._h, 0, host.ctypes.data, 0) == RC_STATUS_ARG
    assert L.rc_weak_profile_into(ctx._h, 4, host.ctypes.data, 1) == RC_STATUS_ARG   # slots are 0 .. 3
    assert L.rc_weak_profile_into(ctx._h, -1, host.ctypes.data, 1) == RC_STATUS_ARG
    assert dev(ctx, 1) == 0
    ctx.sync()
    assert_profile(t_out.cpu().numpy(), restate_all(f["seqs1"][:8], f["k"], f["counts_of"], 1))
    ctx.close()
