"""GPU: the recurrent-correction census (include/rcorrector_amd.h: rc_recur_census; kernels in rc_recur.hip).  The yardstick is
never the library: it is tests/recur_model.py, a pure-Python model over the strings that went in and the strings that came
out.  All comparisons are exact integer equality.
  1. rc_change_keys_device against the model on fabricated arena pairs (no table: "after" can be anything)
  2. the census through every entry point on the data set of tests/recur_data.py, modes 0, 1 and 2
  3. the session rules   4. inertness   5. report, overlap session and census armed together   6. the top list's order"""
import collections

import numpy as np
import pytest

import rcorrector_amd
import recur_data
import recur_model as rm
from test_duplicates import TRANSPORTS, reads_of
from test_recount import packed
from test_weak_profile import packed_inputs

pytestmark = pytest.mark.gpu

RC_STATUS_ARG, RC_STATUS_STATE, RC_STATUS_NOSPACE = -1, -4, -6
MAX_BIN = 6          # (the data set has sites corrected more often: the last bin is used)


# ---- 1. the kernel's keys against the model ------------------------------------------------------------------------------------
def fabricated_pairs():
    """(before, after) strings: every length 0..70 and 255, 256, 257, 1023; changes at p = 0, 13, 14, L - 15, L - 14, L - 1; in
    each of the sixteen byte positions of a granule; adjacent changes; every base changed; N / lower case in the window and as
    the original byte"""
    rng = np.random.default_rng(20261019)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    other = {65: 67, 67: 71, 71: 84, 84: 65}

    def flip(b, p, to=None):
        b[p] = other.get(int(b[p]), 65) if to is None else to

    pairs = []
    for L in list(range(71)) + [255, 256, 257, 1023]:
        a = rng.choice(letters, size=L)
        b = a.copy()
        for p in {0, 13, 14, L - 15, L - 14, L - 1}:
            if 0 <= p < L:
                flip(b, p)
        pairs.append((b, a))
    a = rng.choice(letters, size=90)
    for p in range(30, 46):                      # (sixteen consecutive positions: whatever the read's alignment, every byte of a granule)
        b = a.copy()
        flip(b, p)
        pairs.append((b, a))
    b = a.copy()
    for p in (40, 41, 42, 60, 61):
        flip(b, p)
    pairs.append((b, a))
    for L in (29, 64, 150, 300):
        a = rng.choice(letters, size=L)
        pairs.append((np.array([other[int(c)] for c in a], dtype=np.uint8), a))       # every base changed
    for _ in range(20):                              # more keys in one workgroup's sixteen reads than it stages: 20 x 372
        a = rng.choice(letters, size=400)
        pairs.append((np.array([other[int(c)] for c in a], dtype=np.uint8), a))
    for bad in b"Nnacgt":
        a = rng.choice(letters, size=80)
        b = a.copy()
        for p in (20, 40, 60):
            flip(b, p)
        a2 = a.copy()
        a2[45] = bad                                 # in the corrected read: clips the changes at 40 and 60 (not the one at 20)
        b2 = b.copy()
        b2[45] = bad
        pairs.append((b2, a2))
        b3 = a.copy()
        b3[40] = bad                                 # as the original byte: from = 4 (a lower-case letter of the same base too)
        pairs.append((b3, a))
    pairs.append((np.zeros(0, np.uint8), np.zeros(0, np.uint8)))
    return [(bytes(b), bytes(a)) for b, a in pairs]


def device_change_keys(ctx, pairs, lead=0, cap=None):
    """rc_change_keys_device on two arenas that start `lead` bytes behind a 16-byte boundary of device memory, with letters, not
    NULs, in front of and behind them.  Returns (sorted keys, counts[3], the guard words behind d_keys[cap])."""
    import torch
    before, off = rcorrector_amd.pack_reads([b for b, _ in pairs])
    after, off2 = rcorrector_amd.pack_reads([a for _, a in pairs])
    assert np.array_equal(off, off2)
    n = len(pairs)
    bufs = []
    for arena, fill in ((before, "C"), (after, "G")):
        buf = torch.full((lead + arena.size + 64,), ord(fill), dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        if arena.size:
            buf[lead:lead + arena.size] = torch.from_numpy(arena).cuda()
        bufs.append(buf)
    t_off = torch.from_numpy(off.astype(np.int32)).cuda()
    room = int(before.size) + 8 if cap is None else cap
    keys = torch.full((room + 4,), -7, dtype=torch.int64, device="cuda")
    counts = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.change_keys_device(bufs[0].data_ptr() + lead, bufs[1].data_ptr() + lead, t_off, n, before.size, keys, room, counts)
    ctx.sync()
    c = [int(x) for x in counts.cpu().numpy()]
    k = keys.cpu().numpy()
    return sorted(int(x) for x in k[:min(c[2], room)].view(np.uint64)), c, k[room:].tolist()


@pytest.fixture(scope="module")
def fabricated():
    pairs = fabricated_pairs()
    return pairs, rm.Census().add([b for b, _ in pairs], [a for _, a in pairs])


def test_change_keys_device_equals_the_model(fabricated):
    pairs, want = fabricated
    assert want.contexted > 100 and want.changes - want.contexted > 100
    ctx = rcorrector_amd.Context(k=23, device=0)   # (needs neither a table nor an open census)
    for lead in range(16):
        keys, counts, guard = device_change_keys(ctx, pairs, lead)
        assert counts == [want.changes, want.contexted, want.contexted], (lead, counts)
        assert keys == want.key_list(), lead
        assert guard == [-7] * 4
    # reversed reads: the same multiset
    keys, counts, _ = device_change_keys(ctx, pairs[::-1], 5)
    assert keys == want.key_list() and counts[0] == want.changes
    # n_reads = 0, and an arena of one empty read
    assert device_change_keys(ctx, [], 0) == ([], [0, 0, 0], [-7] * 4)
    assert device_change_keys(ctx, [(b"", b"")], 7)[:2] == ([], [0, 0, 0])
    # cap smaller than the number of keys: the counts are exact, nothing is written behind d_keys[cap]
    for cap in (0, 1, want.contexted // 2, want.contexted - 1):
        keys, counts, guard = device_change_keys(ctx, pairs, 3, cap)
        assert counts == [want.changes, want.contexted, want.contexted] and guard == [-7] * 4
        assert len(keys) == cap and not (set(keys) - set(want.key_list()))
    ctx.sync()
    ctx.close()


def test_change_keys_device_over_more_reads_than_one_stride_of_the_grid():
    """70 000 reads: the persistent workgroups stride over them several times and hand their staged keys on between strides.
    The reads are 40 distinct (before, after) pairs, so the model keys each pair once and the expected multiset is its keys times
    the pair's multiplicity."""
    import torch
    rng = np.random.default_rng(7)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    other = {65: 67, 67: 71, 71: 84, 84: 65}
    distinct = []
    for i in range(40):
        a = rng.choice(letters, size=60)
        b = np.array([other[int(c)] for c in a], dtype=np.uint8) if i % 2 else a.copy()   # every base changed, or one
        if i % 2 == 0:
            b[int(rng.integers(0, 60))] = ord("N")
        distinct.append((bytes(b), bytes(a)))
    pick = rng.integers(0, 40, size=70000)
    mult = np.bincount(pick, minlength=40)
    want_keys, changes, contexted = [], 0, 0
    for (b, a), m in zip(distinct, mult.tolist()):
        ch = rm.read_changes(b, a)
        changes += m * len(ch)
        ks = [k for _, k in ch if k is not None]
        contexted += m * len(ks)
        want_keys += ks * m
    before, off = rcorrector_amd.pack_reads([distinct[i][0] for i in pick.tolist()])
    after, _ = rcorrector_amd.pack_reads([distinct[i][1] for i in pick.tolist()])
    ctx = rcorrector_amd.Context(k=23, device=0)
    t_b, t_a = torch.from_numpy(before).cuda(), torch.from_numpy(after).cuda()
    t_off = torch.from_numpy(off.astype(np.int32)).cuda()
    keys = torch.full((contexted + 4,), -7, dtype=torch.int64, device="cuda")
    counts = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.change_keys_device(t_b, t_a, t_off, len(pick), before.size, keys, contexted, counts)
    ctx.sync()
    assert counts.cpu().numpy().tolist() == [changes, contexted, contexted] and contexted > 1000000
    k = keys.cpu().numpy()
    assert k[contexted:].tolist() == [-7] * 4
    assert np.array_equal(np.sort(k[:contexted].view(np.uint64)), np.sort(np.array(want_keys, dtype=np.uint64)))
    ctx.sync()
    ctx.close()


def test_change_keys_device_refuses_bad_arguments():
    import torch
    ctx = rcorrector_amd.Context(k=23, device=0)
    L, h = rcorrector_amd.load_library(), ctx._h
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
    off = torch.zeros(2, dtype=torch.int32, device="cuda")
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    p, o, k = buf.data_ptr(), off.data_ptr(), out.data_ptr()
    assert L.rc_change_keys_device(h, None, p, o, 1, 16, k, 4, k + 32) == RC_STATUS_ARG
    assert L.rc_change_keys_device(h, p, p, None, 1, 16, k, 4, k + 32) == RC_STATUS_ARG
    assert L.rc_change_keys_device(h, p, p, o, 1, 16, None, 4, k + 32) == RC_STATUS_ARG
    assert L.rc_change_keys_device(h, p, p, o, 1, 16, k, 4, None) == RC_STATUS_ARG
    assert L.rc_change_keys_device(h, p, p, o, 1, 16, k + 4, 2, k + 32) == RC_STATUS_ARG        # d_keys not aligned
    assert L.rc_change_keys_device(h, p, p + 8, o, 1, 16, k, 4, k + 32) == RC_STATUS_ARG       # arenas of different alignment
    assert L.rc_change_keys_device(h, p, p, o, 1, 1 << 32, k, 4, k + 32) == RC_STATUS_ARG      # 4 GiB
    ctx.sync()
    ctx.close()


# ---- 2. the census through every entry point -----------------------------------------------------------------------------------
_sets = {}


def data_ctx(mode):
    """the data set of a mode and ONE context for all its entry points: the table is counted from the set itself, and the counter
    keeps the arenas (what the resident transport corrects)"""
    if mode not in _sets:
        d = recur_data.make(mode)
        d["bad_q"] = b"H"
        if d["mode"] != 1:
            d["seqs2"], d["quals2"] = [], []
        ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
        ctx.count_keep(True)
        ctx.count_begin()
        d["a1"], d["off1"] = rcorrector_amd.pack_reads(d["seqs1"])
        ctx.count_add(d["a1"])
        if mode == 1:
            d["a2"], d["off2"] = rcorrector_amd.pack_reads(d["seqs2"])
            ctx.count_add(d["a2"])
        ctx.count_finish(2)
        ctx.set_run_params(d["rate"], d["bad_q"])
        _sets[mode] = (d, ctx)
    return _sets[mode]


@pytest.fixture(scope="module", autouse=True)
def _close_sets():
    yield
    for _, ctx in _sets.values():
        ctx.sync()
        ctx.close()
    _sets.clear()


def model_of(d, c1, c2):
    """the model's census of data set d and the reads that came back (mates 1, mates 2)"""
    return rm.Census().add(recur_data.all_reads(d), list(c1) + list(c2))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("transport", sorted(TRANSPORTS))
def test_census_through_every_entry_point(transport, mode):
    d, ctx = data_ctx(mode)
    via, lanes = TRANSPORTS[transport]
    ctx.set_slot_lanes(lanes)
    for nb in (1, 5):
        ctx.recur_census_begin()
        ctx.change_report_begin()
        c1, c2 = via(ctx, d, nb)
        got = ctx.recur_census(MAX_BIN, 2, 50)
        rep = ctx.change_report()
        ctx.change_report_end()
        ctx.recur_census_end()
        want = model_of(d, c1, c2)
        # (what makes the comparison mean something: recurring sites, singletons, clipped changes, the last bin in use)
        assert want.contexted > 500 and want.changes > want.contexted and max(want.keys.values()) >= 8
        rm.assert_result(got, want.result(MAX_BIN, 2, 50))
        assert got["recur"][MAX_BIN] >= 1 and got["recur"][1] >= 20
        assert got["changes"] == int(rep["changes"][0]) + int(rep["changes"][1])
    ctx.set_slot_lanes(True)


def test_a_batch_resubmitted_after_nospace_counts_once():
    d, ctx = data_ctx(1)
    n = len(d["seqs1"])
    a, qa, off, _, _ = packed(rcorrector_amd, d, 0, n)
    arena, bases, exc_pos, exc_chr, qb = packed_inputs(ctx, a, qa, d["bad_q"])
    L, h = rcorrector_amd.load_library(), ctx._h
    ctx.recur_census_begin()
    ctx.submit_packed(1, d["mode"], a.size, off, bases, qb, exc_pos, exc_chr, fix_pos=np.zeros(0, np.uint32), fix_chr=np.zeros(0, np.uint8))   # fix_cap = 0
    assert L.rc_wait_packed(h, 1) == RC_STATUS_NOSPACE
    ctx._inflight_packed.pop(1)
    got = ctx.recur_census(MAX_BIN)
    assert got["changes"] == 0 and got["sites"] == 0                     # the batch that did not fit is in no census yet
    ctx.submit_packed(1, d["mode"], a.size, off, bases, qb, exc_pos, exc_chr)
    r = ctx.wait_packed(1)
    assert len(r[4]) > 0
    ctx.apply_fixes(arena, r[4], r[5])
    cor = reads_of(arena, off)
    rm.assert_result(ctx.recur_census(MAX_BIN, 2, 50), model_of(d, cor[:n], cor[n:]).result(MAX_BIN, 2, 50))
    ctx.recur_census_end()


# ---- 3. the session rules -----------------------------------------------------------------------------------------------------------
def halves(d):
    n = len(d["seqs1"])
    return [(0, n // 2), (n // 2, n)]


def run_batch(ctx, d, lo, hi):
    """reads [lo, hi) of a mode-0 set through rc_correct_batch; returns (in, out) strings"""
    a, _, off, _, args = packed(rcorrector_amd, d, lo, hi)
    ctx.correct_batch(d["mode"], *args)
    return d["seqs1"][lo:hi], reads_of(args[0], off)


def test_session_rules():
    d, ctx = data_ctx(0)
    L, h = rcorrector_amd.load_library(), ctx._h
    with pytest.raises(rcorrector_amd.RcorrectorError, match="rc_recur_census_begin"):
        ctx.recur_census(MAX_BIN)                                        # get without begin
    assert L.rc_recur_census_end(h) == RC_STATUS_STATE                   # end without begin
    (lo1, hi1), (lo2, hi2) = halves(d)
    ctx.recur_census_begin()
    assert L.rc_recur_census_begin(h) == RC_STATUS_STATE                 # begin twice
    assert b"open already" in L.rc_last_error(h)
    want = rm.Census()
    want.add(*run_batch(ctx, d, lo1, hi1))
    rm.assert_result(ctx.recur_census(MAX_BIN, 2, 50), want.result(MAX_BIN, 2, 50))
    rm.assert_result(ctx.recur_census(3, 1, 7), want.result(3, 1, 7))     # get twice, other bounds: the keys are kept
    want.add(*run_batch(ctx, d, lo2, hi2))                                # more batches in between
    rm.assert_result(ctx.recur_census(MAX_BIN, 2, 50), want.result(MAX_BIN, 2, 50))
    # bad arguments
    import ctypes as C
    from rcorrector_amd.binding import _RecurCensus
    arr = np.zeros(16, dtype=np.uint64)
    ok = _RecurCensus(0, 0, 0, 0, 0, 0, arr.ctypes.data, arr.ctypes.data, arr.ctypes.data, 0)
    assert L.rc_recur_census_get(h, 0, 2, 4, C.byref(ok)) == RC_STATUS_ARG     # max_bin < 1
    assert L.rc_recur_census_get(h, 4, 0, 4, C.byref(ok)) == RC_STATUS_ARG     # min_count < 1
    assert L.rc_recur_census_get(h, 4, 2, 4, None) == RC_STATUS_ARG
    for bad in (_RecurCensus(0, 0, 0, 0, 0, 0, None, arr.ctypes.data, arr.ctypes.data, 0), _RecurCensus(0, 0, 0, 0, 0, 0, arr.ctypes.data, None, arr.ctypes.data, 0),
                _RecurCensus(0, 0, 0, 0, 0, 0, arr.ctypes.data, arr.ctypes.data, None, 0)):
        assert L.rc_recur_census_get(h, 4, 2, 4, C.byref(bad)) == RC_STATUS_ARG
    assert L.rc_recur_census_merge(h, h) == RC_STATUS_ARG                # merge into itself
    # a batch staged under a census that ends is in no census, and nothing of it reaches the next one
    a, _, off, _, args = packed(rcorrector_amd, d, lo1, hi1)
    ctx.submit(1, d["mode"], *args)
    ctx.recur_census_end()
    ctx.recur_census_begin()
    ctx.wait(1)
    got = ctx.recur_census(MAX_BIN)
    assert got["changes"] == 0 and got["sites"] == 0 and got["n_top"] == 0 and int(got["recur"].sum()) == 0
    want = rm.Census().add(*run_batch(ctx, d, lo2, hi2))                  # end then begin started from zero
    rm.assert_result(ctx.recur_census(MAX_BIN, 2, 50), want.result(MAX_BIN, 2, 50))
    ctx.recur_census_end()


def test_merge_of_two_contexts_equals_one_that_took_all():
    d, ctx = data_ctx(0)
    other = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    other.share_table_of(ctx)
    other.set_run_params(d["rate"], d["bad_q"])
    L = rcorrector_amd.load_library()
    (lo1, hi1), (lo2, hi2) = halves(d)
    ctx.recur_census_begin()
    assert L.rc_recur_census_merge(ctx._h, other._h) == RC_STATUS_STATE   # the source has none open
    other.recur_census_begin()
    want = rm.Census()
    want.add(*run_batch(ctx, d, lo1, hi1))
    want.add(*run_batch(other, d, lo2, hi2))
    ctx.recur_census_merge(other)
    rm.assert_result(ctx.recur_census(MAX_BIN, 2, 50), want.result(MAX_BIN, 2, 50))
    other.recur_census_end()
    ctx.recur_census_end()
    other.sync()
    other.close()


# ---- 4. inertness ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transport", ["correct_batch", "packed", "device"])
def test_a_census_changes_nothing_else(transport):
    d, ctx = data_ctx(1)
    via, _ = TRANSPORTS[transport]
    digest = ctx.table_digest()
    n = len(d["seqs1"])

    def once(census):
        s0 = ctx.summary()
        if census:
            ctx.recur_census_begin()
        out = via(ctx, d, 2)
        a, _, off, _, args = packed(rcorrector_amd, d, 0, n)
        res = ctx.correct_batch(d["mode"], *args)                         # ret / l / m / h and the arenas of one more batch
        if census:
            ctx.recur_census_end()
        s1 = ctx.summary()
        return out, [np.asarray(x).copy() for x in res], [np.asarray(x).copy() for x in args], (s1[0] - s0[0], s1[1] - s0[1])

    plain, with_census = once(False), once(True)
    assert plain[0] == with_census[0] and plain[3] == with_census[3]
    for x, y in zip(plain[1] + plain[2], with_census[1] + with_census[2]):
        assert np.array_equal(x, y)
    assert ctx.table_digest() == digest


# ---- 5. report, overlap session and census together: one shared snapshot ---------------------------------------------------------------
def flat(x):
    return {k: (np.asarray(v).tolist() if isinstance(v, np.ndarray) else v) for k, v in x.items()}


@pytest.mark.parametrize("transport", ["correct_batch", "slots_lanes_on", "packed"])
def test_report_overlap_and_census_together_equal_each_alone(transport):
    d, ctx = data_ctx(1)
    via, _ = TRANSPORTS[transport]

    def run(report, overlap, census):
        if report:
            ctx.change_report_begin()
        if overlap:
            ctx.mate_overlap_begin(20, 10)
        if census:
            ctx.recur_census_begin()
        c1, c2 = via(ctx, d, 3)
        out = {}
        if report:
            out["report"] = flat(ctx.change_report())
            ctx.change_report_end()
        if overlap:
            out["overlap"] = flat(ctx.mate_overlap())
            ctx.mate_overlap_end()
        if census:
            out["census"] = flat(ctx.recur_census(MAX_BIN, 2, 50))
            ctx.recur_census_end()
        return out, (c1, c2)

    together, reads = run(True, True, True)
    assert together["report"] == run(True, False, False)[0]["report"]
    assert together["overlap"] == run(False, True, False)[0]["overlap"]
    alone, reads2 = run(False, False, True)
    assert together["census"] == alone["census"] and reads == reads2
    rm.assert_result(together["census"], model_of(d, *reads).result(MAX_BIN, 2, 50))
    assert together["overlap"]["pairs"] == len(d["seqs1"])


# ---- 6. the top list's order -----------------------------------------------------------------------------------------------------------
def test_top_list_order_ties_and_truncation():
    """fabricated arenas through rc_change_keys_device cannot fill a census; a census is filled by batches.  So: reads whose
    every k-mer the table holds often except one planted substitution each, the same substitution planted in c reads for
    c = 4, 4, 4, 3, 3, 2, 2, 2, 1 ... -- ties in count, told apart by the key alone."""
    rng = np.random.default_rng(99)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    tx = rng.choice(letters, size=900)
    reads = []
    for i in range(800):                                  # the clean depth: 100 reads over every position
        s = int(rng.integers(0, 801))
        reads.append(tx[s:s + 100].tobytes())
    planted = [4, 4, 4, 3, 3, 2, 2, 2, 1, 1, 1]
    for j, c in enumerate(planted):
        p = 60 + 70 * j                                   # (sites far apart: no two in one read)
        alt = b"ACGT"[(b"ACGT".index(bytes(tx[p:p + 1])) + 1) % 4]
        for r in range(c):
            s = p - 30 - 7 * r                            # the site 30 .. 51 bases into the read: contexted
            b = bytearray(tx[s:s + 100].tobytes())
            b[p - s] = alt
            reads.append(bytes(b))
    d = dict(k=23, mfk=4, mode=0, seqs1=reads, quals1=[b"I" * 100] * len(reads), seqs2=[], quals2=[])
    ctx = rcorrector_amd.Context(k=23, max_fix_per_k=4, device=0)
    ctx.count_begin()
    ctx.count_add(rcorrector_amd.pack_reads(reads)[0])
    ctx.count_finish(2)
    ctx.set_run_params(0.01, b"H")
    ctx.recur_census_begin()
    want = rm.Census().add(*run_batch(ctx, d, 0, len(reads)))
    ties = collections.Counter(want.keys.values())
    assert all(ties[c] >= 2 for c in (4, 3, 2, 1))         # (planted ties were corrected: at least two sites at each count)
    for min_count, max_sites in [(1, 100), (2, 100), (2, 7), (2, 5), (2, 3), (2, 1), (3, 3), (4, 1), (5, 10), (1, 0)]:
        got = ctx.recur_census(10, min_count, max_sites)
        rm.assert_result(got, want.result(10, min_count, max_sites))
        top = list(zip(got["top_count"].tolist(), got["top_key"].tolist()))
        assert top == sorted(top, key=lambda t: (-t[0], t[1]))
    ctx.recur_census_end()
    ctx.sync()
    ctx.close()
