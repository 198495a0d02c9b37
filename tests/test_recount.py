"""GPU: the recount session -- rc_recount_begin / add / add_device / follow / finish and the binding's recount_* methods:
the k-mer spectrum of reads AFTER correction and the census of their k-mers that the table does not hold.

Expected values come from a numpy model in this file: the canonical codes of every valid window of an arena (a window
holding a letter outside ACGT or a NUL is skipped) -> np.unique(return_counts=True); table membership from
Context.table_export().  The corrected reads the model runs on are the ORACLE's (datasets.run_oracle), never the GPU's.
Every comparison is exact integer equality.
"""
import numpy as np
import pytest

import datasets
import rcorrector_amd

pytestmark = pytest.mark.gpu
MAX_BIN = 10000
DATASETS = ["pe_k23", "il_k23", "k15", "k32", "k31_mc8", "nrich", "varlen", "pe_var", "edge"]   # edge: the adversarial reads
_CODE = np.full(256, 4, dtype=np.uint64)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def canonical_codes(arena, k):
    """the canonical code of every window of k letters ACGT in a NUL-separated arena"""
    b = _CODE[np.frombuffer(bytes(arena), dtype=np.uint8)]
    n = len(b) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64)
    bad = np.zeros(n, dtype=bool)
    fw = np.zeros(n, dtype=np.uint64)
    rv = np.zeros(n, dtype=np.uint64)
    for j in range(k):
        w = b[j:j + n]
        bad |= w == 4
        fw = (fw << np.uint64(2)) | (w & np.uint64(3))
        rv |= (np.uint64(3) - (w & np.uint64(3))) << np.uint64(2 * j)
    return np.minimum(fw, rv)[~bad]


def model(arenas, k, table_codes, max_bin=MAX_BIN):
    codes = np.concatenate([canonical_codes(a, k) for a in arenas] + [np.zeros(0, dtype=np.uint64)])
    u, c = np.unique(codes, return_counts=True)
    f = np.bincount(np.minimum(c, max_bin), minlength=max_bin + 1).astype(np.uint64)
    f[0] = 0
    absent = ~np.isin(u, np.asarray(table_codes, dtype=np.uint64))
    st = {"distinct": len(u), "total": int(c.sum()), "unique": int((c == 1).sum()), "max_count": int(c.max()) if len(c) else 0,
          "absent_distinct": int(absent.sum()), "absent_total": int(c[absent].sum())}
    return f, st


def assert_recount(got, want, what=""):
    assert got[0].dtype == np.uint64 and len(got[0]) == len(want[0])
    assert np.array_equal(got[0], want[0]), "%s: bins differ at %s" % (what, np.nonzero(got[0] != want[0])[0][:10])
    assert got[1] == want[1], what


def table_ctx(d):
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    ctx.table_build(d["keys"], d["counts"])
    ctx.set_run_params(d["rate"], b"H")
    return ctx


def unit_cuts(d, nb):
    """read index ranges of nb batches (mates travel together)"""
    step = 2 if d["mode"] == 2 else 1
    units = len(d["seqs1"]) // step
    c = (np.linspace(0, units, nb + 1).astype(np.int64) * step).tolist()
    return list(zip(c[:-1], c[1:]))


def packed(po, d, lo, hi):
    """(arena, qualities, offsets over the whole arena, bytes of the first arena) of reads [lo, hi) -- mode 1: both mates' arenas"""
    a, off = po.pack_reads(d["seqs1"][lo:hi])
    qa, _ = po.pack_reads(d["quals1"][lo:hi])
    if d["mode"] != 1:
        return a, qa, off, a.size, (a, qa, off)
    a2, off2 = po.pack_reads(d["seqs2"][lo:hi])
    qa2, _ = po.pack_reads(d["quals2"][lo:hi])
    both = np.concatenate([off, (off2[1:].astype(np.int64) + a.size).astype(np.uint32)])
    return np.concatenate([a, a2]), np.concatenate([qa, qa2]), both, a.size, (a, qa, off, a2, qa2, off2)


# ---- the five transports: each corrects d in nb batches with a session open and returns recount_finish() ----------------
def via_correct_batch(po, ctx, d, nb):
    ctx.recount_begin(MAX_BIN)
    ctx.recount_follow(True)
    for lo, hi in unit_cuts(d, nb):
        if hi > lo:
            ctx.correct_batch(d["mode"], *packed(po, d, lo, hi)[4])
    return ctx.recount_finish()


def via_slots(po, ctx, d, nb):
    """rc_submit / rc_wait, two slots in flight (slot 1 runs in a lane of its own)"""
    ctx.recount_begin(MAX_BIN)
    ctx.recount_follow(True)
    busy = {}
    for i, (lo, hi) in enumerate(unit_cuts(d, nb)):
        s = i % 2
        if s in busy:
            ctx.wait(s)
        busy[s] = packed(po, d, lo, hi)[4]
        ctx.submit(s, d["mode"], *busy[s])
    for s in sorted(busy, reverse=True):
        ctx.wait(s)
    return ctx.recount_finish()


def via_packed(po, ctx, d, nb):
    ctx.recount_begin(MAX_BIN)
    ctx.recount_follow(True)
    busy = {}
    for i, (lo, hi) in enumerate(unit_cuts(d, nb)):
        s = i % 2
        if s in busy:
            ctx.wait_packed(s)
        a, qa, off, _, _ = packed(po, d, lo, hi)
        arena = ctx.host_array(a.size)
        arena[:] = a
        bases, exc_pos, exc_chr = ctx.pack_bases(arena, bases=ctx.host_array((a.size + 15) // 16, np.uint32))
        qb = ctx.host_array((a.size + 7) // 8)
        ctx.pack_quality_bits(qa, b"H", out=qb)
        busy[s] = (arena, bases, exc_pos, exc_chr, qb, off)
        ctx.submit_packed(s, d["mode"], a.size, off, bases, qb, exc_pos, exc_chr)
    for s in sorted(busy):
        ctx.wait_packed(s)
    return ctx.recount_finish()


def via_resident(po, ctx, d, nb):
    """the reads are the arenas the counter kept; every batch a byte range of them"""
    a1, off1 = po.pack_reads(d["seqs1"])
    q1, _ = po.pack_reads(d["quals1"])
    ctx.count_keep(True)
    ctx.count_begin()
    ctx.count_add(a1)
    if d["mode"] == 1:
        a2, off2 = po.pack_reads(d["seqs2"])
        q2, _ = po.pack_reads(d["quals2"])
        ctx.count_add(a2)
    ctx.count_finish(2)
    ctx.table_build(d["keys"], d["counts"])
    ctx.set_run_params(d["rate"], b"H")
    ctx.recount_begin(MAX_BIN)
    ctx.recount_follow(True)
    keep = []
    for i, (lo, hi) in enumerate(unit_cuts(d, nb)):
        if hi == lo:
            continue
        b1 = int(off1[hi] - off1[lo])
        off = [off1[lo:hi + 1].astype(np.int64) - int(off1[lo])]
        qs = [q1[off1[lo]:off1[hi]]]
        args = dict(arena_a=0, begin_a=int(off1[lo]), bytes_a=b1)
        if d["mode"] == 1:
            off.append(off2[lo + 1:hi + 1].astype(np.int64) - int(off2[lo]) + b1)
            qs.append(q2[off2[lo]:off2[hi]])
            args.update(arena_b=1, begin_b=int(off2[lo]), bytes_b=int(off2[hi] - off2[lo]))
        nbytes = b1 + args.get("bytes_b", 0)
        qb = ctx.host_array((nbytes + 7) // 8)
        ctx.pack_quality_bits(np.concatenate(qs), b"H", out=qb)
        keep.append(qb)
        ctx.submit_resident(i % 2, d["mode"], np.concatenate(off).astype(np.uint32), qb, **args)
        ctx.wait_resident(i % 2)
    return ctx.recount_finish()


def via_device(po, ctx, d, nb):
    """rc_correct_device corrects the caller's memory in place; the caller hands it to recount_add_device"""
    import torch
    ctx.recount_begin(MAX_BIN)
    ctx.recount_follow(True)   # (nothing of this transport goes through a wait: only what is added by hand counts)
    for lo, hi in unit_cuts(d, nb):
        if hi == lo:
            continue
        a, qa, off, _, _ = packed(po, d, lo, hi)
        n = len(off) - 1
        t_seq = torch.from_numpy(a.copy()).cuda()
        t_q = torch.from_numpy(qa.copy()).cuda()
        t_off = torch.from_numpy(off.astype(np.int32)).cuda()
        res = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(4)]
        max_len = int(np.diff(off.astype(np.int64)).max()) - 1
        ctx.correct_device(d["mode"], n, a.size, max_len, t_seq, t_q, t_off, *res)
        ctx.sync()
        ctx.recount_add_device(t_seq, a.size)
    return ctx.recount_finish()


TRANSPORTS = {"correct_batch": via_correct_batch, "slots": via_slots, "packed": via_packed, "resident": via_resident, "device": via_device}


def counted_ctx(po, d, min_count, spectrum=True):
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    arenas = [po.pack_reads(d["seqs1"])[0]] + ([po.pack_reads(d["seqs2"])[0]] if d["seqs2"] else [])
    if spectrum:
        ctx.count_spectrum(MAX_BIN)
    ctx.count_begin()
    for a in arenas:
        ctx.count_add(a)
    ctx.count_finish(min_count)
    return ctx, arenas


# ---- 1. identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_count", [2, 3])
@pytest.mark.parametrize("name", ["pe_k23", "nrich", "k32", "edge"])
def test_recount_of_the_uncorrected_reads_is_the_counted_spectrum(oracle, name, min_count):
    d = datasets.make(name)
    ctx, arenas = counted_ctx(oracle, d, min_count)
    counted = ctx.kmer_spectrum("counted", MAX_BIN)
    ctx.recount_begin(MAX_BIN)
    for a in arenas:
        ctx.recount_add(a)
    freq, st = ctx.recount_finish()
    assert np.array_equal(freq, counted[0])
    assert {key: st[key] for key in counted[1]} == counted[1]
    assert st["absent_distinct"] == int(freq[1:min_count].sum())
    assert st["absent_total"] == int((freq[1:min_count] * np.arange(1, min_count, dtype=np.uint64)).sum())
    assert_recount((freq, st), model(arenas, d["k"], ctx.table_export()[0]), name)
    ctx.close()


# ---- 2. corrected reads, every transport, any split ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", DATASETS)
def test_recount_of_corrected_reads_equals_the_model_on_the_oracles_reads(oracle, name):
    d = datasets.make(name)
    corrected = datasets.run_oracle(oracle, d)[4:]
    assert any(np.any(c != o) for c, o in zip(corrected, [oracle.pack_reads(d["seqs1"])[0]] + ([oracle.pack_reads(d["seqs2"])[0]] if d["seqs2"] else [])))
    ctx = table_ctx(d)
    want = model(corrected, d["k"], ctx.table_export()[0])
    assert want[1]["absent_distinct"] > 0 and want[1]["distinct"] > want[1]["absent_distinct"]
    for tname, run in TRANSPORTS.items():
        for nb in (1, 3, 17):
            c = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0) if tname == "resident" else ctx
            assert_recount(run(oracle, c, d, nb), want, "%s through %s in %d batches" % (name, tname, nb))
            if c is not ctx:
                c.close()
    ctx.close()


# ---- 3. layouts, filter, passes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"RC_TABLE_LAYOUT": "wide"}, {}, {"RC_TABLE_FILTER": "force"}, {"RC_TABLE_FILTER": "force", "RC_TABLE_FILTER_KIND": "plain"},
                                 {"RC_COUNT_MEM_MB": "1"}], ids=["wide", "packed", "filter", "filter_plain", "passes"])
@pytest.mark.parametrize("name", ["pe_k23", "k31_mc8", "k15"])
def test_layouts_filter_and_passes_give_the_same_answer(oracle, name, env, monkeypatch):
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    d = datasets.make(name)
    corrected = datasets.run_oracle(oracle, d)[4:]
    ctx = table_ctx(d)
    if "RC_TABLE_LAYOUT" in env:
        assert ctx.table_layout() == 0
    want = model(corrected, d["k"], ctx.table_export()[0])
    if "RC_COUNT_MEM_MB" in env:   # 40 bytes * 1.15 per arena byte over 1 MB: at least four passes
        assert sum(c.size for c in corrected) * 46 >= 4 << 20
    assert_recount(via_correct_batch(oracle, ctx, d, 3), want, "%s %s" % (name, env))
    ctx.recount_begin(7)   # a small bound folds the bins, the statistics stay
    for c in corrected:
        ctx.recount_add(c)
    assert_recount(ctx.recount_finish(), model(corrected, d["k"], ctx.table_export()[0], 7), "%s %s max_bin 7" % (name, env))
    ctx.close()


# ---- 4. nothing disturbed ------------------------------------------------------------------------------------------------------
def test_a_session_disturbs_nothing(oracle):
    d = datasets.make("pe_k23")
    want_res = datasets.run_oracle(oracle, d)
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    a1, off1 = oracle.pack_reads(d["seqs1"])
    a2, off2 = oracle.pack_reads(d["seqs2"])
    q = np.concatenate([oracle.pack_reads(d["quals1"])[0], oracle.pack_reads(d["quals2"])[0]])
    ctx.count_keep(True)
    ctx.count_spectrum(MAX_BIN)
    ctx.count_begin()
    ctx.count_add(a1)
    ctx.count_add(a2)
    ctx.count_finish(2)
    ctx.set_run_params(d["rate"], b"H")
    off = np.concatenate([off1, (off2[1:].astype(np.int64) + a1.size).astype(np.uint32)])
    qb = ctx.host_array((a1.size + a2.size + 7) // 8)
    ctx.pack_quality_bits(q, b"H", out=qb)
    args = dict(arena_a=0, begin_a=0, bytes_a=a1.size, arena_b=1, begin_b=0, bytes_b=a2.size)

    def resident():
        ctx.submit_resident(0, 1, off, qb, **args)
        r = ctx.wait_resident(0)
        return [x.copy() for x in r[:4]] + [sorted(zip(r[4].tolist(), r[5].tolist()))]

    def state():
        c = ctx.kmer_spectrum("counted", MAX_BIN)
        return ctx.table_digest(), ctx.table_stats(), c[0].tolist(), c[1], list(ctx.count_arenas())

    before, first = state(), resident()
    # follow off (the default): the session sees only what is added by hand, whatever completes meanwhile
    ctx.recount_begin(MAX_BIN)
    second = resident()
    ctx.recount_add(a1)
    got = ctx.recount_finish()
    assert_recount(got, model([a1], d["k"], ctx.table_export()[0]), "follow off")
    assert state() == before
    # follow on: the resident batch is taken once per completion, the kept arenas stay as they were
    ctx.recount_begin(MAX_BIN)
    ctx.recount_follow(True)
    third = resident()
    assert state() == before          # (mid-session)
    got = ctx.recount_finish()
    host = np.concatenate([a1, a2])
    fp = np.array([p for p, _ in third[4]], dtype=np.uint32)
    fc = np.array([c for _, c in third[4]], dtype=np.uint8)
    ctx.apply_fixes(host, fp, fc)
    assert_recount(got, model([host], d["k"], ctx.table_export()[0]), "follow on")
    assert state() == before
    ctx.recount_follow(False)
    fourth = resident()
    for r in (second, third, fourth):
        for x, y in zip(first[:4], r[:4]):
            assert np.array_equal(x, y)
        assert r[4] == first[4]
    # a finished session is closed: follow on without one changes nothing and keeps nothing
    ctx.recount_follow(True)
    assert resident()[4] == first[4]
    with pytest.raises(rcorrector_amd.RcorrectorError):
        ctx.recount_finish()
    ctx.close()


# ---- 5. state and argument errors ------------------------------------------------------------------------------------------------
def status_of(call):
    with pytest.raises(rcorrector_amd.RcorrectorError) as e:
        call()
    return e.value


def test_state_and_argument_errors(oracle):
    RC_STATUS_ARG, RC_STATUS_STATE = -1, -4
    d = datasets.make("k15")
    a = oracle.pack_reads(d["seqs1"])[0]
    L = rcorrector_amd.load_library()
    ctx = rcorrector_amd.Context(k=d["k"], device=0)
    h = ctx._h
    freq = np.zeros(MAX_BIN + 1, dtype=np.uint64)
    # no table
    assert L.rc_recount_begin(h, 100) == RC_STATUS_STATE
    assert L.rc_recount_add(h, a.ctypes.data, a.size) == RC_STATUS_STATE
    assert L.rc_recount_finish(h, freq.ctypes.data, None) == RC_STATUS_STATE
    ctx.table_build(d["keys"], d["counts"])
    digest = ctx.table_digest()
    # add / finish without begin
    assert L.rc_recount_add(h, a.ctypes.data, a.size) == RC_STATUS_STATE
    assert L.rc_recount_add_device(h, a.ctypes.data, a.size) == RC_STATUS_STATE
    assert L.rc_recount_finish(h, freq.ctypes.data, None) == RC_STATUS_STATE
    # bad max_bin
    assert L.rc_recount_begin(h, 0) == RC_STATUS_ARG
    assert L.rc_recount_begin(h, (1 << 28) + 1) == RC_STATUS_ARG
    assert L.rc_recount_begin(h, 1 << 28) == 0
    # one session at a time, of either kind
    assert L.rc_recount_begin(h, 100) == RC_STATUS_STATE
    assert L.rc_table_count_begin(h) == RC_STATUS_STATE
    assert L.rc_recount_add(h, a.ctypes.data, a.size) == 0
    big = np.zeros((1 << 28) + 1, dtype=np.uint64)
    st = rcorrector_amd.binding._RecountStats()
    import ctypes as C
    assert L.rc_recount_finish(h, big.ctypes.data, C.byref(st)) == 0
    want = model([a], d["k"], ctx.table_export()[0], 1 << 28)
    assert np.array_equal(big, want[0]) and st.all.distinct == want[1]["distinct"] and st.absent_total == want[1]["absent_total"]
    assert L.rc_recount_finish(h, freq.ctypes.data, None) == RC_STATUS_STATE   # the session is over
    ctx.count_begin()
    assert L.rc_recount_begin(h, 100) == RC_STATUS_STATE                        # a counting session is open
    ctx.count_park()
    assert ctx.table_digest() == digest
    assert L.rc_recount_begin(h, 100) == 0
    assert L.rc_recount_finish(h, None, None) == RC_STATUS_ARG
    assert L.rc_recount_finish(h, freq.ctypes.data, None) == RC_STATUS_STATE   # an error ends the session
    assert ctx.table_digest() == digest
    ctx.close()


def test_a_context_destroyed_mid_session_leaves_nothing_behind(oracle):
    import torch
    d = datasets.make("k15")
    a = oracle.pack_reads(d["seqs1"])[0]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(8):
        ctx = table_ctx(d)
        ctx.recount_begin(MAX_BIN)
        ctx.recount_follow(True)
        ctx.recount_add(a)
        ctx.correct_batch(d["mode"], *packed(oracle, d, 0, len(d["seqs1"]))[4])
        ctx.close()
    torch.cuda.synchronize()
    # (a session's chunks are 2 GiB each: eight leaked sessions would be 16 GiB; other processes may share the device)
    assert free0 - torch.cuda.mem_get_info()[0] < (6 << 30)
    ctx = table_ctx(d)   # ... and the next context counts as if nothing had happened
    ctx.recount_begin(MAX_BIN)
    ctx.recount_add(a)
    assert_recount(ctx.recount_finish(), model([a], d["k"], ctx.table_export()[0]))
    ctx.close()
