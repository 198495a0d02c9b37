"""The chunked pipeline (RC_PIPELINE_CHUNKS=<C>; rc_api_batch.hip: rc_correct_pipelined) on every route a batch can take into
rc_correct_device_impl, and under every instance of the fused probe + threshold kernel -- tests/test_pipeline_chunks.py reaches
it through rc_correct_device alone, with quality bytes, on one context, with the default instance.

Every context here is made with RC_LOCALITY=force and RC_PIPELINE_CHUNKS set, and both stay set for the whole test: a slot
lane is a context of its own, made at its first use, and reads the environment then.  Every case is held three ways:
  * to the oracle (or, on the golden fixture, to the reference's corrected reads) -- exactly, integer work;
  * to the same route at RC_PIPELINE_CHUNKS=0;
  * through rc_debug_pipeline to the batches and non-empty chunks the case must have run as a pipeline -- or to (0, 0) where
    the code says the pipeline stands aside, with the reason stated.  Nothing skips where the pipeline does not run.

A read's results depend on its unit and the table alone (tests/test_quality_vetoes.py: test_batch_split_invariance), so the
oracle's results on a batch's first units are the first rows of its results on the whole batch: computed once, sliced here."""
import ctypes as C

import numpy as np
import pytest

import datasets
import rcorrector_amd
import test_observers_together as tot
import test_pipeline_chunks as tpc
import test_quality_vetoes as tqv
import test_stage_wide as tsw
from test_change_report import _Trace
from test_duplicates import TRANSPORTS
from test_gpu_parity import KNOBS
from test_pipeline_chunks import chunks_expected, reads_per_tile

pytestmark = pytest.mark.gpu

CHUNKS = 3


# ---- C1: the fused kernel's instances under a tile range ---------------------------------------------------------------------

def _knob(**want):
    """the member of test_gpu_parity.KNOBS that sets exactly `want` beside RC_LOCALITY (which every context here forces)"""
    hits = [kn for kn in KNOBS if {k: v for k, v in kn.items() if k != "RC_LOCALITY"} == want]
    assert hits, "test_gpu_parity.KNOBS has no member %r" % want
    return dict(want)


FUSED = {
    "xcd": {"RC_FUSED_XCD": "1"},
    "dedup": _knob(RC_FUSED_DEDUP="1"),
    "wave_tiles": _knob(RC_FUSED_WAVE_TILES="1"),
    "quad": _knob(RC_PROBE_QUAD="1"),
    "xcd_dedup": {"RC_FUSED_XCD": "1", "RC_FUSED_DEDUP": "1"},
    "wide": _knob(RC_TABLE_LAYOUT="wide"),
    "filter_plain": _knob(RC_TABLE_FILTER="force", RC_TABLE_FILTER_KIND="plain"),
    "filter_core": _knob(RC_TABLE_FILTER="force", RC_TABLE_FILTER_KIND="core"),
}
# None of these makes rc_fused_tiles (rc_correct.hip) say 0 -- it refuses a batch for a read beyond 160 bases, k < 4,
# RC_K2_WAVE_PER_READ and RC_NO_FUSE only -- so under every one of them the pipeline must RUN: (1, chunks), never (0, 0).

# A chunk of s tiles: tile_at(c) = T * c // C (rc_correct_pipelined) cuts T tiles into chunks of T // C or T // C + 1 tiles, so
# 1, 7 and 9 need a batch each.  wanted chunk size: (tiles T, chunks C) -> 7 * c // 7: seven chunks of 1;  23 * c // 3 = 0, 7,
# 15, 23: chunks of 7, 8, 8;  25 * c // 3 = 0, 8, 16, 25: chunks of 8, 8, 9.  (7 and 9 are no multiple of 8: under
# RC_FUSED_XCD=1 their grids of 8 and 16 workgroups hold one and seven that own no tile.)
SIZED = {1: (7, 7), 7: (23, 3), 9: (25, 3)}


def _chunk_sizes(tiles, chunks):
    return [tiles * (c + 1) // chunks - tiles * c // chunks for c in range(chunks)]


def _first_units(d, want, n):
    """the batch of d's first n reads (mode 1: n / 2 pairs) and the oracle's results on them, cut out of those on all of d"""
    from oracle import pyoracle as po
    units = n // 2 if d["mode"] == 1 else n
    total = len(d["seqs1"])
    assert 0 < units <= total and (d["mode"] != 1 or n % 2 == 0)
    sub = dict(d, seqs1=d["seqs1"][:units], quals1=d["quals1"][:units])
    rows = [np.arange(units)]
    bases = [want[4][:int(po.pack_reads(sub["seqs1"])[1][-1])]]
    if d["mode"] == 1:
        sub.update(seqs2=d["seqs2"][:units], quals2=d["quals2"][:units])
        rows.append(total + np.arange(units))
        bases.append(want[5][:int(po.pack_reads(sub["seqs2"])[1][-1])])
    rows = np.concatenate(rows)
    return sub, [w[rows] for w in want[:4]] + [np.concatenate(bases)]


def _run_device(ctx, d):
    arrays = tsw._device_arrays(d)
    res, work = tpc._launch(ctx, d, arrays)
    ctx.sync()
    return tpc._fetch(res, work), tpc._routes(ctx, arrays[1], False), arrays[1], arrays[2]


def _fused_case(monkeypatch, d, want, env, rpt, label, sized=True):
    """d whole at C = 3 and its first reads in chunks of 1, 7 and 9 tiles, the last tile a partial one each time: results
    against the oracle and the unchunked context, routes against the unchunked context's, the counters after every batch"""
    n_all = (2 if d["mode"] == 1 else 1) * len(d["seqs1"])
    plan = [(n_all, CHUNKS, None)]
    for size, (tiles, chunks) in sorted(SIZED.items()) if sized else []:
        n = (tiles - 1) * rpt + rpt // 2        # tiles - 1 full tiles and half a tile; even, so pairs stay whole
        assert n <= n_all and (n + rpt - 1) // rpt == tiles and n % rpt != 0
        assert size in _chunk_sizes(tiles, chunks) and sum(_chunk_sizes(tiles, chunks)) == tiles
        plan.append((n, chunks, size))
    ctxs, ran = {}, {}
    for n, chunks, size in plan:
        sub, want_sub = _first_units(d, want, n)
        for c in (0, chunks):
            if c not in ctxs:
                ctxs[c], ran[c] = tpc._context(monkeypatch, d, env, c), [0, 0]
        got0, routes0, n0, max_len = _run_device(ctxs[0], sub)
        got, routes, n1, _ = _run_device(ctxs[chunks], sub)
        what = "%s, %d reads in %d chunks" % (label, n, chunks)
        assert n0 == n1 == n and reads_per_tile(max_len, rpt == 4) == rpt
        tpc._equal(want_sub, got, what + ", against the oracle")
        tpc._equal(got0, got, what + ", against no chunks")
        for a, b, name in zip(routes0, routes, ["cls", "cand", "runs"]):
            assert np.array_equal(a, b), "%s: the routes' %s differ from those without chunks" % (what, name)
        ran[chunks][0] += 1
        ran[chunks][1] += chunks_expected(n, rpt, chunks)
        if size is not None:
            assert chunks_expected(n, rpt, chunks) == chunks, "every chunk of a sized case holds tiles"
        assert ctxs[chunks].debug_pipeline() == tuple(ran[chunks]), "%s: (batches, chunks) run as a pipeline: %r, expected %r" % (
            what, ctxs[chunks].debug_pipeline(), tuple(ran[chunks]))
        assert ctxs[0].debug_pipeline() == (0, 0)
    return ctxs


@pytest.mark.parametrize("name", ["pe150", "k31", "two"])
@pytest.mark.parametrize("knobs", sorted(FUSED))
def test_fused_kernel_variants_in_chunks(oracle, monkeypatch, knobs, name):
    d, want = tpc._case(name)
    env = FUSED[knobs]
    # the wave-tile instance (4 reads a tile) is taken for reads of at most 128 k-mers over a table without extension bits
    # (rc_fused_tiles): pe150 and two (k = 23: 128 k-mers, PACKED without them); k31's table has them unless the layout is WIDE
    ext = name == "k31" and env.get("RC_TABLE_LAYOUT") != "wide"
    rpt = reads_per_tile(150, "RC_FUSED_WAVE_TILES" in env and not ext)
    # two: 2 reads are one tile, hence one chunk whatever C is -- chunks of 7 or 9 tiles do not exist there
    ctxs = _fused_case(monkeypatch, d, want, env, rpt, "%s under %s" % (name, env), sized=name != "two")
    for ctx in ctxs.values():
        if name == "k31":
            assert d["mfk"] == 8 and (ctx.table_layout() == 1 and ctx.table_stats()["buckets"] < 1 << (2 * d["k"] - 32)) == ext
        if name == "pe150":
            assert ctx.table_layout() == (0 if "RC_TABLE_LAYOUT" in env else 1)
        ctx.close()


def test_packed_table_with_extension_bits_in_chunks(oracle, monkeypatch):
    """k = 26 over a PACKED table padded to 120 000 entries (tests/test_k_sweep.py: ext = 4), 600 pairs of 100 bases: the
    4 096-byte tile's instance with extension bits, 32 reads a tile"""
    import test_k_sweep as tks
    d, want = tks._case(26, 1, 120_000)
    assert max(len(r) for r in d["seqs1"] + d["seqs2"]) == 100
    ctxs = _fused_case(monkeypatch, d, want, {}, reads_per_tile(100), "k = 26 with extension bits")
    for ctx in ctxs.values():
        layout, ext = tks._check_layout(ctx, d)
        assert layout == 1 and ext > 0 and ctx.table_stats()["buckets"] < 1 << (2 * 26 - 32)
        ctx.close()


# ---- C2 / C3: every transport, and the observers, behind a chunked batch -------------------------------------------------------

_runs = {}


def _transport_run(monkeypatch, transport, armed, chunks, nospace=False):
    """test_observers_together.run (64 pairs of fx_pe_k23 in three batches through slots 0, 1 and 2) with the pipeline at
    `chunks`; what the context says of itself just before run() closes it is kept beside run()'s results.  Runs without chunks
    are made once and shared."""
    key = (transport, armed, chunks, nospace)
    if chunks == 0 and key in _runs:
        return _runs[key]
    monkeypatch.setenv("RC_LOCALITY", "force")
    monkeypatch.setenv("RC_PIPELINE_CHUNKS", str(chunks))
    seen = []
    close = rcorrector_amd.Context.close

    def closing(self):
        seen.append((self.debug_pipeline(), self.summary()))
        close(self)
    monkeypatch.setattr(rcorrector_amd.Context, "close", closing)
    out = tot.run(transport, armed, nospace=nospace)
    monkeypatch.setattr(rcorrector_amd.Context, "close", close)
    assert len(seen) == 1
    _runs[key] = (out, seen[0][0], seen[0][1])
    return _runs[key]


def _fixture_batches():
    """per batch of the run: (reads, the reference's corrected arena, substitutions)"""
    d = tot.dataset()
    assert max(len(r) for r in d["seqs1"] + d["seqs2"]) <= 160, "a longer read would make the batch a tiered one"
    f = tot.fixture("fx_pe_k23")
    out = []
    for lo, hi in tot.unit_cuts(d, tot.BATCHES):
        before = tot.packed(rcorrector_amd, d, lo, hi)[0]
        after = np.concatenate([rcorrector_amd.pack_reads(f["cor1"][lo:hi])[0], rcorrector_amd.pack_reads(f["cor2"][lo:hi])[0]])
        assert before.shape == after.shape
        out.append((2 * (hi - lo), after, int((before != after).sum())))
    return out


@pytest.mark.parametrize("chunks", [2, 3])
@pytest.mark.parametrize("transport", sorted(TRANSPORTS))
def test_every_transport_behind_a_chunked_batch(monkeypatch, transport, chunks):
    """what a transport queues behind the batch on the context's stream -- copies back, fix-list kernels -- sees a joined batch"""
    fx = _fixture_batches()
    plain, ran0, summary0 = _transport_run(monkeypatch, transport, (), 0)
    got, ran, summary = _transport_run(monkeypatch, transport, (), chunks)
    tot.assert_same(got["batches"], plain["batches"], "%s in %d chunks against no chunks" % (transport, chunks))
    for i, ((n, after, subst), b) in enumerate(zip(fx, got["batches"])):
        assert len(b[1]) == n and np.array_equal(b[0], after), "%s in %d chunks: batch %d is not the reference's corrected reads" % (transport, chunks, i)
        assert int(b[1][b[1] > 0].sum()) == subst
    # 150-base reads: 16 a tile; batches of 42, 42 and 44 reads are three tiles each
    assert ran0 == (0, 0)
    assert ran == (3, sum(chunks_expected(n, reads_per_tile(150), chunks) for n, _, _ in fx)), "lanes included"
    assert summary == summary0 == (sum(n for n, _, _ in fx), sum(s for _, _, s in fx))
    assert summary[1] > 0


@pytest.mark.parametrize("transport,nospace", [("device", False), ("packed", False), ("resident", False), ("slots_lanes_on", False), ("packed", True)])
def test_observers_behind_a_chunked_batch(monkeypatch, transport, nospace):
    """the observers' "after" work is queued on the context's stream behind the batch: field by field what they see without chunks"""
    plain, ran0, summary0 = _transport_run(monkeypatch, transport, tot.OBSERVERS, 0, nospace)
    got, ran, summary = _transport_run(monkeypatch, transport, tot.OBSERVERS, CHUNKS, nospace)
    tot.assert_same(got, plain, "%s with every observer armed, %d chunks against none" % (transport, CHUNKS))
    assert int(got["report"]["reads"].sum()) == 2 * tot.PAIRS and got["census"]["units"] == tot.PAIRS   # the middle batch once
    # nospace: the middle batch's first submission (room for one substitution) runs the correction too -- the fix list overflows
    # behind it, at the wait -- so the correction kernels see four batches where the observers see three
    assert ran0 == (0, 0) and ran == ((4, 12) if nospace else (3, 9))
    assert summary == summary0


# ---- C4: quality bytes, quality bits, the split quality arena ----------------------------------------------------------------

QV = ["qv_mixed_pe/straddle", "qv_dense_mfk2/straddle"]


def _qv_ctx(monkeypatch, d, chunks, table=True):
    monkeypatch.setenv("RC_LOCALITY", "force")
    monkeypatch.setenv("RC_PIPELINE_CHUNKS", str(chunks))
    return tqv._ctx(d, table)


def _qv_bytes_device(oracle, ctx, d):
    import torch
    _ar, a, qa, off = tqv._one_arena(oracle, d)
    n, max_len = len(off) - 1, int(np.diff(off.astype(np.int64)).max()) - 1
    seq, qual, t_off = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(qa.copy()).cuda(), torch.from_numpy(off.astype(np.int32)).cuda()
    res = [torch.full((n,), -77, dtype=torch.int32, device="cuda") for _ in range(4)]
    ctx.correct_device(d["mode"], n, int(seq.numel()), max_len, seq, qual, t_off, *res)
    ctx.sync()
    return [r.cpu().numpy() for r in res] + [seq.cpu().numpy()]


def _qv_bits_batch(oracle, ctx, d):
    """rc_correct_batch in quality-bit mode: a paired batch's second bit array lies apart (qual_split / qual_base2)"""
    ctx.set_quality_bits(True)
    ar = tqv._arenas(oracle, d)
    for j in range(1, len(ar), 3):
        ar[j] = ctx.pack_quality_bits(ar[j], d["badq"])
    return list(ctx.correct_batch(d["mode"], *ar)) + [np.concatenate(ar[0::3])]


def _through_fix_list(ctx, res, arena):
    host = arena.copy()
    ctx.apply_fixes(host, res[4], res[5])
    return list(res[:4]) + [host]


def _qv_packed(oracle, ctx, d):
    _ar, a, qa, off = tqv._one_arena(oracle, d)
    arena = ctx.host_array(a.size)
    arena[:] = a
    bases, exc_pos, exc_chr = ctx.pack_bases(arena, bases=ctx.host_array((a.size + 15) // 16, np.uint32))
    ctx.submit_packed(0, d["mode"], arena.size, off, bases, tqv._quality_bits(ctx, d, qa), exc_pos, exc_chr)
    return _through_fix_list(ctx, ctx.wait_packed(0), a)


def _qv_resident(oracle, ctx, d):
    ar, a, qa, off = tqv._one_arena(oracle, d)
    ctx.count_keep(True)
    ctx.count_begin()
    ctx.count_add(ar[0])
    args = dict(arena_a=0, begin_a=0, bytes_a=ar[0].size)
    if d["mode"] == 1:
        ctx.count_add(ar[3])
        args.update(arena_b=1, begin_b=0, bytes_b=ar[3].size)
    ctx.count_finish(2)
    ctx.table_build(d["keys"], d["counts"])   # (counting built a table of its own: the data set's goes back in)
    ctx.set_run_params(d["rate"], d["badq"])
    ctx.submit_resident(0, d["mode"], off, tqv._quality_bits(ctx, d, qa), **args)
    return _through_fix_list(ctx, ctx.wait_resident(0), a)


QV_ROUTES = {"bytes_device": _qv_bytes_device, "bits_batch": _qv_bits_batch, "packed": _qv_packed, "resident": _qv_resident}


@pytest.mark.parametrize("route", sorted(QV_ROUTES))
@pytest.mark.parametrize("name", QV)
def test_quality_modes_in_chunks(oracle, monkeypatch, name, route):
    d, want = tqv._case(oracle, name)
    assert max(len(r) for r in d["seqs1"] + (d["seqs2"] or [])) == 100, "at most 160 bases: not a tiered batch"
    assert datasets.quality_dependent(oracle, d, want) >= 30, "the qualities are to decide on %s" % name
    assert (name == QV[0]) == (d["mode"] == 1)
    want = list(want[:4]) + [np.concatenate(want[4:])]
    got = {}
    for c in (0, CHUNKS):
        ctx = _qv_ctx(monkeypatch, d, c, table=route != "resident")
        got[c] = QV_ROUTES[route](oracle, ctx, d)
        # 100-base reads: 32 a tile (the 4 096-byte tile); 1 500 reads are 47 tiles, the last one of 28 reads
        ran = (1, chunks_expected(len(want[0]), reads_per_tile(100), c)) if c else (0, 0)
        assert ran in ((0, 0), (1, 3)) and len(want[0]) % 32 != 0
        assert ctx.debug_pipeline() == ran, "%s through %s, RC_PIPELINE_CHUNKS=%d: %r" % (name, route, c, ctx.debug_pipeline())
        ctx.close()
    tpc._equal(want, got[CHUNKS], "%s through %s in %d chunks, against the oracle" % (name, route, CHUNKS))
    tpc._equal(got[0], got[CHUNKS], "%s through %s in %d chunks, against no chunks" % (name, route, CHUNKS))


def test_two_lanes_pipelines_in_flight_keep_their_own_qualities(oracle, monkeypatch):
    """The same reads in slots 0 and 1 at once with a different quality model each, lanes on: two contexts' pipelines, four
    streams.  First as byte batches, then as packed ones; rc_debug_pipeline and rc_summary add the lane to the context."""
    cases = [tqv._case(oracle, "qv_mixed_pe/high"), tqv._case(oracle, "qv_mixed_pe/straddle")]
    assert cases[0][0]["seqs1"] == cases[1][0]["seqs1"] and int((cases[0][1][0] != cases[1][1][0]).sum()) >= 30
    wants = [list(w[:4]) + [np.concatenate(w[4:])] for _, w in cases]
    n = len(wants[0][0])
    per_batch = chunks_expected(n, reads_per_tile(100), CHUNKS)
    got = {}
    for c in (0, CHUNKS):
        ctx = _qv_ctx(monkeypatch, cases[0][0], c)
        ctx.set_slot_lanes(True)
        held = []
        for slot, (d, _w) in enumerate(cases):
            ar = tqv._arenas(oracle, d)
            ctx.submit(slot, d["mode"], *ar)
            held.append(ar)
        got[c, "bytes"] = {slot: list(ctx.wait(slot)) + [np.concatenate(held[slot][0::3])] for slot in (1, 0)}
        assert ctx.debug_pipeline() == ((2, 2 * per_batch) if c else (0, 0)), "a lane made in this test reads RC_PIPELINE_CHUNKS itself"
        held = []
        for slot, (d, _w) in enumerate(cases):
            _ar, a, qa, off = tqv._one_arena(oracle, d)
            arena = ctx.host_array(a.size)
            arena[:] = a
            bases, exc_pos, exc_chr = ctx.pack_bases(arena, bases=ctx.host_array((a.size + 15) // 16, np.uint32))
            ctx.submit_packed(slot, d["mode"], arena.size, off, bases, tqv._quality_bits(ctx, d, qa), exc_pos, exc_chr)
            held.append(a)
        got[c, "packed"] = {slot: _through_fix_list(ctx, ctx.wait_packed(slot), held[slot]) for slot in (1, 0)}
        assert ctx.debug_pipeline() == ((4, 4 * per_batch) if c else (0, 0))
        assert ctx.summary() == (4 * n, 2 * sum(int(w[0][w[0] > 0].sum()) for w in wants))
        ctx.close()
    for kind in ("bytes", "packed"):
        for slot in (0, 1):
            what = "%s slot %d of two in %d chunks" % (kind, slot, CHUNKS)
            tpc._equal(wants[slot], got[CHUNKS, kind][slot], what + ", against the oracle")
            tpc._equal(got[0, kind][slot], got[CHUNKS, kind][slot], what + ", against no chunks")


# ---- C5: where the pipeline stands aside ---------------------------------------------------------------------------------------

def _traced(ctx, d):
    """rc_correct_batch_traced through the C ABI (tests/test_change_report.py: via_traced): results and the five trace arrays"""
    from oracle import pyoracle as po
    max_iter, words = 4, 36   # RC_TRACE_ITER_WORDS
    _a, _qa, off, _n1, args = tot.packed(po, d, 0, len(d["seqs1"]))
    args = list(args)
    b, res, _keep = ctx._batch(d["mode"], *(args + [None] * (6 - len(args))))
    nbytes, reads = sum(a.size for a in args[0::3]), len(res[0])
    bufs = [np.zeros(nbytes, np.int32), np.zeros(nbytes, np.int32), np.zeros(reads, np.int32), np.zeros(reads, np.int32),
            np.zeros(reads * max_iter * words, np.int32)]
    t = _Trace(max_iter, *[x.ctypes.data for x in bufs])
    rc = rcorrector_amd.load_library().rc_correct_batch_traced(C.c_void_p(ctx._h), C.byref(b), C.byref(t))
    assert rc == 0, rc
    # the two count arrays hold a count where a k-mer of a read starts; the k bytes behind a read's last k-mer (its NUL among
    # them) are written by no kernel and show whatever the buffer held before
    held = np.zeros(nbytes, bool)
    for lo, hi in zip(off[:-1].astype(np.int64), off[1:].astype(np.int64)):
        held[lo:max(lo, hi - d["k"])] = True
    # of the iteration records the header defines the first min(n_iter, max_iter) of a read, and the 32 bitmap words of a
    # record only where its word 2 says that the bitmap was reached; the rest is as the device buffer was
    it = bufs[4].reshape(reads, max_iter, words).copy()
    recorded = np.arange(max_iter)[None, :] < np.minimum(bufs[3], max_iter)[:, None]
    it[~recorded] = 0
    it[recorded & (it[:, :, 2] != 1), 4:] = 0
    return list(res) + [np.concatenate(args[0::3])], [bufs[0][held], bufs[1][held], bufs[2], bufs[3], it]


def test_the_traced_entry_point_stands_aside(oracle, monkeypatch):
    """rc_correct_pipelined returns before it launches anything while a trace is armed (trace_cap != 0): the traced k_correct is
    read back step by step, and the counts before the correction are taken from one whole probe launch"""
    d, want = tpc._case("few")
    want = list(want[:4]) + [np.concatenate(want[4:])]
    got = {}
    for c in (0, CHUNKS):
        ctx = tpc._context(monkeypatch, d, {}, c)
        got[c] = _traced(ctx, d)
        assert ctx.debug_pipeline() == (0, 0), "RC_PIPELINE_CHUNKS=%d under a trace" % c
        ctx.close()
    tpc._equal(want, got[CHUNKS][0], "traced, RC_PIPELINE_CHUNKS=%d, against the oracle" % CHUNKS)
    tpc._equal(got[0][0], got[CHUNKS][0], "traced, RC_PIPELINE_CHUNKS=%d, against 0" % CHUNKS)
    for a, b, what in zip(got[0][1], got[CHUNKS][1], ["counts_before", "counts_after", "flags", "n_iter", "iter"]):
        assert np.array_equal(a, b), "the trace's %s differs between RC_PIPELINE_CHUNKS=0 and %d" % (what, CHUNKS)
    assert int(got[CHUNKS][1][3].sum()) > 0, "some read was traced through an iteration"


def test_the_instrumented_kernel_stands_aside(oracle, monkeypatch):
    """RC_PHASE_PROF=1: rc_launch_correct zeroes the phase counters at every launch, so a pipeline's second chunk would wipe
    the first one's -- the pipeline must not run (phase_prof).  The counters are sums over the listed reads of what one read's
    search does, whatever the wave it runs in: the same with RC_PIPELINE_CHUNKS=0 and 3 if the same one launch made them."""
    d, want = tpc._case("pe150")
    want = list(want[:4]) + [np.concatenate(want[4:])]
    got = {}
    for c in (0, CHUNKS):
        ctx = tpc._context(monkeypatch, d, {"RC_PHASE_PROF": "1"}, c)
        ctx.profile_reset()
        fetched, _routes, _n, _max_len = _run_device(ctx, d)
        got[c] = (fetched, ctx.profile_correct_counters())
        assert ctx.debug_pipeline() == (0, 0), "RC_PIPELINE_CHUNKS=%d under RC_PHASE_PROF=1" % c
        ctx.close()
    tpc._equal(want, got[CHUNKS][0], "RC_PHASE_PROF=1, RC_PIPELINE_CHUNKS=%d, against the oracle" % CHUNKS)
    tpc._equal(got[0][0], got[CHUNKS][0], "RC_PHASE_PROF=1, RC_PIPELINE_CHUNKS=%d, against 0" % CHUNKS)
    print("(reads listed, gather rounds, bucket requests): %r without chunks, %r with RC_PIPELINE_CHUNKS=%d" % (got[0][1], got[CHUNKS][1], CHUNKS))
    assert got[CHUNKS][1][0] > 0
    assert got[CHUNKS][1] == got[0][1]


@pytest.mark.parametrize("env,why", [({"RC_NO_CLASSIFY": "1"}, "the follower's lists are made of the classification"),
                                     ({"RC_LOCALITY": "off"}, "the chunks are stretches of the locality list, which this batch has not")],
                         ids=["no_classify", "locality_off"])
def test_batches_the_pipeline_cannot_take(oracle, monkeypatch, env, why):
    d, want = tpc._case("pe150")
    want = list(want[:4]) + [np.concatenate(want[4:])]
    ctx = tpc._context(monkeypatch, d, env, CHUNKS)
    arrays = tsw._device_arrays(d)   # (no routes here: rc_debug_routes has none to show without the classification)
    res, work = tpc._launch(ctx, d, arrays)
    ctx.sync()
    tpc._equal(want, tpc._fetch(res, work), "pe150 under %s with RC_PIPELINE_CHUNKS=%d, against the oracle" % (env, CHUNKS))
    assert ctx.debug_pipeline() == (0, 0), "%s: %s" % (env, why)
    ctx.close()


# ---- C6: one context, piped and tiered batches in turn -------------------------------------------------------------------------

def test_piped_tiered_and_larger_piped_batches_on_one_context(oracle, monkeypatch):
    """40 reads piped, 3 001 reads tiered (one of 200 bases: the pipeline stands aside), 3 000 reads piped -- every follower-side
    buffer reserved for the first batch is reserved again, larger, for the third -- with one sync at the end"""
    names = ["few", "long", "pe150"]
    cases = [tpc._case(nm) for nm in names]
    assert all(np.array_equal(cases[0][0]["keys"], d["keys"]) for d, _ in cases), "one table for all three"
    arrays = [tsw._device_arrays(d) for d, _ in cases]
    assert arrays[0][1] == 40 and arrays[1][2] == 200 and arrays[2][1] == 3000 > arrays[0][1]
    ctx = tpc._context(monkeypatch, cases[0][0], {}, CHUNKS)
    launched = [tpc._launch(ctx, d, a) for (d, _), a in zip(cases, arrays)]
    ctx.sync()
    for nm, (_, want), r in zip(names, cases, launched):
        tpc._equal(list(want[:4]) + [np.concatenate(want[4:])], tpc._fetch(*r), "%s, one of three batches on one context" % nm)
    assert ctx.debug_pipeline() == (2, chunks_expected(40, 16, CHUNKS) + chunks_expected(3000, 16, CHUNKS)) == (2, 6)
    ctx.close()
