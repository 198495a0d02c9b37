"""GPU: the three vetoes that close k_correct (rc_correct_core.h: pairwise, end-of-read, density) all read the base qualities,
and the older parity sets never let a quality decide anything: every fix there lands on a base below the threshold.  Here the
qv_ data sets (tests/datasets.py; tests/test_quality_datasets.py asserts on the oracle that qualities decide on them) go through
every way a quality reaches the kernel -- byte arenas, quality bits, the packed and the resident boundary, memory the caller
keeps in HBM, slots in flight -- and through the alternative kernel paths and the compiled-for-k instances.  Every comparison is
with the oracle, read for read: ret, l, m, h and the corrected bytes, all exactly equal (integer work, no tolerance)."""
import numpy as np
import pytest

import datasets
import rcorrector_amd

pytestmark = pytest.mark.gpu

WHAT = ["ret", "l", "m", "h", "seq1", "seq2"]
NOT_FASTA = [n for n in datasets.QV_NAMES if not n.endswith("/fasta")]
FASTA = [n for n in datasets.QV_NAMES if n.endswith("/fasta")]
# one member per family where the threshold byte itself occurs, and the mixed lengths
BOUNDARY = ["qv_pair/straddle", "qv_ends/straddle", "qv_dense_mfk2/straddle", "qv_dense_mfk1/straddle", "qv_mixed_pe/straddle", "qv_mixed_il/straddle",
            "qv_lengths/straddle", "qv_signed/signed"]


_CASES = {}


def _case(oracle, name, pad_to=0):
    """(data set, the oracle's results on it): computed once per name, left unchanged"""
    if (name, pad_to) not in _CASES:
        d = datasets.make(name)
        if pad_to:
            keys, cnt = datasets.pad_table(d["keys"], d["counts"], d["k"], pad_to, 9300 + d["k"])
            d = dict(d, keys=keys, counts=cnt)
        want = datasets.run_oracle(oracle, d)
        for a in want:
            a.setflags(write=False)
        _CASES[name, pad_to] = (d, want)
    return _CASES[name, pad_to]


def _ctx(d, table=True):
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    if table:
        ctx.table_build(d["keys"], d["counts"])
        ctx.set_run_params(d["rate"], d["badq"])
    return ctx


def _arenas(oracle, d):
    """[seq1, qual1, off1(, seq2, qual2, off2)]: fresh arrays, the arguments of correct_batch / submit after the mode"""
    out = []
    for s, q in ((d["seqs1"], d["quals1"]), (d["seqs2"], d["quals2"])):
        if s is not None:
            a, off = oracle.pack_reads(s)
            out += [a, oracle.pack_reads(q)[0], off]
    return out


def _same(want, got, note):
    for w, g, what in zip(want, got, WHAT):
        bad = np.nonzero(w != g)[0]
        assert len(bad) == 0, "%s differs %s at %s (want %s got %s)" % (what, note, bad[:5], w[bad[:5]], g[bad[:5]])


def _byte_path(oracle, ctx, d, want, note):
    ar = _arenas(oracle, d)
    got = ctx.correct_batch(d["mode"], *ar) + tuple(ar[0::3])
    _same(want, got, note)


@pytest.mark.parametrize("name", datasets.QV_NAMES)
def test_byte_arenas(oracle, name):
    """rc_correct_batch, quality bytes as they are: thresholds '!', 'H' and '~', bytes equal to the threshold, bytes above
    0x7F (compared as signed chars), no qualities at all (qual[0] == 0), max_fix_per_k from 1 to 8."""
    d, want = _case(oracle, name)
    if "dense" in name:
        assert int((want[0] == -1).sum()) >= 20, "the density veto rejects too few reads of %s" % name
    ctx = _ctx(d)
    _byte_path(oracle, ctx, d, want, "on %s" % name)
    reads, cors = ctx.summary()
    assert reads == len(want[0]) and cors == int(want[0][want[0] > 0].sum())
    ctx.close()


@pytest.mark.parametrize("name", NOT_FASTA)
def test_quality_bits(oracle, name):
    """rc_set_quality_bits + rc_pack_quality_bits: the bit array is `quality > threshold` on signed chars, computed here in
    numpy, and the results are the oracle's on the bytes."""
    d, want = _case(oracle, name)
    thr = d["badq"][0]
    ctx = _ctx(d)
    ctx.set_quality_bits(True)
    ar = _arenas(oracle, d)
    for j in range(1, len(ar), 3):
        qa = ar[j]
        qb = ctx.pack_quality_bits(qa, d["badq"])
        assert qb.size == (qa.size + 7) // 8
        assert np.array_equal(np.unpackbits(qb, bitorder="little")[:qa.size], (qa.view(np.int8) > np.int8(thr)).astype(np.uint8)), "the bit array of %s" % name
        ar[j] = qb
    got = ctx.correct_batch(d["mode"], *ar) + tuple(ar[0::3])
    _same(want, got, "on %s in quality-bit mode" % name)
    ctx.close()


def _one_arena(oracle, d):
    """(arena, qualities, offsets) with the second mates behind the first, as the packed and the resident boundary take them"""
    ar = _arenas(oracle, d)
    a, qa, off = ar[:3]
    if d["mode"] == 1:
        off = np.concatenate([off, (ar[5][1:].astype(np.int64) + a.size).astype(np.uint32)])
        a, qa = np.concatenate([a, ar[3]]), np.concatenate([qa, ar[4]])
    return ar, a, qa, off


def _quality_bits(ctx, d, qa):
    if d["fasta"]:
        return None
    qb = ctx.host_array((qa.size + 7) // 8)
    ctx.pack_quality_bits(qa, d["badq"], out=qb)
    return qb


def _same_through_a_fix_list(ctx, want, res, arena, note):
    ret, l, m, h, fix_pos, fix_chr = res
    host = arena.copy()
    ctx.apply_fixes(host, fix_pos, fix_chr)
    _same(want[:4] + (np.concatenate(want[4:]),), (ret, l, m, h, host), note)
    assert len(fix_pos) == len(np.unique(fix_pos)) == int(want[0][want[0] > 0].sum())


@pytest.mark.parametrize("name", BOUNDARY + FASTA)
def test_packed_boundary(oracle, name):
    """rc_submit_packed / rc_wait_packed: a quality bit per base goes down, or (the fasta members) no quality array at all;
    the caller's arena plus the fix list is the oracle's corrected arena."""
    d, want = _case(oracle, name)
    ctx = _ctx(d)
    _ar, a, qa, off = _one_arena(oracle, d)
    arena = ctx.host_array(a.size)
    arena[:] = a
    bases, exc_pos, exc_chr = ctx.pack_bases(arena, bases=ctx.host_array((a.size + 15) // 16, np.uint32))
    ctx.submit_packed(0, d["mode"], arena.size, off, bases, _quality_bits(ctx, d, qa), exc_pos, exc_chr)
    _same_through_a_fix_list(ctx, want, ctx.wait_packed(0), a, "on %s through the packed boundary" % name)
    ctx.close()


@pytest.mark.parametrize("name", BOUNDARY + FASTA)
def test_resident_boundary(oracle, name):
    """rc_submit_resident / rc_wait_resident: the reads are the arenas the counter kept in HBM, only offsets and quality bits
    (or no qualities) go down."""
    d, want = _case(oracle, name)
    ctx = _ctx(d, table=False)
    ar, a, qa, off = _one_arena(oracle, d)
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
    ctx.submit_resident(0, d["mode"], off, _quality_bits(ctx, d, qa), **args)
    _same_through_a_fix_list(ctx, want, ctx.wait_resident(0), a, "on %s through the resident boundary" % name)
    ctx.close()


@pytest.mark.parametrize("name", ["qv_mixed_pe/straddle", "qv_mixed_pe/high", "qv_mixed_pe/fasta", "qv_mixed_pe_q126/straddle", "qv_lengths/straddle",
                                  "qv_lengths/fasta", "qv_signed/signed"])
def test_correct_device(oracle, name):
    """rc_correct_device: reads and quality bytes already in HBM, corrected in place"""
    import torch
    d, want = _case(oracle, name)
    dev = torch.device("cuda", 0)
    _ar, a, qa, off = _one_arena(oracle, d)
    n, max_len = len(off) - 1, int(np.diff(off.astype(np.int64)).max()) - 1
    seq, qual, t_off = torch.from_numpy(a.copy()).to(dev), torch.from_numpy(qa.copy()).to(dev), torch.from_numpy(off.astype(np.int32)).to(dev)
    res = [torch.full((n,), -77, dtype=torch.int32, device=dev) for _ in range(4)]
    ctx = _ctx(d)
    ctx.correct_device(d["mode"], n, int(seq.numel()), max_len, seq, qual, t_off, *res)
    ctx.sync()
    _same(want[:4] + (np.concatenate(want[4:]),), [r.cpu().numpy() for r in res] + [seq.cpu().numpy()], "on %s in the caller's device memory" % name)
    ctx.close()


@pytest.mark.parametrize("lanes", [True, False])
def test_two_slots_in_flight_keep_their_own_qualities(oracle, lanes):
    """The same reads in two slots at once, with a different quality model each -- first as byte batches, then as packed ones:
    a slot that read the other slot's qualities would give the other slot's results, and the two differ."""
    cases = [_case(oracle, "qv_mixed_pe/high"), _case(oracle, "qv_mixed_pe/straddle")]
    assert cases[0][0]["seqs1"] == cases[1][0]["seqs1"] and int((cases[0][1][0] != cases[1][1][0]).sum()) >= 30
    ctx = _ctx(cases[0][0])
    ctx.set_slot_lanes(lanes)
    held = []
    for slot, (d, _want) in enumerate(cases):
        ar = _arenas(oracle, d)
        ctx.submit(slot, d["mode"], *ar)
        held.append(ar)
    for slot in (1, 0):
        _same(cases[slot][1], ctx.wait(slot) + tuple(held[slot][0::3]), "in byte slot %d of two (lanes %s)" % (slot, lanes))
    held = []
    for slot, (d, _want) in enumerate(cases):
        _ar, a, qa, off = _one_arena(oracle, d)
        arena = ctx.host_array(a.size)
        arena[:] = a
        bases, exc_pos, exc_chr = ctx.pack_bases(arena, bases=ctx.host_array((a.size + 15) // 16, np.uint32))
        ctx.submit_packed(slot, d["mode"], arena.size, off, bases, _quality_bits(ctx, d, qa), exc_pos, exc_chr)
        held.append(a)
    for slot in (1, 0):
        _same_through_a_fix_list(ctx, cases[slot][1], ctx.wait_packed(slot), held[slot], "in packed slot %d of two (lanes %s)" % (slot, lanes))
    ctx.close()


# the knobs that change which kernel finishes a read, or how
KNOBS = [{"RC_K3_GENERIC": "1"}, {"RC_NO_SINGLE": "1"}, {"RC_NO_ALT": "1"}, {"RC_NO_CLASSIFY": "1"}, {"RC_K2_WAVE_PER_READ": "1"}, {"RC_LOCALITY": "force"},
         {"RC_LOCALITY": "force", "RC_NO_FUSE": "1"}, {"RC_NO_TIER": "1"}, {"RC_TABLE_LAYOUT": "wide"}, {"RC_K3_LOCAL": "1", "RC_LOCALITY": "force"}]


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda d: "+".join("%s=%s" % kv for kv in d.items()))
@pytest.mark.parametrize("name", ["qv_mixed_pe/straddle", "qv_dense_mfk2/high"])
def test_alternative_code_paths(oracle, name, knobs, monkeypatch):
    for kk, v in knobs.items():
        monkeypatch.setenv(kk, v)
    d, want = _case(oracle, name)
    ctx = _ctx(d)
    _byte_path(oracle, ctx, d, want, "on %s under %s" % (name, knobs))
    ctx.close()


@pytest.mark.parametrize("k,pad_to,min_buckets", [(23, 30_000, 1 << 14), (25, 450_000, 1 << 18)])
def test_instances_compiled_for_k23_and_k25(oracle, k, pad_to, min_buckets):
    """k_correct's instances compiled for one k are taken over a PACKED table without extension bits, i.e. of at least
    2^(2k-32) home buckets (tests/test_k_sweep.py): the table is padded to that size with k-mers no read holds, the oracle gets
    the same table, and the layout is asserted.  (k = 31 and 32 run on the any-k instance in test_byte_arenas.)"""
    from test_k_sweep import _check_layout, _packed_home_buckets
    d, want = _case(oracle, datasets.qv_name("pair", "straddle", k=k), pad_to)
    assert len(d["keys"]) == pad_to
    ctx = _ctx(d)
    layout, ext = _check_layout(ctx, d)
    assert layout == 1 and ext == 0
    assert ctx.table_stats()["buckets"] >= min_buckets and _packed_home_buckets(pad_to) >= min_buckets
    _byte_path(oracle, ctx, d, want, "on qv_pair/straddle at k = %d over a table of %d entries" % (k, pad_to))
    ctx.close()


def test_batch_split_invariance(oracle):
    """qv_mixed_il/straddle as one batch and as three: a read's result does not depend on the batch it travels in"""
    d, want = _case(oracle, "qv_mixed_il/straddle")
    ctx = _ctx(d)
    n = len(d["seqs1"])
    cuts = [0, 2 * (n // 6), 2 * (n // 2) - 2 * (n // 12), n]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        a, off = oracle.pack_reads(d["seqs1"][lo:hi])
        qa, _ = oracle.pack_reads(d["quals1"][lo:hi])
        parts.append(ctx.correct_batch(2, a, qa, off) + (a,))
    assert len(parts) == 3 and all(len(p[0]) > 0 for p in parts)
    _same(want, [np.concatenate([p[j] for p in parts]) for j in range(5)], "on qv_mixed_il/straddle in three batches")
    _byte_path(oracle, ctx, d, want, "on qv_mixed_il/straddle in one batch")
    ctx.close()
