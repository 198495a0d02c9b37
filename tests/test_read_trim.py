"""GPU: rc_read_trim_device (Context.read_trim_device; kernel in rcorrector_amd/csrc/rc_trim.hip) on the synthetic batches of
tests/trim_cases.py, each named by the edge it hits: the rows, d_keep and the tally equal tests/trim_model.py exactly.  Then the
arena's alignment, the grid-stride wrap, the tally added onto, the optional outputs, the calls that do nothing or are refused,
and the offset the pair cut shares with the mate-overlap report."""
import ctypes

import numpy as np
import pytest

import rcorrector_amd
import trim_cases as tc
import trim_model as tm
from rcorrector_amd import binding as B

pytestmark = pytest.mark.gpu
RC_STATUS_ARG = -1
SCENARIOS = tc.all_scenarios()


def bare_ctx():
    return rcorrector_amd.Context(k=23, max_fix_per_k=4, device=0)     # (no table: trimming needs none)


def params_of(p):
    return B.trim_params(p["qual_min"], p["qual_base"], p["adapter1"], p["adapter2"], p["adapter_min"], p["adapter_mm_pct"], p["pair_overlap"],
                         p["pair_min_overlap"], p["pair_mm_pct"], p["min_len"])


def on_device(arena, lead, exact=False):
    """a copy of `arena` that starts `lead` bytes behind a 16-byte boundary of device memory, letters in front of and behind it;
    exact: the allocation ends with the arena's last byte"""
    import torch
    buf = torch.full((lead + arena.size + (0 if exact else 64),), ord("A"), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if arena.size:
        buf[lead:lead + arena.size] = torch.from_numpy(arena.copy()).cuda()
    return buf


def run(ctx, seqs, quals, mode, p, max_read_len, lead=0, exact=False, tally=None, want_keep=True, want_tally=True):
    """(rows, keep or None, the tally as a dict or None, the device tally)"""
    import torch
    arena, off = rcorrector_amd.pack_reads(seqs)
    t_seq = on_device(arena, lead, exact)
    t_qual = None
    if quals is not None:
        qa, qoff = rcorrector_amd.pack_reads(quals)
        assert np.array_equal(off, qoff)
        t_qual = on_device(qa, lead, exact)
    t_off = torch.from_numpy(off.astype(np.int32)).cuda()
    n = len(seqs)
    units = n if mode == 0 else n // 2
    d_out = torch.full((max(n, 1), 4), -7, dtype=torch.int32, device="cuda")
    d_keep = torch.full((max(units, 1),), 9, dtype=torch.uint8, device="cuda") if want_keep else None
    if tally is None and want_tally:
        tally = torch.zeros(B.TRIM_TALLY_WORDS, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.read_trim_device(t_seq.data_ptr() + lead, None if t_qual is None else t_qual.data_ptr() + lead, t_off, n, arena.size, max_read_len, mode, params_of(p),
                         d_out, d_keep, tally)
    ctx.sync()
    return (d_out.cpu().numpy()[:n], None if d_keep is None else d_keep.cpu().numpy()[:units],
            None if tally is None else B.trim_tally_dict(tally.cpu().numpy()), tally)


def assert_equal(got, want, what=""):
    rows, keep, tally = got[:3]
    assert np.array_equal(rows, want[0]), "%s rows: first difference at read %d" % (what, int(np.argmax((rows != want[0]).any(axis=1))))
    assert np.array_equal(keep, want[1]), what + " keep"
    for k in tm.empty_tally():
        assert np.array_equal(np.asarray(tally[k], np.uint64), np.asarray(want[2][k], np.uint64)), "%s tally %s" % (what, k)


@pytest.fixture(scope="module")
def ctx():
    c = bare_ctx()
    yield c
    c.close()


@pytest.mark.parametrize("i", range(len(SCENARIOS)), ids=[s["name"] for s in SCENARIOS])
def test_device_equals_the_model(ctx, i):
    s = SCENARIOS[i]
    assert_equal(run(ctx, s["seqs"], s["quals"], s["mode"], s["p"], s["max_read_len"], lead=i % 16), tc.expected(i), s["name"])


def _mixed(rng, n_pairs):
    """pairs of 37 to 150 bases, some overlapping, some run through, with adapters behind the fragment and noisy qualities"""
    seqs, quals = [], []
    for _ in range(n_pairs):
        La, Lb, F = (int(x) for x in rng.integers(37, 151, 3))
        a, b = tc.pair_of(rng, F, La, Lb, tail=tc.AD)
        seqs += [a, b]
        quals += [tc.rand_qual(rng, La, 15, 41)[:La - 5] + tc.rand_qual(rng, 5, 2, 30), tc.rand_qual(rng, Lb, 2, 41)]
    return seqs, quals


@pytest.fixture(scope="module")
def mixed():
    seqs, quals = _mixed(np.random.default_rng(5), 40)
    p = tm.params()
    return seqs, quals, p, {mode: tm.trim_batch(seqs, quals, mode, p) for mode in (0, 1, 2)}


@pytest.mark.parametrize("lead", range(16))
def test_every_alignment_of_the_arena(ctx, mixed, lead):
    seqs, quals, p, want = mixed
    mode = lead % 3
    assert_equal(run(ctx, seqs, quals, mode, p, 150, lead=lead), want[mode], "lead %d" % lead)


def test_the_last_read_ends_at_the_last_byte_of_the_allocation(ctx, mixed):
    seqs, quals, p, want = mixed
    for lead in (0, 7):
        assert_equal(run(ctx, seqs, quals, 2, p, 150, lead=lead, exact=True), want[2])


def test_more_units_than_the_grid_has_waves(ctx):
    """20 000 pairs of 40 bases: 500 distinct ones, 40 times over -- the model runs once on the distinct ones"""
    rng = np.random.default_rng(6)
    seqs, quals = [], []
    for _ in range(500):
        F = int(rng.integers(28, 60))
        a, b = tc.pair_of(rng, F, 40, 40, tail=tc.AD)
        seqs += [a, b]
        quals += [tc.rand_qual(rng, 40, 2, 41), tc.rand_qual(rng, 40, 15, 41)]
    p = tm.params(min_len=25, pair_min_overlap=20)
    rows, keep, t = tm.trim_batch(seqs, quals, 2, p)
    reps = 40
    want_t = {k: (np.asarray(v, np.uint64) * np.uint64(reps)) for k, v in t.items()}
    got = run(ctx, seqs * reps, quals * reps, 2, p, 40)
    assert_equal(got, (np.tile(rows, (reps, 1)), np.tile(keep, reps), want_t))
    assert 0 < t["units_kept"] < 500 and t["pairs_overlapping"] > 100 and got[2]["units"] == 20000 > 256 * 7 * 4 * 2


def test_a_tally_is_added_to_and_the_optional_outputs_may_be_null(ctx, mixed):
    import torch
    seqs, quals, p, want = mixed
    start = torch.arange(B.TRIM_TALLY_WORDS, dtype=torch.int64, device="cuda") * 3 + 1
    rows, keep, tally, _ = run(ctx, seqs, quals, 1, p, 150, tally=start.clone())
    base = B.trim_tally_dict(start.cpu().numpy())
    for k in tm.empty_tally():
        assert np.array_equal(np.asarray(tally[k], np.uint64), np.asarray(base[k], np.uint64) + np.asarray(want[1][2][k], np.uint64)), k
    assert np.array_equal(rows, want[1][0]) and np.array_equal(keep, want[1][1])
    rows, keep, tally, _ = run(ctx, seqs, quals, 1, p, 150, want_keep=False, want_tally=False)
    assert np.array_equal(rows, want[1][0]) and keep is None and tally is None
    rows, keep, tally, _ = run(ctx, seqs, quals, 0, p, 150, want_keep=False)
    assert np.array_equal(rows, want[0][0]) and tm.tally_equal(tally, want[0][2])


def test_no_reads_is_no_launch_and_the_refusals_say_why(ctx):
    import torch
    L = rcorrector_amd.load_library()
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    off = torch.zeros(8, dtype=torch.int32, device="cuda")
    out = torch.full((8, 4), -7, dtype=torch.int32, device="cuda")
    keep = torch.full((8,), 9, dtype=torch.uint8, device="cuda")
    tal = torch.zeros(B.TRIM_TALLY_WORDS, dtype=torch.int64, device="cuda")
    s, o, r, k, t = buf.data_ptr(), off.data_ptr(), out.data_ptr(), keep.data_ptr(), tal.data_ptr()

    def dev(seq=s, qual=s, d_off=o, n=2, nbytes=4, max_len=1, mode=1, d_out=r, d_keep=k, d_tally=t, null_params=False, **pk):
        p = B.trim_params(**pk)
        return L.rc_read_trim_device(ctx._h, seq, qual, d_off, n, nbytes, max_len, mode, None if null_params else ctypes.byref(p), d_out, d_keep, d_tally)

    assert dev() == 0
    ctx.sync()
    assert tm.tally_equal(B.trim_tally_dict(tal.cpu().numpy()), tm.trim_batch([b"", b""], None, 1, tm.params())[2])      # one pair of two empty reads
    assert out.cpu().numpy()[:3].tolist() == [[0] * 4] * 2 + [[-7] * 4] and keep.cpu().numpy()[:2].tolist() == [0, 9]
    refused = [
        (dict(mode=-1), "mode -1"), (dict(mode=3), "mode 3"), (dict(n=3), "pairs need an even number of reads (got 3)"), (dict(n=3, mode=2), "pairs need an even number"),
        (dict(seq=None), "null pointer"), (dict(d_off=None), "null pointer"), (dict(d_out=None), "null pointer"), (dict(null_params=True), "params must not be NULL"),
        (dict(nbytes=1 << 32), "exceeds the 4 GiB batch limit"), (dict(max_len=1024), "max_read_len must be 0..1023 (got 1024)"), (dict(max_len=-1), "max_read_len"),
        (dict(adapter_min=0), "adapter_min must be 1..64 (got 0)"), (dict(adapter_min=65), "adapter_min must be 1..64 (got 65)"),
        (dict(adapter_mm_pct=-1), "adapter_mm_pct must be 0..50 (got -1)"), (dict(adapter_mm_pct=51), "adapter_mm_pct must be 0..50 (got 51)"),
        (dict(pair_mm_pct=-1), "pair_mm_pct must be 0..50 (got -1)"), (dict(pair_mm_pct=51), "pair_mm_pct must be 0..50 (got 51)"),
        (dict(pair_min_overlap=0), "pair_min_overlap must be 1..1023 (got 0)"), (dict(pair_min_overlap=1024), "pair_min_overlap must be 1..1023 (got 1024)"),
        (dict(min_len=-1), "min_len must be 0..1023 (got -1)"), (dict(min_len=1024), "min_len must be 0..1023 (got 1024)"),
        (dict(adapter1_len=65), "adapter1_len must be 0..64 (got 65)"), (dict(adapter2_len=-1), "adapter2_len must be 0..64 (got -1)"),
        (dict(adapter1=b"ACGN"), "adapter1 holds a base outside upper-case ACGT at position 3"), (dict(adapter2=b"acgt"), "adapter2 holds a base outside upper-case ACGT at position 0"),
        (dict(qual_min=-1), "qual_min must be 0..93 (got -1)"), (dict(qual_min=94), "qual_min must be 0..93 (got 94)"), (dict(qual_base=256), "qual_base must be 0..255 (got 256)"),
        (dict(d_out=r + 2), "d_out must lie on a 4-byte boundary"), (dict(d_tally=t + 4), "d_tally on an 8-byte one"),
    ]
    for kw, text in refused:
        assert dev(**kw) == RC_STATUS_ARG, kw
        err = L.rc_last_error(ctx._h).decode()
        assert err.startswith("read_trim_device: ") and text in err, (kw, err)
        if not set(kw) & {"n", "seq", "d_off", "d_out", "d_tally"}:      # (checked whatever n_reads is)
            assert dev(**dict(kw, n=0, seq=None, qual=None, d_off=None, d_out=None, d_keep=None, d_tally=None)) == RC_STATUS_ARG, kw
    assert dev(mode=0, n=3, nbytes=4) == 0                                   # (single reads may be odd in number)
    before = tal.clone()
    assert dev(n=0, seq=None, qual=None, d_off=None, d_out=None, d_keep=None, d_tally=None) == 0
    assert dev(n=0) == 0
    ctx.sync()
    assert torch.equal(before, tal)
    with pytest.raises(rcorrector_amd.RcorrectorError, match="qual_min must be 0..93"):
        ctx.read_trim_device(buf, None, off, 2, 4, 1, 1, B.trim_params(qual_min=100), out)
    with pytest.raises(ValueError, match="at most 64 bases"):
        B.trim_params(adapter1=b"A" * 65)


def test_the_pair_cut_and_the_overlap_report_choose_the_same_offset(ctx):
    """no other cut, min_len 0: mate 1's keep_len is min(La, F), so over pairs whose fragments are all shorter than mate 1 the
    histogram of mate 1's keep_len is the report's frag histogram"""
    import torch
    rng = np.random.default_rng(8)
    seqs = []
    for n in range(300):
        La, Lb = (int(x) for x in rng.integers(80, 151, 2))
        F = int(rng.integers(35, La)) if n % 5 else int(rng.integers(10, 30))       # (every fifth: too short to be accepted)
        a, b = tc.pair_of(rng, F, La, Lb, tail=b"")                                  # ... and then random bases behind the fragment
        a, b = a + tc.rand_seq(rng, La - len(a)), b + tc.rand_seq(rng, Lb - len(b))
        a = bytearray(a)
        for j in set(rng.integers(0, min(F, La), int(rng.integers(0, 5))).tolist()):     # a few disagreements inside the overlap
            a[j] = b"ACGTN"[(b"ACGT".index(a[j]) + 1 + int(rng.integers(0, 4))) % 5]
        seqs += [bytes(a), b]
    p = tm.params(qual_min=0, adapter1=b"", min_len=0)
    rows, keep, tally, _ = run(ctx, seqs, None, 2, p, 150, lead=3)
    arena, off = rcorrector_amd.pack_reads(seqs)
    t_seq, t_off = torch.from_numpy(arena).cuda(), torch.from_numpy(off.astype(np.int32)).cuda()
    counts = torch.zeros(B.OVERLAP_WORDS, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.mate_overlap_device(t_seq, t_seq, t_off, len(seqs), arena.size, 150, 2, counts)
    ctx.sync()
    rep = B.mate_overlap_dict(counts.cpu().numpy())
    assert tally["pairs_overlapping"] == rep["overlapping"] and 200 < rep["overlapping"] < 300 and rep["pairs"] == tally["units"] == 300
    La = np.array([len(s) for s in seqs[0::2]])
    cut = rows[0::2, 3] < La                                   # the pairs whose fragment is shorter than mate 1
    frag = np.bincount(rows[0::2, 3][cut], minlength=B.OVERLAP_FRAG_LEN)
    uncut = int(rep["overlapping"]) - int(cut.sum())           # accepted with F >= La: frag bins at or above La
    assert uncut >= 0 and np.array_equal(frag[:80], rep["frag"][:80].astype(np.int64))        # (below the shortest mate 1 every bin is a cut pair's)
    assert int(rep["frag"].sum()) - int(frag.sum()) == uncut
    hist = tally["keep_hist"][0].astype(np.int64)
    assert np.array_equal(hist[:80], rep["frag"][:80].astype(np.int64)) and tm.tally_equal(tally, tm.trim_batch(seqs, None, 2, p)[2])
