"""GPU: rc_read_merge_device (Context.read_merge_device; kernels in rcorrector_amd/csrc/rc_merge.hip) on the synthetic batches of
tests/merge_cases.py, each named by the edge it hits: the rows, d_moff, both output arenas and the tally equal
tests/merge_model.py exactly, and every byte of the output arenas at or behind d_moff[units] is still the poison they were filled
with.  Then the input arena's alignment, the output offsets' residues, the grid-stride wrap, the calls that do nothing or are
refused, the offset shared with read_trim and the mate-overlap report, the merged arena handed on to read_depth_device, and an
input arena across byte 2^31.  The rest of the high offsets -- both modes and the quality arenas up to byte 2^32 - 2, a merged
arena and d_moff past 2^31, and that arena handed on -- are in tests/test_high_arena.py (test_read_merge_device,
test_one_filled_arena_merged)."""
import ctypes

import numpy as np
import pytest

import high_arena as ha
import merge_cases as mc
import merge_model as mm
import rcorrector_amd
import trim_cases as tc
import trim_model as tm
from rcorrector_amd import binding as B

pytestmark = pytest.mark.gpu
RC_STATUS_ARG = -1
SCENARIOS = mc.all_scenarios()
POISON = 0xEE
SLACK = 96          # poison behind out_cap too: nothing may be written there either


def bare_ctx():
    return rcorrector_amd.Context(k=23, max_fix_per_k=4, device=0)     # (no table: merging needs none)


def params_of(p):
    return B.merge_params(p["min_overlap"], p["max_mismatch_pct"], p["qual_base"], p["qual_cap"])


def on_device(arena, lead):
    """a copy of `arena` that starts `lead` bytes behind a 16-byte boundary of device memory, letters in front of and behind it"""
    import torch
    buf = torch.full((lead + arena.size + 64,), ord("A"), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if arena.size:
        buf[lead:lead + arena.size] = torch.from_numpy(arena.copy()).cuda()
    return buf


def run(ctx, seqs, quals, mode, p, max_read_len, lead=0, tally=None, want_qual=True, want_tally=True, out=None):
    """{"rows", "moff", "mseq", "mqual" (the arenas up to d_moff[units]; None: not asked for), "tally", "bufs": the device
    tensors}.  The output arenas hold exactly out_cap = nbytes bytes and SLACK more, all poison before the call; asserts that
    every byte at or behind d_moff[units] still is.  out: the device tensors of an earlier run, to write into again"""
    import torch
    arena, off = rcorrector_amd.pack_reads(seqs)
    t_seq = on_device(arena, lead)
    t_qual = None
    if quals is not None:
        qa, qoff = rcorrector_amd.pack_reads(quals)
        assert np.array_equal(off, qoff)
        t_qual = on_device(qa, lead)
    t_off = torch.from_numpy(off.astype(np.int32)).cuda()
    n, units = len(seqs), len(seqs) // 2
    if out is None:
        out = {"rows": torch.full((max(units, 1), 4), -7, dtype=torch.int32, device="cuda"),
               "mseq": torch.full((arena.size + SLACK,), POISON, dtype=torch.uint8, device="cuda"),
               "mqual": torch.full((arena.size + SLACK,), POISON, dtype=torch.uint8, device="cuda") if quals is not None and want_qual else None,
               "moff": torch.full((units + 2,), -7, dtype=torch.int32, device="cuda")}
    if tally is None and want_tally:
        tally = torch.zeros(B.MERGE_TALLY_WORDS, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.read_merge_device(t_seq.data_ptr() + lead, None if t_qual is None else t_qual.data_ptr() + lead, t_off, n, arena.size, max_read_len, mode, params_of(p),
                          out["rows"], out["mseq"], out["mqual"], out["moff"], arena.size, tally)
    ctx.sync()
    moff = out["moff"].cpu().numpy().view(np.uint32)
    assert moff[units + 1] == np.uint32(-7 & 0xFFFFFFFF), "d_moff has units + 1 entries"
    moff = moff[:units + 1]
    total = int(moff[units])
    assert total <= arena.size
    res = {"rows": out["rows"].cpu().numpy()[:units], "moff": moff, "tally": None if tally is None else B.merge_tally_dict(tally.cpu().numpy()), "bufs": out}
    for k in ("mseq", "mqual"):
        if out[k] is None:
            res[k] = None
            continue
        assert bool((out[k][total:] == POISON).all()), "%s: a byte at or behind d_moff[units] = %d was written" % (k, total)
        res[k] = out[k][:total].cpu().numpy().tobytes()
    return res


def assert_equal(got, want, what=""):
    rows, moff, mseq, mqual, tally = want
    assert np.array_equal(got["rows"], rows), "%s rows: first difference at unit %d" % (what, int(np.argmax((got["rows"] != rows).any(axis=1))))
    assert np.array_equal(got["moff"], moff), what + " moff"
    assert got["mseq"] == mseq, "%s mseq: first difference at byte %d" % (what, next(i for i, (a, b) in enumerate(zip(got["mseq"], mseq)) if a != b))
    if got["mqual"] is not None or mqual is not None:
        assert got["mqual"] == mqual, "%s mqual: first difference at byte %d" % (what, next(i for i, (a, b) in enumerate(zip(got["mqual"], mqual)) if a != b))
    if got["tally"] is not None:
        for k in mm.TALLY_KEYS:
            assert np.array_equal(np.asarray(got["tally"][k], np.uint64), np.asarray(tally[k], np.uint64)), "%s tally %s" % (what, k)


@pytest.fixture(scope="module")
def ctx():
    c = bare_ctx()
    yield c
    c.close()


@pytest.mark.parametrize("i", range(len(SCENARIOS)), ids=[s["name"] for s in SCENARIOS])
def test_device_equals_the_model(ctx, i):
    s = SCENARIOS[i]
    assert_equal(run(ctx, s["seqs"], s["quals"], s["mode"], s["p"], s["max_read_len"], lead=i % 16), mc.expected(i), s["name"])


def test_modes_1_and_2_give_the_same_merged_arena(ctx):
    S = {s["name"]: i for i, s in enumerate(SCENARIOS)}
    s1, s2 = SCENARIOS[S["offsets mode 1"]], SCENARIOS[S["offsets mode 2"]]
    a, b = run(ctx, s1["seqs"], None, 1, s1["p"], 100), run(ctx, s2["seqs"], None, 2, s2["p"], 100)
    assert a["mseq"] == b["mseq"] == mc.expected(S["offsets without qualities"])[2] and np.array_equal(a["moff"], b["moff"]) and np.array_equal(a["rows"], b["rows"])
    assert mm.tally_equal(a["tally"], b["tally"])


def _mixed(rng, n_pairs, lo=37, hi=151):
    """pairs of lo to hi - 1 bases, some overlapping, some run through, some not at all, with a few disagreements, an N here and
    there and noisy qualities"""
    seqs, quals = [], []
    for n in range(n_pairs):
        La, Lb = (int(x) for x in rng.integers(lo, hi, 2))
        F = int(rng.integers(lo - 7, 2 * hi))
        a, b = tc.pair_of(rng, F, La, Lb, tail=tc.AD)
        a = bytearray(a)
        for j in set(rng.integers(0, La, int(rng.integers(0, 4))).tolist()):
            a[j] = b"ACGTN"[(b"ACGT".index(a[j]) + 1 + int(rng.integers(0, 4))) % 5] if a[j] in b"ACGT" else a[j]
        seqs += [bytes(a), b]
        quals += [tc.rand_qual(rng, La, 2, 41), tc.rand_qual(rng, Lb, 2, 41)]
    return seqs, quals


@pytest.fixture(scope="module")
def mixed():
    seqs, quals = _mixed(np.random.default_rng(5), 40)
    p = mm.params()
    want = {mode: mm.merge_batch(seqs if mode == 2 else seqs[0::2] + seqs[1::2], quals if mode == 2 else quals[0::2] + quals[1::2], mode, p) for mode in (1, 2)}
    t = want[2][4]
    assert 10 < t["merged"] < 40 and t["readthrough"] > 3 and t["took_mate1"] and t["took_mate2"] and mm.tally_equal(want[1][4], t)
    return seqs, quals, p, want


@pytest.mark.parametrize("lead", range(16))
def test_every_alignment_of_the_input_arena(ctx, mixed, lead):
    seqs, quals, p, want = mixed
    mode = 1 + lead % 2
    s, q = (seqs, quals) if mode == 2 else (seqs[0::2] + seqs[1::2], quals[0::2] + quals[1::2])
    assert_equal(run(ctx, s, q, mode, p, 150, lead=lead), want[mode], "lead %d" % lead)


def test_the_output_offsets_walk_every_residue_of_16(ctx):
    """the leading units take 33 bytes each, so d_moff[u] mod 16 is u mod 16: every position of a span's first and last byte in
    its granule; behind them merged lengths of 10 to 80 and unmerged units"""
    rng = np.random.default_rng(9)
    pairs = [tc.pair_of(rng, 32, 20, 22) for _ in range(18)] + [(tc.rand_seq(rng, 12), tc.rand_seq(rng, 14))] * 3
    pairs += [tc.pair_of(rng, F, min(F, (F + 11) // 2 + 1), min(F, (F + 11) // 2 + 1)) for F in range(10, 81)]      # (the mates overlap by 10 to 13)
    seqs = [m for pr in pairs for m in pr]
    quals = [tc.rand_qual(rng, len(s)) for s in seqs]
    p = mm.params(min_overlap=10, max_mismatch_pct=0)
    want = mm.merge_batch(seqs, quals, 2, p)
    assert want[0][:18, 0].tolist() == [32] * 18 and set((want[1][:18] % 16).tolist()) == set(range(16)) and want[0][18:21, 0].tolist() == [0] * 3
    assert want[0][21:, 0].tolist() == list(range(10, 81)) and set((want[1] % 16).tolist()) == set(range(16))
    assert_equal(run(ctx, seqs, quals, 2, p, 80, lead=3), want)
    assert_equal(run(ctx, seqs, quals, 2, p, 80, lead=0, want_qual=False), want[:3] + (None, want[4]))      # (the qualities decide, no arena of them)


def test_an_all_unmerged_batch_is_units_nul_bytes_and_no_pairs_is_nothing(ctx):
    import torch
    rng = np.random.default_rng(10)
    seqs = [tc.rand_seq(rng, int(n)) for n in rng.integers(0, 90, 2 * 37)]
    quals = [tc.rand_qual(rng, len(s)) for s in seqs]
    got = run(ctx, seqs, quals, 2, mm.params(), 90)
    assert got["mseq"] == b"\0" * 37 == got["mqual"] and got["moff"].tolist() == list(range(38)) and not got["rows"].any()
    assert got["tally"]["unmerged"] == 37 == got["tally"]["len_hist"][0] and got["tally"]["merged"] == 0
    assert_equal(got, mm.merge_batch(seqs, quals, 2, mm.params()))
    # units = 0: no launch, nothing written
    buf = torch.full((64,), POISON, dtype=torch.uint8, device="cuda")
    moff = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    rows = torch.full((1, 4), -7, dtype=torch.int32, device="cuda")
    tal = torch.zeros(B.MERGE_TALLY_WORDS, dtype=torch.int64, device="cuda")
    ctx.read_merge_device(buf, buf, moff, 0, 0, 0, 2, None, rows, buf, buf, moff, 0, tal)
    ctx.read_merge_device(None, None, None, 0, 0, 0, 1, None, None, None, None, None, 0, None)
    ctx.sync()
    assert bool((buf == POISON).all()) and bool((moff == -7).all()) and bool((rows == -7).all()) and not bool(tal.any())


def test_more_units_than_the_grid_has_waves_and_the_same_call_twice(ctx):
    """20 000 pairs of 40 bases: 500 distinct ones, 40 times over -- the model runs once on the distinct ones"""
    rng = np.random.default_rng(6)
    seqs, quals = [], []
    for _ in range(500):
        F = int(rng.integers(15, 90))
        a, b = tc.pair_of(rng, F, 40, 40, tail=tc.AD)
        seqs += [_noisy(rng, a), b]
        quals += [tc.rand_qual(rng, 40, 2, 41), tc.rand_qual(rng, 40, 15, 41)]
    p = mm.params(min_overlap=20)
    rows, moff, mseq, mqual, t = mm.merge_batch(seqs, quals, 2, p)
    reps = 40
    want_t = {k: (np.asarray(v, np.uint64) * np.uint64(reps)) for k, v in t.items()}
    want_moff = np.concatenate([(moff[:-1].astype(np.int64) + r * int(moff[-1])) for r in range(reps)] + [[reps * int(moff[-1])]]).astype(np.uint32)
    got = run(ctx, seqs * reps, quals * reps, 2, p, 40)
    assert_equal(got, (np.tile(rows, (reps, 1)), want_moff, mseq * reps, mqual * reps, want_t))
    assert 100 < t["merged"] < 500 and t["readthrough"] > 50 and t["mismatches"] > 50 and got["tally"]["pairs"] == 20000 > 256 * 8 * 4 * 2
    first = {k: got["bufs"][k].clone() for k in ("rows", "mseq", "mqual", "moff")}
    again = run(ctx, seqs * reps, quals * reps, 2, p, 40, out=got["bufs"])
    import torch
    assert all(torch.equal(first[k], again["bufs"][k]) for k in first) and mm.tally_equal(again["tally"], got["tally"])


def _noisy(rng, a):
    a = bytearray(a)
    for j in set(rng.integers(0, len(a), int(rng.integers(0, 3))).tolist()):
        a[j] = b"ACGT"[(b"ACGT".index(a[j]) + 1) % 4]
    return bytes(a)


def test_a_tally_is_added_to_and_may_be_null(ctx, mixed):
    import torch
    seqs, quals, p, want = mixed
    start = torch.arange(B.MERGE_TALLY_WORDS, dtype=torch.int64, device="cuda") * 3 + 1
    got = run(ctx, seqs, quals, 2, p, 150, tally=start.clone())
    base = B.merge_tally_dict(start.cpu().numpy())
    for k in mm.TALLY_KEYS:
        assert np.array_equal(np.asarray(got["tally"][k], np.uint64), np.asarray(base[k], np.uint64) + np.asarray(want[2][4][k], np.uint64)), k
    got = run(ctx, seqs, quals, 2, p, 150, want_tally=False)
    assert got["tally"] is None
    assert_equal(got, want[2])


def test_the_refusals_say_why(ctx):
    import torch
    L = rcorrector_amd.load_library()
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    outb = torch.full((128,), POISON, dtype=torch.uint8, device="cuda")
    off = torch.zeros(8, dtype=torch.int32, device="cuda")
    rows = torch.full((8, 4), -7, dtype=torch.int32, device="cuda")
    moff = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    tal = torch.zeros(B.MERGE_TALLY_WORDS, dtype=torch.int64, device="cuda")
    s, o, r, ms, mq, mo, t = buf.data_ptr(), off.data_ptr(), rows.data_ptr(), outb.data_ptr(), outb.data_ptr() + 64, moff.data_ptr(), tal.data_ptr()

    def dev(seq=s, qual=s, d_off=o, n=2, nbytes=4, max_len=1, mode=2, d_rows=r, d_mseq=ms, d_mqual=mq, d_moff=mo, out_cap=4, d_tally=t, null_params=False, **pk):
        p = B.merge_params(**pk)
        return L.rc_read_merge_device(ctx._h, seq, qual, d_off, n, nbytes, max_len, mode, None if null_params else ctypes.byref(p), d_rows, d_mseq, d_mqual, d_moff,
                                      out_cap, d_tally)

    assert dev() == 0                                    # one pair of two empty reads: unmerged
    ctx.sync()
    assert mm.tally_equal(B.merge_tally_dict(tal.cpu().numpy()), mm.merge_batch([b"", b""], None, 2, mm.params())[4])
    assert rows.cpu().numpy()[:2].tolist() == [[0] * 4, [-7] * 4] and moff.cpu().numpy()[:3].tolist() == [0, 1, -7]
    assert outb.cpu().numpy()[[0, 1, 64, 65]].tolist() == [0, POISON, 0, POISON]
    refused = [
        (dict(mode=0), "mode 0"), (dict(mode=-1), "mode -1"), (dict(mode=3), "mode 3"), (dict(n=3), "pairs need an even number of reads (got 3)"),
        (dict(seq=None), "null pointer"), (dict(d_off=None), "null pointer"), (dict(d_rows=None), "null pointer"), (dict(d_mseq=None), "null pointer"),
        (dict(d_moff=None), "null pointer"), (dict(null_params=True), "params must not be NULL"),
        (dict(nbytes=1 << 32, out_cap=1 << 32), "exceeds the 4 GiB batch limit"), (dict(max_len=1024), "max_read_len must be 0..1023 (got 1024)"), (dict(max_len=-1), "max_read_len"),
        (dict(min_overlap=0), "min_overlap must be 1..1023 (got 0)"), (dict(min_overlap=1024), "min_overlap must be 1..1023 (got 1024)"),
        (dict(max_mismatch_pct=-1), "max_mismatch_pct must be 0..50 (got -1)"), (dict(max_mismatch_pct=51), "max_mismatch_pct must be 0..50 (got 51)"),
        (dict(qual_base=-1), "qual_base must be 0..124 (got -1)"), (dict(qual_base=125), "qual_base must be 0..124 (got 125)"),
        (dict(qual_cap=1), "qual_cap must be 2..93 (got 1)"), (dict(qual_cap=94), "qual_cap must be 2..93 (got 94)"),
        (dict(qual_base=64, qual_cap=63), "qual_base + qual_cap must be at most 126 (got 127)"),
        (dict(qual=None), "d_mqual given without d_qual"), (dict(out_cap=3), "out_cap of 3 bytes is below the input arena's 4"),
        (dict(d_rows=r + 2), "d_rows and d_moff must lie on a 4-byte boundary"), (dict(d_moff=mo + 1), "d_rows and d_moff must lie on a 4-byte boundary"),
        (dict(d_mseq=ms + 8), "d_mseq and d_mqual on a 16-byte one"), (dict(d_mqual=mq + 1), "d_mseq and d_mqual on a 16-byte one"), (dict(d_tally=t + 4), "d_tally on an 8-byte one"),
    ]
    before = (outb.clone(), rows.clone(), moff.clone(), tal.clone())
    for kw, text in refused:
        assert dev(**kw) == RC_STATUS_ARG, kw
        err = L.rc_last_error(ctx._h).decode()
        assert err.startswith("read_merge_device: ") and text in err, (kw, err)
        if not set(kw) & {"n", "seq", "d_off", "d_rows", "d_mseq", "d_mqual", "d_moff", "d_tally"}:      # (checked whatever n_reads is)
            assert dev(**dict(kw, n=0)) == RC_STATUS_ARG, kw
    assert dev(qual=None, d_mqual=None) == 0 and dev(d_mqual=None) == 0 and dev(d_tally=None) == 0 and dev(out_cap=1 << 40) == 0
    ctx.sync()
    assert torch.equal(before[0], outb) and torch.equal(before[1], rows) and torch.equal(before[2], moff)
    with pytest.raises(rcorrector_amd.RcorrectorError, match="qual_cap must be 2..93"):
        ctx.read_merge_device(buf, None, off, 2, 4, 1, 2, B.merge_params(qual_cap=1), rows, outb, None, moff, 4)


def test_the_merge_the_pair_cut_and_the_overlap_report_choose_the_same_offset(ctx, mixed):
    """one arena given to all three: every merged pair's d and min(La, F) are read_trim's pair cuts, the merged pairs are the
    report's overlapping ones, and the histogram of merged_len is the report's fragment histogram"""
    import torch
    seqs, _, p, want = mixed
    got = run(ctx, seqs, None, 2, p, 150)
    arena, off = rcorrector_amd.pack_reads(seqs)
    t_seq, t_off = torch.from_numpy(arena).cuda(), torch.from_numpy(off.astype(np.int32)).cuda()
    d_out = torch.full((len(seqs), 4), -7, dtype=torch.int32, device="cuda")
    counts = torch.zeros(B.OVERLAP_WORDS, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.read_trim_device(t_seq, None, t_off, len(seqs), arena.size, 150, 2, B.trim_params(qual_min=0, adapter1=b"", min_len=0), d_out)
    ctx.mate_overlap_device(t_seq, t_seq, t_off, len(seqs), arena.size, 150, 2, counts)
    ctx.sync()
    trim, rep = d_out.cpu().numpy(), B.mate_overlap_dict(counts.cpu().numpy())
    rows = got["rows"]
    La, Lb = np.array([len(s) for s in seqs[0::2]]), np.array([len(s) for s in seqs[1::2]])
    merged = rows[:, 0] > 0
    assert np.array_equal(rows[:, 0], want[2][0][:, 0]) and 10 < merged.sum() < 40
    assert np.array_equal(trim[0::2, 3], np.where(merged, np.minimum(La, rows[:, 0]), La))
    assert np.array_equal(trim[1::2, 3], np.where(merged, np.minimum(Lb, Lb + rows[:, 1]), Lb))
    assert rep["overlapping"] == got["tally"]["merged"] == merged.sum() and rep["pairs"] == got["tally"]["pairs"] == 40
    assert rep["compared_before"] == got["tally"]["compared"] and rep["disagree_before"] == got["tally"]["mismatches"] > 0
    hist = got["tally"]["len_hist"].astype(np.int64)
    assert hist[0] == 40 - merged.sum() and np.array_equal(hist[1:], rep["frag"][1:].astype(np.int64)) and rep["frag"][0] == 0


def test_the_merged_arena_goes_to_read_depth_device_as_it_is():
    """a table counted from the fragments; the arena the merge left in HBM, mode 0, against the same strings uploaded from the
    host (a read longer than 1023 bases among them: read_depth_device takes it as no read, on either way in)"""
    import torch
    from test_read_depth import device_depth, table_of
    from seam_arena import canonical
    k = 23
    rng = np.random.default_rng(12)
    pairs = [tc.pair_of(rng, int(F), 150, 150) for F in rng.integers(100, 280, 30)] + [tc.pair_of(rng, 1500, 1000, 1000), (tc.rand_seq(rng, 80), tc.rand_seq(rng, 80))]
    seqs = [_noisy(rng, m) for pr in pairs for m in pr]
    quals = [tc.rand_qual(rng, len(s), 2, 41) for s in seqs]
    counts = {}
    for a, _ in pairs:
        for i in range(0, len(a) - k + 1):
            code = canonical(a[i:i + k])
            counts[code] = counts.get(code, 0) + 1 + i % 7
    ctx = rcorrector_amd.Context(k=k, device=0)
    try:
        table_of(ctx, counts)
        p = mm.params()
        want = mm.merge_batch(seqs, quals, 2, p)
        got = run(ctx, seqs, quals, 2, p, 1000)
        assert_equal(got, want)
        units = len(pairs)
        merged_strings = [want[2][want[1][u]:want[1][u + 1] - 1] for u in range(units)]
        assert max(len(s) for s in merged_strings) == 1500 and merged_strings[-1] == b"" and sum(1 for s in merged_strings if s) > 25
        d_out = torch.full((units, 4), -7, dtype=torch.int32, device="cuda")
        ctx.read_depth_device(got["bufs"]["mseq"], got["bufs"]["moff"], units, int(want[1][units]), 1023, d_out)
        ctx.sync()
        on_the_spot = d_out.cpu().numpy()
        arena, off = rcorrector_amd.pack_reads(merged_strings)
        assert arena.tobytes() == want[2] and np.array_equal(off.astype(np.uint32), want[1])
        uploaded = device_depth(ctx, arena, off, lead=0, max_len=1023)
        # (not an empty comparison: most units merge, and the table holds mate 1's 128 windows -- over half of a merged read's
        # unless the fragment has 278 bases or more or a substitution took too many of them)
        assert np.array_equal(on_the_spot, uploaded) and (on_the_spot[:, 0] > 0).sum() > 25 and (on_the_spot[:, 2] > 0).sum() > units // 2
        assert on_the_spot[-1].tolist() == [0, 0, 0, 0] == on_the_spot[-2].tolist() and len(merged_strings[-2]) == 1500
    finally:
        ctx.close()


def test_an_input_arena_across_byte_2_to_the_31(ctx):
    """tests/high_arena.py's trimming batch, interleaved pairs, placed so that a mate's bases lie on both sides of byte 2^31 and
    so that a mate starts at it exactly; the merged arena is small and starts at byte 0 of its own buffer"""
    import torch
    reads, quals, tp = ha.trim_case()
    p = mm.params(min_overlap=tp["pair_min_overlap"])
    want = mm.merge_batch(reads, None, 2, p)
    assert want[4]["merged"] >= 9 and want[0][3].tolist()[:2] == [130, 50]           # (reads 6 and 7: a fragment of 130 bases, 100 and 80 deep)
    buf = ha.allocate()
    n, units = len(reads), len(reads) // 2
    out_cap = ha.MID_NBYTES
    mseq = torch.empty((out_cap,), dtype=torch.uint8, device="cuda")
    total = int(want[1][units])
    for kind, i in ha.TRIM_MID:
        w = (ha.mid_seam if kind == "seam" else ha.mid_straddle)(reads, i)
        for lead in ha.MID_LEADS:
            ps, t_off = ha.put(buf, lead, w), ha.off_tensor(w)
            mseq[:total + 4096] = POISON
            rows = torch.full((units, 4), -7, dtype=torch.int32, device="cuda")
            moff = torch.full((units + 1,), -7, dtype=torch.int32, device="cuda")
            tal = torch.zeros(B.MERGE_TALLY_WORDS, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ctx.read_merge_device(ps, None, t_off, n, w["nbytes"], 1023, 2, params_of(p), rows, mseq, None, moff, out_cap, tal)
            ctx.sync()
            got = {"rows": rows.cpu().numpy(), "moff": moff.cpu().numpy().view(np.uint32), "mseq": mseq[:total].cpu().numpy().tobytes(), "mqual": None,
                   "tally": B.merge_tally_dict(tal.cpu().numpy())}
            assert_equal(got, want, "%s %d lead %d" % (kind, i, lead))
            assert bool((mseq[total:total + 4096] == POISON).all())
