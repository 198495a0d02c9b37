"""GPU: the correction report -- rc_change_report_begin / get / end and the binding's change_report_* methods: what the
correction changed, by position from either end, substitution, quality class, mate and read.

Expected values come from a numpy model in this file.  It takes the uncorrected arena, the offsets, the mode, the quality
bytes with the bad-quality character, and the corrected arena and `ret` that the ORACLE gives for the same input
(oracle.correct_batch) -- never the library's own output.  Every comparison is exact integer equality.

Does `changes` equal the rc_summary delta?  rc_summary adds up the positive `ret` values (UpdateSummary, main.cpp:73-79).  On
the oracle's own outputs for every data set used here the number of bytes that differ equals sum(ret[ret > 0]) (checked on
the CPU: se_k23 1 190, pe_k23 1 311, il_k23 1 260, tiers_se 2 737, tiers_pe and tiers_il 5 599, edge 109, nrich 2 024,
pe_var 1 565 on both sides), so the test asserts it -- after asserting that the oracle's outputs satisfy it for the case at hand.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import datasets
import rcorrector_amd
from rcorrector_amd.binding import REPORT_MAX_LEN as MAX_LEN, REPORT_MAX_PER_READ as MAX_PER_READ

pytestmark = pytest.mark.gpu
BAD_Q = b"H"
SHAPES = {"reads": (2,), "reads_changed": (2,), "reads_unfixable": (2,), "changes": (2,), "len_hist": (2, MAX_LEN), "by_pos5": (2, MAX_LEN),
          "by_pos3": (2, MAX_LEN), "subst": (5, 4), "by_qual": (3,), "per_read": (MAX_PER_READ + 1,)}
_FROM = np.full(256, 4, dtype=np.int64)   # upper case only: the kernels read a lower-case letter as a letter outside ACGT
for _i, _c in enumerate(b"ACGT"):
    _FROM[_c] = _i


def zero_report():
    return {name: np.zeros(shape, dtype=np.uint64) for name, shape in SHAPES.items()}


def add_reports(a, b):
    return {name: a[name] + b[name] for name in SHAPES}


def model(orig, corr, off, ret, qual, mate_of, bad_q=BAD_Q):
    """the report of one arena: orig / corr uint8 arrays before / after correction, off its n + 1 offsets, ret the oracle's
    return values of its reads, qual its quality bytes (None: a batch without qualities), mate_of(r) the mate of read r"""
    R = zero_report()
    bq = np.frombuffer(bad_q, dtype=np.int8)[0]
    for r in range(len(off) - 1):
        o, e = int(off[r]), int(off[r + 1]) - 1
        length, mate = e - o, mate_of(r)
        R["reads"][mate] += 1
        R["len_hist"][mate][min(length, MAX_LEN - 1)] += 1
        R["reads_unfixable"][mate] += int(ret[r] == -1)
        d = np.nonzero(orig[o:e] != corr[o:e])[0]
        R["per_read"][min(len(d), MAX_PER_READ)] += 1
        if len(d) == 0:
            continue
        R["reads_changed"][mate] += 1
        R["changes"][mate] += len(d)
        for p in d.tolist():
            R["by_pos5"][mate][min(p, MAX_LEN - 1)] += 1
            R["by_pos3"][mate][min(length - 1 - p, MAX_LEN - 1)] += 1
            to = int(_FROM[corr[o + p]])
            assert to < 4          # a correction writes one of ACGT
            R["subst"][int(_FROM[orig[o + p]])][to] += 1
            if qual is None or qual[o] == 0:
                R["by_qual"][2] += 1
            else:
                R["by_qual"][0 if qual[o + p].view(np.int8) <= bq else 1] += 1
    return R


def consistent(R):
    total = int(R["changes"].sum())
    assert int(R["by_pos5"].sum()) == int(R["by_pos3"].sum()) == int(R["subst"].sum()) == int(R["by_qual"].sum()) == total
    assert int(R["per_read"].sum()) == int(R["len_hist"].sum()) == int(R["reads"].sum())
    assert np.array_equal(R["len_hist"].sum(axis=1), R["reads"])
    assert int(R["per_read"][1:].sum()) == int(R["reads_changed"].sum())
    return total


def assert_report(got, want, what=""):
    for name, shape in SHAPES.items():
        assert got[name].dtype == np.uint64 and got[name].shape == shape, name
        assert np.array_equal(got[name], want[name]), "%s: %s differs at %s: got %s, want %s" % (
            what, name, np.argwhere(got[name] != want[name])[:6].tolist(), got[name][got[name] != want[name]][:6], want[name][got[name] != want[name]][:6])
    consistent(got)


@functools.lru_cache(maxsize=None)
def _dataset(name):
    return datasets.make(name)


def arenas_of(po, d, fasta=False):
    """[(arena, qualities or None, offsets)] of the data set's one or two arenas, uncorrected"""
    out = []
    for s, q in ((d["seqs1"], d["quals1"]), (d["seqs2"], d["quals2"])):
        if s is None:
            continue
        a, off = po.pack_reads(s)
        out.append((a, None if fasta else po.pack_reads(q)[0], off))
    return out


_EXPECTED = {}


def expected(po, name, fasta=False):
    """(the model's report of the whole data set from the oracle's outputs, sum of the oracle's positive ret values)"""
    key = (name, fasta)
    if key not in _EXPECTED:
        d = _dataset(name)
        T = po.Table(d["k"], len(d["keys"]))
        T.put_many(d["keys"], d["counts"])
        P = po.make_params(d["k"], d["mfk"], d["rate"], d.get("badq", BAD_Q))
        ar = arenas_of(po, d, fasta)
        corr = [a.copy() for a, _, _ in ar]
        quals = [np.zeros_like(a) if q is None else q for a, q, _ in ar]   # (no qualities: the reference sees qual[0] == 0)
        if d["mode"] == 1:
            ret = po.correct_batch(P, T, 1, corr[0], quals[0], ar[0][2], corr[1], quals[1], ar[1][2], threads=4)[0]
        else:
            ret = po.correct_batch(P, T, d["mode"], corr[0], quals[0], ar[0][2], threads=4)[0]
        n = len(ar[0][2]) - 1
        R = zero_report()
        for i, (a, q, off) in enumerate(ar):
            mate_of = (lambda r: r & 1) if d["mode"] == 2 else (lambda r, i=i: i)
            R = add_reports(R, model(a, corr[i], off, ret[i * n:(i + 1) * n], q, mate_of, d.get("badq", BAD_Q)))
        assert consistent(R) > 0, "%s: the oracle changes nothing, the case would pass vacuously" % name
        _EXPECTED[key] = (R, int(ret[ret > 0].sum()))
    return _EXPECTED[key]


def new_ctx(d, qbits=False):
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    ctx.table_build(d["keys"], d["counts"])
    ctx.set_run_params(d["rate"], d.get("badq", BAD_Q))
    if qbits:
        ctx.set_quality_bits(True)
    return ctx


def unit_cuts(d, nb):
    """read index ranges of nb batches (mates travel together)"""
    step = 2 if d["mode"] == 2 else 1
    units = len(d["seqs1"]) // step
    c = (np.linspace(0, units, nb + 1).astype(np.int64) * step).tolist()
    return [(lo, hi) for lo, hi in zip(c[:-1], c[1:]) if hi > lo]


def batch_of(po, ctx, d, lo, hi, qbits=False, fasta=False):
    """host-batch arguments (seq, qual, off[, seq2, qual2, off2]) of reads [lo, hi): qualities as bytes, as zeros (fasta) or,
    with qbits, as one bit array per arena"""
    out = []
    for s, q in ((d["seqs1"], d["quals1"]), (d["seqs2"], d["quals2"])):
        if s is None:
            continue
        a, off = po.pack_reads(s[lo:hi])
        qa = np.zeros_like(a) if fasta else po.pack_reads(q[lo:hi])[0]
        if qbits:
            qa = ctx.pack_quality_bits(qa, d.get("badq", BAD_Q))
        out += [a, qa, off]
    return out


def one_arena(po, d, lo, hi, fasta=False):
    """(arena, quality bytes, offsets, bytes of the first mates' arena) of reads [lo, hi) as ONE arena (mode 1: first mates, then second mates)"""
    b = batch_of(po, None, d, lo, hi, fasta=fasta)
    if d["mode"] != 1:
        return b[0], b[1], b[2], b[0].size
    off = np.concatenate([b[2], (b[5][1:].astype(np.int64) + b[0].size).astype(np.uint32)])
    return np.concatenate([b[0], b[3]]), np.concatenate([b[1], b[4]]), off, b[0].size


# ---- the transports: each corrects d in nb batches on ctx (report armed by the caller) ---------------------------------------
def via_correct_batch(po, ctx, d, nb, qbits=False, fasta=False):
    for lo, hi in unit_cuts(d, nb):
        ctx.correct_batch(d["mode"], *batch_of(po, ctx, d, lo, hi, qbits, fasta))


class _Trace(C.Structure):   # rc_trace (rcorrector_amd.h)
    _fields_ = [("max_iter", C.c_int32), ("counts_before", C.c_void_p), ("counts_after", C.c_void_p), ("flags", C.c_void_p), ("n_iter", C.c_void_p),
                ("iter", C.c_void_p)]


def via_traced(po, ctx, d, nb, qbits=False, fasta=False):
    """rc_correct_batch_traced (what `rcorrector -verbose` runs): the binding has no method for it, so through the C ABI"""
    L = rcorrector_amd.load_library()
    max_iter, words = 4, 36   # RC_TRACE_ITER_WORDS
    for lo, hi in unit_cuts(d, nb):
        args = batch_of(po, ctx, d, lo, hi, qbits, fasta)
        b, res, keep = ctx._batch(d["mode"], *(args + [None] * (6 - len(args))))
        nbytes = sum(a.size for a in args[0::3])
        reads = len(res[0])
        bufs = [np.zeros(nbytes, np.int32), np.zeros(nbytes, np.int32), np.zeros(reads, np.int32), np.zeros(reads, np.int32),
                np.zeros(reads * max_iter * words, np.int32)]
        t = _Trace(max_iter, *[x.ctypes.data for x in bufs])
        rc = L.rc_correct_batch_traced(C.c_void_p(ctx._h), C.byref(b), C.byref(t))
        assert rc == 0, rc


def via_slots(po, ctx, d, nb, qbits=False, fasta=False, lanes=True):
    """rc_submit / rc_wait, four slots in flight (with lanes, slots 1..3 run in contexts of their own)"""
    ctx.set_slot_lanes(lanes)
    busy = {}
    for i, (lo, hi) in enumerate(unit_cuts(d, nb)):
        s = i % 4
        if s in busy:
            ctx.wait(s)
        busy[s] = batch_of(po, ctx, d, lo, hi, qbits, fasta)
        ctx.submit(s, d["mode"], *busy[s])
    for s in sorted(busy, reverse=True):
        ctx.wait(s)


def via_slots_lanes_off(po, ctx, d, nb, qbits=False, fasta=False):
    via_slots(po, ctx, d, nb, qbits, fasta, lanes=False)


def submit_packed(po, ctx, d, lo, hi, slot, fasta=False, fix_cap=None):
    a, qa, off, _ = one_arena(po, d, lo, hi, fasta)
    arena = ctx.host_array(a.size)
    arena[:] = a
    bases, exc_pos, exc_chr = ctx.pack_bases(arena, bases=ctx.host_array((a.size + 15) // 16, np.uint32))
    qb = None
    if not fasta:
        qb = ctx.host_array((a.size + 7) // 8)
        ctx.pack_quality_bits(qa, d.get("badq", BAD_Q), out=qb)
    ctx.submit_packed(slot, d["mode"], a.size, off, bases, qb, exc_pos, exc_chr, fix_cap=fix_cap)
    return arena, bases, exc_pos, exc_chr, qb, off


def via_packed(po, ctx, d, nb, qbits=False, fasta=False):
    busy = {}
    for i, (lo, hi) in enumerate(unit_cuts(d, nb)):
        s = i % 4
        if s in busy:
            ctx.wait_packed(s)
        busy[s] = submit_packed(po, ctx, d, lo, hi, s, fasta)
    for s in sorted(busy):
        ctx.wait_packed(s)


def keep_arenas(po, ctx, d):
    """the data set's arenas counted and kept in HBM, the table then replaced by the data set's own"""
    ar = arenas_of(po, d)
    ctx.count_keep(True)
    ctx.count_begin()
    for a, _, _ in ar:
        ctx.count_add(a)
    ctx.count_finish(2)
    ctx.table_build(d["keys"], d["counts"])
    ctx.set_run_params(d["rate"], d.get("badq", BAD_Q))
    return ar


def submit_resident(ctx, d, ar, lo, hi, slot, fasta=False, fix_cap=None):
    a1, q1, off1 = ar[0]
    b1 = int(off1[hi] - off1[lo])
    off = [off1[lo:hi + 1].astype(np.int64) - int(off1[lo])]
    qs = [q1[off1[lo]:off1[hi]]] if not fasta else []
    args = dict(arena_a=0, begin_a=int(off1[lo]), bytes_a=b1)
    if d["mode"] == 1:
        a2, q2, off2 = ar[1]
        off.append(off2[lo + 1:hi + 1].astype(np.int64) - int(off2[lo]) + b1)
        if not fasta:
            qs.append(q2[off2[lo]:off2[hi]])
        args.update(arena_b=1, begin_b=int(off2[lo]), bytes_b=int(off2[hi] - off2[lo]))
    qb = None
    if not fasta:
        qb = ctx.host_array((b1 + args.get("bytes_b", 0) + 7) // 8)
        ctx.pack_quality_bits(np.concatenate(qs), d.get("badq", BAD_Q), out=qb)
    ctx.submit_resident(slot, d["mode"], np.concatenate(off).astype(np.uint32), qb, fix_cap=fix_cap, **args)
    return qb


def via_resident(po, ctx, d, nb, qbits=False, fasta=False):
    """the reads are the arenas the counter kept; every batch a byte range of them (ctx: a context of its own)"""
    ar = keep_arenas(po, ctx, d)
    keep = []   # (only keeps the page-locked quality bits of every batch alive until the end)
    for i, (lo, hi) in enumerate(unit_cuts(d, nb)):
        keep.append(submit_resident(ctx, d, ar, lo, hi, i % 2, fasta))
        ctx.wait_resident(i % 2)


def via_device(po, ctx, d, nb, qbits=False, fasta=False):
    """rc_correct_device on the caller's memory, at an address that is no multiple of 16"""
    import torch
    keep = []   # (only keeps the tensors of every batch alive until the sync below: rc_correct_device is asynchronous)
    for lo, hi in unit_cuts(d, nb):
        a, qa, off, _ = one_arena(po, d, lo, hi, fasta)
        if qbits:
            qa = ctx.pack_quality_bits(qa, d.get("badq", BAD_Q))
        n = len(off) - 1
        t_buf = torch.zeros(a.size + 64, dtype=torch.uint8, device="cuda")
        t_seq = t_buf[5:5 + a.size]
        t_seq.copy_(torch.from_numpy(a))
        assert t_seq.data_ptr() % 16 != 0
        t_q = torch.from_numpy(qa.copy()).cuda()
        t_off = torch.from_numpy(off.astype(np.int32)).cuda()
        res = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(4)]
        max_len = int(np.diff(off.astype(np.int64)).max()) - 1
        ctx.correct_device(d["mode"], n, a.size, max_len, t_seq, t_q, t_off, *res)
        keep.append((t_buf, t_q, t_off, res))
    ctx.sync()


def via_correct_read(po, ctx, d, nb, qbits=False, fasta=False):
    """ErrorCorrection read by read (single-end data: a read without a mate is corrected with pair threshold -1)"""
    assert d["mode"] == 0
    for s, q in zip(d["seqs1"], d["quals1"]):
        ctx.correct_read(s, None if fasta else q)


TRANSPORTS = {"correct_batch": via_correct_batch, "slots": via_slots, "slots_lanes_off": via_slots_lanes_off, "packed": via_packed,
              "resident": via_resident, "device": via_device}
# modes 0, 1 and 2; tiers_*: reads beyond 160 and 320 bases; edge: the adversarial reads (letters outside ACGT: the N row of
# subst); pe_var / nrich: N-rich, variable lengths
# qv_mixed_pe/straddle: qualities either side of and on the threshold, fixes on both kinds of base (tests/datasets.py: qv_)
QV = "qv_mixed_pe/straddle"
NAMES = ["se_k23", "pe_k23", "il_k23", "tiers_se", "tiers_pe", "tiers_il", "edge", "nrich", "pe_var", QV]


def run_case(oracle, name, tname, nb, qbits=False, fasta=False):
    d = _dataset(name)
    want, cor = expected(oracle, name, fasta)
    ctx = new_ctx(d, qbits)
    ctx.change_report_begin()
    reads0, cor0 = ctx.summary()
    (TRANSPORTS.get(tname) or {"traced": via_traced}.get(tname) or via_correct_read)(oracle, ctx, d, nb, qbits, fasta)
    got = ctx.change_report()
    what = "%s through %s in %d batches%s%s" % (name, tname, nb, ", quality bits" if qbits else "", ", no qualities" if fasta else "")
    assert_report(got, want, what)
    reads1, cor1 = ctx.summary()
    assert reads1 - reads0 == int(want["reads"].sum())
    assert int(want["changes"].sum()) == cor       # the oracle's own outputs: bytes that differ = sum of the positive ret values
    assert cor1 - cor0 == int(got["changes"].sum())
    assert_report(ctx.change_report(), want, what + " (read twice)")
    ctx.change_report_end()
    ctx.close()
    return want


# ---- 1. every transport against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", sorted(TRANSPORTS))
@pytest.mark.parametrize("name", NAMES)
def test_report_equals_the_model_on_the_oracles_output(oracle, name, tname):
    want = run_case(oracle, name, tname, 5)
    if name == "edge":
        assert int(want["subst"][4].sum()) > 0 and int(want["len_hist"][0][:23].sum()) > 0   # a letter outside ACGT was replaced; reads shorter than k
    if name.startswith("tiers"):
        assert int(want["len_hist"][:, 161:321].sum()) > 0 and int(want["len_hist"][:, 321:].sum()) > 0
        assert int(want["by_pos5"][:, 160:].sum()) > 0
    if name == QV:
        assert want["by_qual"][0] >= 50 and want["by_qual"][1] >= 50 and want["by_qual"][2] == 0
    if name in ("pe_k23", "il_k23", "tiers_pe", "tiers_il", "pe_var", QV):
        assert want["reads"][0] == want["reads"][1] > 0 and want["changes"][1] > 0
    else:
        assert want["reads"][1] == 0 and int(want["by_pos5"][1].sum()) == 0


@pytest.mark.parametrize("name", ["se_k23", "pe_k23", "il_k23", "edge"])
def test_report_of_batches_through_the_traced_entry_point(oracle, name):
    """rc_correct_batch_traced reaches the report through the public rc_correct_device it calls: pinned here"""
    run_case(oracle, name, "traced", 3)


@pytest.mark.parametrize("name", ["se_k23", "edge"])
def test_report_of_reads_corrected_one_by_one(oracle, name):
    run_case(oracle, name, "correct_read", 1)


# ---- 2. the shapes quality arrives in ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", ["correct_batch", "slots", "device"])
@pytest.mark.parametrize("name", ["se_k23", "pe_k23", "il_k23", "tiers_pe", "pe_var", "edge", QV])
def test_quality_bits_give_the_same_report(oracle, name, tname):
    """rc_set_quality_bits: the byte entry points take bit arrays; a paired host batch has its second arena's bits apart
    (qual_split / qual_base2).  (tiers_pe: every change is on a low-quality base.)"""
    want = run_case(oracle, name, tname, 3, qbits=True)
    assert want["by_qual"][0] > 0 and (want["by_qual"][1] > 0 or name == "tiers_pe") and want["by_qual"][2] == 0
    if name == QV:
        assert want["by_qual"][0] >= 50 and want["by_qual"][1] >= 50


@pytest.mark.parametrize("tname", ["correct_batch", "packed", "resident", "device", "correct_read"])
def test_a_batch_without_qualities_counts_as_none(oracle, tname):
    want = run_case(oracle, "se_k23", tname, 2, fasta=True)
    assert want["by_qual"][2] == want["changes"].sum() > 0 and want["by_qual"][0] == want["by_qual"][1] == 0


def test_a_paired_batch_without_qualities(oracle):
    run_case(oracle, "pe_k23", "packed", 2, fasta=True)
    run_case(oracle, "pe_k23", "slots", 2, fasta=True)


@pytest.mark.parametrize("tname", ["correct_batch", "packed", "resident", "device"])
def test_the_reads_on_which_qualities_decide_without_their_qualities(oracle, tname):
    """qv_mixed_pe/fasta, the twin of QV: the same reads with no qualities, on which the pairwise veto is never skipped"""
    want = run_case(oracle, QV, tname, 2, fasta=True)
    assert want["by_qual"][2] == want["changes"].sum() >= 50 and want["by_qual"][0] == want["by_qual"][1] == 0


# ---- 3. behaviour --------------------------------------------------------------------------------------------------------------------
def test_report_is_cumulative_and_get_leaves_it_armed(oracle):
    d = _dataset("pe_k23")
    want = expected(oracle, "pe_k23")[0]
    ctx = new_ctx(d)
    ctx.change_report_begin()
    via_correct_batch(oracle, ctx, d, 3)
    assert_report(ctx.change_report(), want, "first pass")
    assert_report(ctx.change_report(), want, "read again")
    via_slots(oracle, ctx, d, 4)
    twice = {name: want[name] * np.uint64(2) for name in SHAPES}
    assert_report(ctx.change_report(), twice, "two passes")
    # end and begin: a fresh report
    ctx.change_report_end()
    ctx.change_report_begin()
    via_packed(oracle, ctx, d, 2)
    assert_report(ctx.change_report(), want, "after end + begin")
    ctx.close()


@pytest.mark.parametrize("tname", ["packed", "resident"])
def test_a_batch_that_did_not_fit_its_fix_list_counts_once(oracle, tname):
    RC_STATUS_NOSPACE = -6
    d = _dataset("pe_k23")
    want = expected(oracle, "pe_k23")[0]
    n = len(d["seqs1"])
    ctx = new_ctx(d)
    ar = keep_arenas(oracle, ctx, d) if tname == "resident" else None
    ctx.change_report_begin()

    def go(cap):
        if tname == "packed":
            keep = submit_packed(oracle, ctx, d, 0, n, 0, fix_cap=cap)
            return keep, ctx.wait_packed(0)
        keep = submit_resident(ctx, d, ar, 0, n, 0, fix_cap=cap)
        return keep, ctx.wait_resident(0)

    with pytest.raises(rcorrector_amd.RcorrectorError) as e:
        go(3)
    assert "fix_cap" in str(e.value)
    assert consistent(ctx.change_report()) == 0      # the refused batch is not in the report ...
    assert int(ctx.change_report()["reads"].sum()) == 0
    _, res = go(None)
    assert len(res[4]) == int(want["changes"].sum())
    assert_report(ctx.change_report(), want, "%s: resubmitted with room" % tname)   # ... and its resubmission is, once
    ctx.close()


def test_a_batch_on_a_lane_slot_lands_in_the_parents_report(oracle):
    d = _dataset("il_k23")
    want = expected(oracle, "il_k23")[0]
    ctx = new_ctx(d)
    ctx.set_slot_lanes(True)
    ctx.change_report_begin()
    n = len(d["seqs1"])
    for slot in (3, 1):
        b = batch_of(oracle, ctx, d, 0, n)
        ctx.submit(slot, d["mode"], *b)
        ctx.wait(slot)
    assert_report(ctx.change_report(), {name: want[name] * np.uint64(2) for name in SHAPES}, "slots 3 and 1")
    ctx.close()


def test_state_errors_and_an_empty_batch(oracle):
    RC_STATUS_STATE = -4
    d = _dataset("se_k23")
    L = rcorrector_amd.load_library()
    ctx = rcorrector_amd.Context(k=d["k"], device=0)
    h = ctx._h
    rep = rcorrector_amd.binding._ChangeReport()
    assert L.rc_change_report_get(h, C.byref(rep)) == RC_STATUS_STATE
    assert L.rc_change_report_end(h) == RC_STATUS_STATE
    assert L.rc_change_report_begin(h) == 0            # (needs no table)
    assert L.rc_change_report_begin(h) == RC_STATUS_STATE
    assert L.rc_change_report_get(h, C.byref(rep)) == 0
    assert L.rc_change_report_end(h) == 0
    assert L.rc_change_report_end(h) == RC_STATUS_STATE
    assert L.rc_change_report_get(h, C.byref(rep)) == RC_STATUS_STATE
    ctx.table_build(d["keys"], d["counts"])
    ctx.set_run_params(d["rate"], d.get("badq", BAD_Q))
    ctx.change_report_begin()
    empty, off0 = np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    ctx.correct_batch(0, empty, empty, off0)
    ctx.submit(1, 0, empty, empty, off0)
    ctx.wait(1)
    got = ctx.change_report()
    assert all(int(got[name].sum()) == 0 for name in SHAPES)
    ctx.close()      # (armed: rc_destroy releases the report)


def test_armed_or_not_the_results_are_the_same(oracle):
    d = _dataset("pe_k23")
    n = len(d["seqs1"])

    def run(armed):
        ctx = new_ctx(d)
        if armed:
            ctx.change_report_begin()
        out = []
        b = batch_of(oracle, ctx, d, 0, n)
        out += [x.copy() for x in ctx.correct_batch(d["mode"], *b)] + [b[0].copy(), b[3].copy()]
        keep, res = submit_packed(oracle, ctx, d, 0, n, 1), None
        res = ctx.wait_packed(1)
        out += [x.copy() for x in res[:4]] + [np.array(sorted(zip(res[4].tolist(), res[5].tolist())))]
        out += [np.array(ctx.summary()), np.array([ctx.table_digest()])]
        ctx.close()
        return out

    for x, y in zip(run(False), run(True)):
        assert np.array_equal(x, y)
