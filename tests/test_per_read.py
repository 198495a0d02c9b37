"""The three per-read entry points -- rc_strong_threshold_read, rc_correct_read, rc_kmer_info_read: ErrorCorrection.h:26-28 at
the reference's own granularity -- against the oracle's three functions, read by read.  Every comparison is exact.

They are a kernel path of their own, not wrappers of the batch (rc_api_batch.hip):
  * rc_correct_read runs no threshold kernel: k_correct computes the read's threshold itself (fused_front_end = 1, rc_front_end
    inside the kernel), which a batch reaches only under RC_K2_WAVE_PER_READ or -verbose, i.e. on the 192 class or the TRACE
    build.  Here the plain 192 / 320 / 1024 instances, the instances compiled for k = 23 and 25 and a table with extension bits
    run it (b, c);
  * pair_strong_threshold reaches the kernel as rc_kernel_args::pair_override from this call alone (d, e);
  * the launch has no work list, a grid of one and max_len = the read's length;
  * one_read_upload has rules of its own for the quality string and for what it refuses (f, g);
  * the calls share the context's buffers and flags with the batch calls (h).
tests/test_hostsim.py runs the pair_t sweep of (d) on the lane-serial build of the same control flow."""
import ctypes as C

import numpy as np
import pytest

import datasets
import synth
from test_hostsim import check_pair_sweep_is_not_vacuous, oracle_pair_sweep, oracle_read, oracle_setup

pytestmark = pytest.mark.gpu

RC_ERR_ARG, RC_ERR_STATE = -1, -4   # rc_internal.h


def _ctx(d):
    import rcorrector_amd
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    ctx.table_build(d["keys"], d["counts"])
    ctx.set_run_params(d["rate"], d.get("badq", b"H"))
    return ctx


def _three_calls(oracle, ctx, P, T, seq, qual, what, pair_t=-1):
    """The three comparisons of one read: its threshold, its correction (return value and bases), the k-mer information of the
    read as given and as corrected.  Returns the oracle's (ret, bases, l, m, h)."""
    want = oracle_read(oracle, P, T, seq, qual, pair_t)
    assert ctx.strong_threshold_read(seq) == oracle.strong_threshold(P, T, seq), "%s: strong threshold" % what
    got = ctx.correct_read(seq, qual, pair_t)
    assert got == want[:2], "%s: (ret, bases) %r, the oracle's %r" % (what, got, want[:2])
    assert ctx.kmer_info_read(seq) == oracle.kmer_information(P, T, seq), "%s: l/m/h of the read as given" % what
    assert ctx.kmer_info_read(got[1]) == want[2:], "%s: l/m/h of the corrected read" % what
    return want


# ---- a. the three calls, read by read ------------------------------------------------------------------------------------------
# reads run per data set: 200, or as many as it takes to meet every return value (> 0, 0, -1) among them
N_READS = {"se_k23": 200, "skew": 200, "nrich": 200, "varlen": 200, "k15": 200, "k11": 200, "k32": 200, "k31_mc8": 200, "polya_k23": 200,
           "edge": None, "max1023": None}


@pytest.mark.parametrize("name", list(N_READS))
def test_three_calls_equal_the_oracle_read_by_read(oracle, name):
    d = datasets.make(name)
    n = N_READS[name] or len(d["seqs1"])
    T, P = oracle_setup(oracle, d)
    batch = datasets.run_oracle(oracle, d)   # the whole set as one mode-0 batch: what the rest of the suite rests on
    corrected = oracle.unpack_reads(batch[4], oracle.pack_reads(d["seqs1"])[1])
    ctx = _ctx(d)
    rets = []
    for i in range(n):
        want = _three_calls(oracle, ctx, P, T, d["seqs1"][i], d["quals1"][i], "%s read %d" % (name, i))
        assert want == (batch[0][i], corrected[i], batch[1][i], batch[2][i], batch[3][i]), "%s read %d: per read and as a batch differ" % (name, i)
        rets.append(want[0])
    ctx.close()
    rets = np.array(rets)
    seen = (int((rets > 0).sum()), int((rets == 0).sum()), int((rets == -1).sum()))
    if name in ("max1023", "k11"):
        # the oracle returns -1 for none of max1023's 80 reads and for none of k11's 1 500: taking more reads cannot help, and the
        # other nine sets have that case
        assert seen[0] > 0 and seen[1] > 0, "%s: reads with ret > 0 / 0 / -1: %s" % (name, seen)
    elif name != "edge":
        assert min(seen) > 0, "%s: reads with ret > 0 / 0 / -1 among the first %d: %s" % (name, n, seen)


# ---- b. the capacity classes of k_correct with the front end inside ----------------------------------------------------------

def _uncut_max1023():
    """max1023's reads at their full 1 023 bases (the data set itself cuts each to a length of its own) over the exact counts
    of their k-mers"""
    c = datasets.CONFIGS["max1023"]
    kw = dict(c["kw"], var_len=False)
    s1, q1, _, _, _ = synth.make_reads(kw.pop("seed"), kw.pop("n"), kw.pop("length"), **kw)
    keys, cnt = synth.count_kmers([s1, None], c["k"])
    return dict(k=c["k"], mfk=c["mfk"], rate=c["rate"], mode=0, keys=keys, counts=cnt, seqs1=[r.tobytes() for r in s1],
                quals1=[q.tobytes() for q in q1], seqs2=None, quals2=None)


def _long600_mates():
    d = datasets.make("long600_k31")
    return dict(d, mode=0, seqs1=d["seqs1"] + d["seqs2"], quals1=d["quals1"] + d["quals2"], seqs2=None, quals2=None)


# lengths either side of fill_args' 192 / 320 / 1024 classes (capacity = length + 1 rounded up to 64: 191 -> 192, 192 -> 256)
@pytest.mark.parametrize("source,lengths", [(_uncut_max1023, [191, 192, 193, 319, 320, 321, 640, 1023]), (_long600_mates, [193, 321, 600])],
                         ids=["max1023", "long600_k31"])
def test_capacity_classes_with_the_front_end_inside(oracle, source, lengths):
    d = source()
    T, P = oracle_setup(oracle, d)
    ctx = _ctx(d)
    for length in lengths:
        # reads that carry a substitution within the cut (tools/synth.py gives a substituted base the quality '#')
        picked = [(s[:length], q[:length]) for s, q in zip(d["seqs1"], d["quals1"]) if len(s) >= length and b"#" in q[:length]][:12]
        assert len(picked) >= 10, "%d reads of %d bases" % (len(picked), length)
        rets = [_three_calls(oracle, ctx, P, T, s, q, "k = %d, %d bases, read %d" % (d["k"], length, i))[0] for i, (s, q) in enumerate(picked)]
        assert max(rets) > 0, "no read of %d bases corrected: %s" % (length, rets)
    ctx.close()


# ---- c. the instances compiled for one k, and a table with extension bits -----------------------------------------------------

@pytest.mark.parametrize("k,pad_to", [(23, 30_000), (25, 450_000), (28, 120_000)])
def test_compiled_for_k_and_extension_bit_instances(oracle, k, pad_to):
    from test_k_sweep import _check_layout
    d = datasets.k_sweep(k, 0, pad_to)
    T, P = oracle_setup(oracle, d)
    ctx = _ctx(d)
    layout, ext = _check_layout(ctx, d)
    assert layout == 1 and ((ext > 0) if k == 28 else (ext == 0))   # rc_k3_special: PACKED without extension bits at k = 23 / 25
    n = min(300, len(d["seqs1"]))
    rets = [_three_calls(oracle, ctx, P, T, d["seqs1"][i], d["quals1"][i], "k = %d read %d" % (k, i))[0] for i in range(n)]
    ctx.close()
    assert sum(r > 0 for r in rets) >= 50, "k = %d: %d of %d reads corrected" % (k, sum(r > 0 for r in rets), n)


# ---- d. pair_strong_threshold -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n", [("se_k23", 150), ("skew", 150), ("max1023", 80)])
def test_any_pair_strong_threshold_matches_the_oracle(oracle, name, n):
    d = datasets.make(name)
    sweep = oracle_pair_sweep(oracle, d, n)
    acts = check_pair_sweep_is_not_vacuous(name, sweep)
    ctx = _ctx(d)
    for i, (strong, res) in enumerate(sweep):
        for t, want in res.items():
            got = ctx.correct_read(d["seqs1"][i], d["quals1"][i], t)
            assert got == want[:2], "%s read %d (strong %d) under pair_t = %d: %r, the oracle's %r (pair_t acts on %d of %d reads)" % (
                name, i, strong, t, got, want[:2], acts, n)
    ctx.close()


# ---- e. a pair, done the reference's way (main.cpp:401-402, ErrorCorrection.cpp:96-121) -----------------------------------------

@pytest.mark.parametrize("name", ["pe_k23", "pe_var"])
def test_a_pair_corrected_read_by_read_equals_the_paired_batch(oracle, name):
    d = datasets.make(name)
    n_pairs, n = len(d["seqs1"]), 150
    ret, l, m, h, a1, a2 = datasets.run_oracle(oracle, d)
    want1 = oracle.unpack_reads(a1, oracle.pack_reads(d["seqs1"])[1])
    want2 = oracle.unpack_reads(a2, oracle.pack_reads(d["seqs2"])[1])
    ctx = _ctx(d)
    lowered = 0
    for i in range(n):
        m1, m2 = d["seqs1"][i], d["seqs2"][i]
        s1, s2 = ctx.strong_threshold_read(m1), ctx.strong_threshold_read(m2)
        t = min(s1, s2)
        lowered += s1 != s2 and t >= 1
        for j, seq, qual, want in ((i, m1, d["quals1"][i], want1[i]), (n_pairs + i, m2, d["quals2"][i], want2[i])):
            got = ctx.correct_read(seq, qual, t)
            assert got == (ret[j], want), "%s pair %d, mate %d: %r, the paired batch's %r" % (name, i, 1 + (j >= n_pairs), got, (ret[j], want))
            assert ctx.kmer_info_read(got[1]) == (l[j], m[j], h[j]), "%s pair %d, mate %d: l/m/h" % (name, i, 1 + (j >= n_pairs))
    ctx.close()
    assert lowered >= 20 and int((ret[:n] > 0).sum()) >= 20, "%s: %d pairs whose mates' thresholds differ" % (name, lowered)


# ---- f. qualities as they arrive ------------------------------------------------------------------------------------------------

def test_qualities_as_they_arrive(oracle):
    d = datasets.make("se_k23")
    T, P = oracle_setup(oracle, d)
    ctx = _ctx(d)
    picked = [i for i in range(400) if oracle.error_correction(P, T, d["seqs1"][i], d["quals1"][i])[0] > 0][:40]
    assert len(picked) == 40
    for i in picked:
        seq, qual = d["seqs1"][i], d["quals1"][i]
        full = oracle.error_correction(P, T, seq, qual)
        none = oracle.error_correction(P, T, seq, b"\0" * len(seq))
        assert ctx.correct_read(seq, None) == none and ctx.correct_read(seq, b"") == none, "read %d without qualities" % i
        half = qual[:len(seq) // 2]
        want_half = oracle.error_correction(P, T, seq, half + b"\0" * (len(seq) - len(half)))
        assert ctx.correct_read(seq, half) == want_half, "read %d with half its qualities" % i
        assert ctx.correct_read(seq, qual + b"IIII#") == ctx.correct_read(seq, qual) == full, "read %d with five quality bytes too many" % i
    ctx.close()
    # a read on which the qualities decide (datasets.quality_dependent: its result changes when no quality test is ever true)
    name = "qv_ends/high"
    assert name in datasets.QV_NAMES
    d = datasets.make(name)
    assert d["mode"] == 0 and d["badq"] == b"H"
    T, P = oracle_setup(oracle, d)
    for i, (seq, qual) in enumerate(zip(d["seqs1"], d["quals1"])):
        with_q, flat, without = (oracle.error_correction(P, T, seq, q) for q in (qual, b"H" * len(seq), None))
        if with_q != flat and with_q != without:
            break
    else:
        raise AssertionError("qv_pair/high: no read on which the qualities decide")
    ctx = _ctx(d)
    got_with, got_without = ctx.correct_read(seq, qual), ctx.correct_read(seq, None)
    ctx.close()
    assert got_with != got_without and got_with == with_q and got_without == without, "qv_pair/high read %d" % i


# ---- g. refusals ----------------------------------------------------------------------------------------------------------------

def _refused(ctx, status, text, seq=b"ACGT" * 30):
    """All three calls are refused with `status` and `text` in rc_last_error, and correct_read leaves its buffer as it was."""
    L, h = ctx._L, ctx._h
    out = [C.c_int32(-77) for _ in range(4)]
    buf = C.create_string_buffer(seq)
    calls = {"strong_threshold_read": lambda: L.rc_strong_threshold_read(h, seq, C.byref(out[0])),
             "correct_read": lambda: L.rc_correct_read(h, buf, b"I" * len(seq), -1, C.byref(out[0])),
             "kmer_info_read": lambda: L.rc_kmer_info_read(h, seq, C.byref(out[1]), C.byref(out[2]), C.byref(out[3]))}
    for what, call in calls.items():
        assert call() == status, what
        assert text in L.rc_last_error(h).decode(), "%s: %s" % (what, L.rc_last_error(h).decode())
    assert buf.raw == seq + b"\0" and [o.value for o in out] == [-77] * 4


def test_what_the_per_read_calls_refuse(oracle):
    import rcorrector_amd
    d = datasets.make("max1023")
    T, P = oracle_setup(oracle, d)
    long_read = (d["seqs1"][0] + d["seqs1"][1] + d["seqs1"][2] + d["seqs1"][3])[:1024]
    assert len(long_read) == 1024
    # no table; a table, but no run parameters
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    _refused(ctx, RC_ERR_STATE, "no k-mer table loaded")
    ctx.table_build(d["keys"], d["counts"])
    _refused(ctx, RC_ERR_STATE, "rc_set_run_params")
    ctx.set_run_params(d["rate"], b"H")
    # 1 024 bases: refused; 1 023 and none: accepted
    _refused(ctx, RC_ERR_ARG, "exceeds the 1023-base limit", long_read)
    for seq in (long_read[:1023], b""):
        _three_calls(oracle, ctx, P, T, seq, b"I" * len(seq), "a read of %d bases" % len(seq))
    # quality bits on: refused; off again: accepted
    ctx.set_quality_bits(True)
    _refused(ctx, RC_ERR_STATE, "per-read entry points take quality bytes")
    with pytest.raises(rcorrector_amd.RcorrectorError, match="rc=-4: .*per-read entry points take quality bytes"):
        ctx.correct_read(d["seqs1"][0], d["quals1"][0])
    ctx.set_quality_bits(False)
    _three_calls(oracle, ctx, P, T, d["seqs1"][0], d["quals1"][0], "after quality bits")
    ctx.close()


# ---- h. the context afterwards --------------------------------------------------------------------------------------------------

def _batch_inputs(oracle, ctx, d, pinned):
    a, off = oracle.pack_reads(d["seqs1"])
    qa, _ = oracle.pack_reads(d["quals1"])
    if not pinned:
        return a, qa, off, None
    pa, pq = ctx.host_array(a.size), ctx.host_array(qa.size)
    pa[:], pq[:] = a, qa
    return pa, pq, off, [ctx.host_array(len(off) - 1, np.int32) for _ in range(4)]


def _run_batch(oracle, ctx, d, slots):
    a, qa, off, res = _batch_inputs(oracle, ctx, d, slots)
    if slots:
        ctx.submit(0, 0, a, qa, off, res=res)
        got = ctx.wait(0)
    else:
        got = ctx.correct_batch(0, a, qa, off)
    return tuple(np.array(x) for x in got) + (np.array(a),)


@pytest.mark.parametrize("slots", [False, True], ids=["correct_batch", "submit_wait_pinned"])
def test_batches_around_per_read_calls(oracle, slots):
    import rcorrector_amd
    d = datasets.make("se_k23")
    want = datasets.run_oracle(oracle, d)
    T, P = oracle_setup(oracle, d)
    ctx = _ctx(d)
    first = _run_batch(oracle, ctx, d, slots)
    for w, g, what in zip(want, first, ["ret", "l", "m", "h", "seq"]):
        assert np.array_equal(w, g), "%s of the first batch" % what
    assert ctx.debug_routes(len(d["seqs1"]))[0].shape == (len(d["seqs1"]),)
    # 20 per-read calls of all three kinds, reads of 50, 300 and 1 023 bases among them: the shared buffers regrow
    joined = b"".join(d["seqs1"][:11])
    reads = [d["seqs1"][0], d["seqs1"][1][:50], joined[:300], joined[:1023], d["seqs1"][2], joined[100:400], d["seqs1"][3][:50]]
    for j, seq in enumerate(reads[:5]):
        _three_calls(oracle, ctx, P, T, seq, b"I" * len(seq), "read %d between the batches" % j)   # (4 calls each)
    # the summary counts a correct_read as a batch of one, and the other two calls not at all
    for j, seq in enumerate(reads):
        before = ctx.summary()
        ctx.strong_threshold_read(seq)
        ctx.kmer_info_read(seq)
        assert ctx.summary() == before
        ret, _ = ctx.correct_read(seq, b"I" * len(seq))
        assert ctx.summary() == (before[0] + 1, before[1] + max(ret, 0)), "read %d: ret %d" % (j, ret)
    corrected = [i for i in range(len(want[0])) if want[0][i] > 0][:3]
    for i in corrected:
        before = ctx.summary()
        ret, _ = ctx.correct_read(d["seqs1"][i], d["quals1"][i])
        assert ret == want[0][i] > 0 and ctx.summary() == (before[0] + 1, before[1] + ret)
    # the routes of the last batch are gone (no classification ran for the read); the next batch brings them back
    with pytest.raises(rcorrector_amd.RcorrectorError, match="without classification"):
        ctx.debug_routes(len(d["seqs1"]))
    again = _run_batch(oracle, ctx, d, slots)
    for w, f, g, what in zip(want, first, again, ["ret", "l", "m", "h", "seq"]):
        assert np.array_equal(f, g) and np.array_equal(w, g), "%s of the batch after the per-read calls" % what
    cls, cand, _ = ctx.debug_routes(len(d["seqs1"]))
    assert cls.shape == cand.shape == (len(d["seqs1"]),)
    ctx.close()


def test_per_read_calls_are_in_no_census(oracle):
    """rcorrector_amd.h on rc_correct_read: one read is no batch of the run for the duplicate and the recurrent-correction census."""
    d = datasets.make("se_k23")
    want = datasets.run_oracle(oracle, d)
    ctx = _ctx(d)
    ctx.dup_census_begin()
    ctx.recur_census_begin()
    a, off = oracle.pack_reads(d["seqs1"][:500])
    qa, _ = oracle.pack_reads(d["quals1"][:500])
    ctx.correct_batch(0, a, qa, off)

    def census():
        dup, rec = ctx.dup_census(100), ctx.recur_census(100)
        flat = lambda c: {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        return flat(dup), flat(rec)
    before = census()
    assert before[0]["units"] == 500 and before[1]["changes"] > 0
    corrected = [i for i in range(500, len(want[0])) if want[0][i] > 0][:10]
    for i in corrected:
        assert ctx.correct_read(d["seqs1"][i], d["quals1"][i])[0] == want[0][i]
    assert len(corrected) == 10 and census() == before
    ctx.dup_census_end()
    ctx.recur_census_end()
    ctx.close()


# ---- i. small k: the segment capacity rule is fill_args' own, for both entries -------------------------------------------------

@pytest.mark.parametrize("length", [100, 250, 600])
def test_small_k_per_read_and_batch_of_one_agree(oracle, length):
    import rcorrector_amd
    d = datasets.k_sweep(5, 0)
    T, P = oracle_setup(oracle, d)
    rng = np.random.Generator(np.random.PCG64(5005))
    seq = synth.NUC[rng.integers(0, 4, 1000, dtype=np.uint8)].tobytes()[200:200 + length]
    qual = b"I" * length
    want = oracle_read(oracle, P, T, seq, qual)
    ctx = _ctx(d)
    outcomes = []
    for entry in ("correct_read", "correct_batch"):
        try:
            if entry == "correct_read":
                outcomes.append(ctx.correct_read(seq, qual) + ctx.kmer_info_read(ctx.correct_read(seq, qual)[1]))
            else:
                a, off = oracle.pack_reads([seq])
                qa, _ = oracle.pack_reads([qual])
                ret, l, m, h = ctx.correct_batch(0, a, qa, off)
                outcomes.append((int(ret[0]), oracle.unpack_reads(a, off)[0], int(l[0]), int(m[0]), int(h[0])))
        except rcorrector_amd.RcorrectorError as e:
            assert "too many segments" in str(e), "%s: %s" % (entry, e)
            outcomes.append("too many segments")
    ctx.close()
    assert outcomes[0] == outcomes[1], "k = 5, %d bases: correct_read %r, correct_batch %r" % (length, outcomes[0], outcomes[1])
    assert outcomes[0] in (want, "too many segments"), "k = 5, %d bases: %r, the oracle's %r" % (length, outcomes[0], want)
