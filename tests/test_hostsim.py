"""CPU: the kernel's wave-uniform control flow (rc_correct_core.h, lane-serial build) must give
the oracle's results read for read.  This is what lets the search kernel be debugged without a GPU."""
import numpy as np
import pytest

import datasets


@pytest.mark.parametrize("name", ["se_k23", "pe_k23", "il_k23", "k31_mc8", "skew", "nrich", "varlen", "k15", "k32", "pe_var", "edge", "long300", "long600_k31", "max1023", "k11", "polya_k23", "polya_k31", "polya_k15",
                                  "se_151", "pe_151", "pe_160_k15", "tiers_se", "tiers_pe", "tiers_il"] + datasets.QV_NAMES + datasets.HUGE_NAMES)
def test_core_control_flow_matches_oracle(oracle, hostsim, name):
    d = datasets.make(name)
    want = datasets.run_oracle(oracle, d)
    got = datasets.run_oracle(oracle, d, fn=lambda p, t, b: hostsim.hostsim_correct_batch(p, t, b, None))
    for w, g, what in zip(want, got, ["ret", "l", "m", "h", "seq1", "seq2"]):
        assert np.array_equal(w, g), "%s differs on %s" % (what, name)
    assert (want[0] > 0).sum() > 0 or name == "edge"


# ---- one read per call, with any pairStrongTrustThreshold (ErrorCorrection.h:27) ----
# The batch above passes a read either -1 or the minimum of the two mates' thresholds.  rc_correct_read passes whatever its
# caller says (rc_kernel_args::pair_override) and runs the front end inside the correction kernel; hostsim_correct_read is
# that wave's work, lane-serial.  tests/test_per_read.py runs the same sweep on the GPU.

def oracle_setup(oracle, d):
    """(table, parameters) of data set d for the oracle's per-read functions, quality threshold 'H'"""
    T = oracle.Table(d["k"], len(d["keys"]))
    T.put_many(d["keys"], d["counts"])
    return T, oracle.make_params(d["k"], d["mfk"], d["rate"], b"H")


def oracle_read(oracle, P, T, seq, qual, pair_t=-1):
    """(ret, corrected bases, l, m, h) of one read: ErrorCorrection, then GetKmerInformation of what it left"""
    ret, out = oracle.error_correction(P, T, seq, qual, pair_t)
    return (ret, out) + oracle.kmer_information(P, T, out)


def pair_sweep(strong):
    """The values of pairStrongTrustThreshold a read with threshold `strong` is corrected with: none, the edges of
    `pair_t >= 1` (ErrorCorrection.cpp:818), either side of the `pair_t < 20` of :819, either side of `strong > pair_t`,
    and one far beyond any count."""
    return list(dict.fromkeys([-1, 0, 1, 2, 19, 20, max(strong - 1, 1), strong, strong + 1, 10 ** 6]))


def oracle_pair_sweep(oracle, d, n):
    """Per read of the first n of d: (strong, {pair_t: oracle_read(...)}) over pair_sweep(strong)"""
    T, P = oracle_setup(oracle, d)
    out = []
    for seq, qual in zip(d["seqs1"][:n], d["quals1"][:n]):
        strong = oracle.strong_threshold(P, T, seq)
        out.append((strong, {t: oracle_read(oracle, P, T, seq, qual, t) for t in pair_sweep(strong)}))
    return out


def check_pair_sweep_is_not_vacuous(name, sweep, floor=5):
    """What the oracle alone must show before a sweep may count as a test of pair_t: on at least `floor` reads some value
    changes the result, and on no read does a value outside 1 <= pair_t < strong (:818: `pairStrongTrustThreshold >= 1 &&
    strongTrustThreshold > pairStrongTrustThreshold`).  Returns the number of reads on which pair_t acts."""
    acts = 0
    for i, (strong, res) in enumerate(sweep):
        acts += any(r != res[-1] for r in res.values())
        for t in (0, strong, strong + 1, 10 ** 6):
            assert res[t] == res[-1], "%s read %d (strong %d): the oracle's result under pair_t = %d differs from -1's" % (name, i, strong, t)
        for t, r in res.items():
            assert r == res[-1] or 1 <= t < strong, "%s read %d (strong %d): pair_t = %d acts" % (name, i, strong, t)
    assert acts >= floor, "%s: pair_t changes the oracle's result on %d of %d reads only (need %d)" % (name, acts, len(sweep), floor)
    return acts


@pytest.mark.parametrize("name", ["se_k23", "skew", "edge", "k31_mc8", "max1023"])
def test_one_read_with_any_pair_threshold_matches_oracle(oracle, hostsim, name):
    import ctypes as C
    fn = hostsim.hostsim_correct_read
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_int] + [C.POINTER(C.c_int32)] * 4
    d = datasets.make(name)
    n = min(300, len(d["seqs1"]))
    sweep = oracle_pair_sweep(oracle, d, n)
    acts = check_pair_sweep_is_not_vacuous(name, sweep)
    T, P = oracle_setup(oracle, d)
    corrected = 0
    for i, (strong, res) in enumerate(sweep):
        seq, qual = d["seqs1"][i], d["quals1"][i]
        for t, want in res.items():
            buf = C.create_string_buffer(seq)
            qbuf = C.create_string_buffer(qual, len(seq) + 1)
            out = [C.c_int32(0) for _ in range(4)]
            fn(C.byref(P), T.h, buf, qbuf, t, *[C.byref(o) for o in out])
            got = (out[0].value, buf.value, out[1].value, out[2].value, out[3].value)
            assert got == want, "%s read %d (strong %d) under pair_t = %d: (ret, bases, l, m, h) differ (pair_t acts on %d of %d reads)" % (
                name, i, strong, t, acts, n)
        corrected += res[-1][0] > 0
    assert corrected > 0 or name == "edge", "%s: no read of %d corrected; pair_t acts on %d" % (name, n, acts)
