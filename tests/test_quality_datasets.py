"""CPU: the qv_ data sets (tests/datasets.py) are inputs on which the base qualities decide what the correction's closing vetoes
do.  That is a condition on the inputs, so it is checked on the oracle alone: the tests that lean on these sets (test_hostsim,
test_quality_vetoes, ...) would otherwise pass just as well on reads whose qualities never matter, as the older sets' do."""
import numpy as np
import pytest

import datasets


@pytest.mark.parametrize("name", datasets.QV_NAMES)
def test_qualities_decide_on_the_qv_sets(oracle, name):
    """Reads whose (ret, corrected bases) change when every quality byte is set to the threshold: none on the `low` controls, at
    least 100 on the high / inverted members of qv_pair, qv_ends, qv_dense and qv_mixed_*, at least 30 on every other set."""
    d = datasets.make(name)
    want = datasets.run_oracle(oracle, d)
    n = datasets.quality_dependent(oracle, d, want)
    print("%s: qualities decide on %d of %d reads (%d unfixable, %d corrected)" % (name, n, len(want[0]), int((want[0] == -1).sum()), int((want[0] > 0).sum())))
    assert len(want[0]) <= (600 if "lengths" in name else 2000)
    if d["control"]:
        assert n == 0, "%s: %d reads depend on their qualities" % (name, n)
    else:
        need = 100 if name in datasets.QV_STRONG else 30
        assert n >= need, "%s: qualities decide on %d reads, fewer than %d" % (name, n, need)
    if "dense" in name:   # the density veto's reject branch ran
        assert int((want[0] == -1).sum()) >= 20


def test_qv_sets_are_what_their_names_say():
    """By construction: qv_pair has exactly two substitutions per affected read, away from the ends, some exactly k - 1 and k
    apart; qv_ends has at least four, two to four of them in an end window; qv_dense has its bursts inside one k-window; the
    straddle model puts about a fifth of the bytes on the threshold; qv_lengths holds every length of the list."""
    for k in (23, 32):
        _, errs, _, _, _ = datasets.qv_reads("pair", k, 0, 0)
        per_read = errs[0].sum(axis=1)
        assert set(per_read.tolist()) == {0, 2} and not errs[0][:, :12].any() and not errs[0][:, -12:].any()
        gaps = np.array([np.diff(np.nonzero(e)[0])[0] for e in errs[0][per_read == 2]])
        assert gaps.min() >= 2 and gaps.max() == k and (gaps == k - 1).sum() >= 10 and (gaps == k).sum() >= 10
    _, errs, _, _, _ = datasets.qv_reads("ends", 23, 0, 0)
    hit = errs[0][errs[0].any(axis=1)]
    ends = np.maximum(hit[:, :10].sum(axis=1), hit[:, -10:].sum(axis=1))
    assert hit.sum(axis=1).min() >= 4 and ends.min() >= 2 and ends.max() <= 4
    for mfk in (1, 2, 3, 4, 5):
        _, errs, _, _, _ = datasets.qv_reads("dense", 23, mfk, 0)
        hit = errs[0][errs[0].any(axis=1)]
        width = np.array([np.ptp(np.nonzero(e)[0]) + 1 for e in hit])
        assert width.max() <= 23 and hit.sum(axis=1).min() >= (1 if mfk == 1 else mfk) and hit.sum(axis=1).max() <= (3 if mfk == 1 else mfk + 3)
    d = datasets.make("qv_mixed_pe/straddle")
    q = np.frombuffer(b"".join(d["quals1"] + d["quals2"]), np.uint8)
    assert 0.18 < (q == ord("H")).mean() < 0.22 and q.min() == ord("H") - 2 and q.max() == ord("H") + 2
    assert b"".join(d["quals1"]) != b"".join(d["quals2"])
    d = datasets.make("qv_lengths/straddle")
    assert sorted(set(len(r) for r in d["seqs1"])) == datasets.QV_LENGTHS
    d = datasets.make("qv_signed/signed")
    q = np.frombuffer(b"".join(d["quals1"]), np.uint8)
    assert 0.4 < (q >= 0x80).mean() < 0.6 and q.max() == 0xFF and q.min() > 0
