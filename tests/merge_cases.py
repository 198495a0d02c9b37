"""The synthetic batches the merging tests share (tests/test_read_merge_host.py on the CPU, tests/test_read_merge.py on the GPU),
each named by the edge it hits, and the model's answer for each, computed once (tests/merge_model.py).  Every batch says what the
model must give for it -- the merged lengths, how often mate 2 won -- so that none of them passes on an empty result."""
import functools

import numpy as np

import merge_model as mm
from trim_cases import pair_of, rand_qual, rand_seq, revcomp

_SEED = 20261022


def _scenario(name, mode, pairs, quals=True, max_read_len=None, lens=None, took=None, through=None, **p):
    """pairs: (a, b) or (a, b, qa, qb); quals: True -- random ones where a pair brings none; False -- none at all.  lens, took,
    through: what the model must give: every unit's merged_len, (took_mate1, took_mate2, ties), the read-through count"""
    rng = np.random.default_rng(sum(name.encode()))      # (the random qualities of a batch: by its name)
    full = []
    for pr in pairs:
        a, b = pr[0], pr[1]
        qa, qb = (pr[2], pr[3]) if len(pr) == 4 else (rand_qual(rng, len(a)), rand_qual(rng, len(b)))
        full.append((a, b, qa, qb))
    if mode == 2:
        seqs = [m for a, b, _, _ in full for m in (a, b)]
        qs = [m for _, _, qa, qb in full for m in (qa, qb)]
    else:
        seqs = [a for a, _, _, _ in full] + [b for _, b, _, _ in full]
        qs = [qa for _, _, qa, _ in full] + [qb for _, _, _, qb in full]
    return {"name": name, "mode": mode, "seqs": seqs, "quals": qs if quals else None, "p": mm.params(**p),
            "max_read_len": max_read_len if max_read_len is not None else max([len(s) for s in seqs] + [0]), "lens": lens, "took": took, "through": through}


def _mutate(s, at):
    s = bytearray(s)
    for i in at:
        s[i] = b"ACGT"[(b"ACGT".index(s[i]) + 1) % 4]
    return bytes(s)


def _flat(q, n):
    return bytes([33 + q]) * n


def scenarios():
    rng = np.random.default_rng(_SEED)
    out = []
    # ---- offsets ---------------------------------------------------------------------------------------------------------------
    a100 = rand_seq(rng, 100)
    pairs = [pair_of(rng, 60, 100, 80),        # d* = -20 < 0, F < La
             pair_of(rng, 80, 100, 80),        # d* = 0, F < La
             pair_of(rng, 90, 100, 60),        # d* = 30 > 0, F below La
             pair_of(rng, 100, 100, 80),       # d* = 20, F at La
             pair_of(rng, 130, 100, 80),       # d* = 50, F above La
             (a100, revcomp(a100[20:70])),     # mate 2 contained in mate 1: d* = 20, F = 70
             pair_of(rng, 90, 90, 120),        # mate 2 runs through: d* = -30, F = La
             (rand_seq(rng, 100), rand_seq(rng, 77)),     # unrelated mates: no accepted offset
             (a100, revcomp(a100)[:20]),       # a mate shorter than min_overlap
             (a100, b""), (b"", a100), (b"", b""),        # an empty mate
             pair_of(rng, 29 + 60, 60, 59),    # an overlap of 30: exactly min_overlap
             pair_of(rng, 29 + 60, 60, 58)]    # ... and of 29
    lens = [60, 80, 90, 100, 130, 70, 90, 0, 0, 0, 0, 0, 89, 0]
    for mode in (2, 1):
        out.append(_scenario("offsets mode %d" % mode, mode, pairs, lens=lens, took=(0, 0, 0), through=5))
    out.append(_scenario("offsets without qualities", 2, pairs, quals=False, lens=lens, took=(0, 0, 0), through=5))
    # ---- the mismatch share ----------------------------------------------------------------------------------------------------
    noisy = []
    for nerr in (7, 8):                        # 70 faced: 7 of 70 is 10 %, 8 is past it
        a, b = pair_of(rng, 70, 100, 100)
        noisy.append((_mutate(a, [5 + 8 * i for i in range(nerr)]), b, _flat(30, 100), _flat(20, 100)))
    out.append(_scenario("mismatch share at and past max_mismatch_pct", 2, noisy, lens=[70, 0], took=(7, 0, 0), through=1))
    out.append(_scenario("mismatch share, 12 per cent allowed, no qualities", 2, noisy, quals=False, lens=[70, 70], took=(0, 0, 15), through=2, max_mismatch_pct=12))
    # ---- merged lengths around the granule and the round -----------------------------------------------------------------------
    pairs = [pair_of(rng, 15, 12, 13), pair_of(rng, 16, 13, 13), pair_of(rng, 17, 13, 14), pair_of(rng, 1024, 600, 600), pair_of(rng, 1025, 600, 601),
             pair_of(rng, 31, 16, 25), pair_of(rng, 32, 20, 22), pair_of(rng, 33, 30, 13)]
    out.append(_scenario("merged lengths 15, 16, 17, 1024, 1025", 2, pairs, lens=[15, 16, 17, 1024, 1025, 31, 32, 33], took=(0, 0, 0), through=0, min_overlap=10))
    out.append(_scenario("two mates of 1023 bases overlapping by min_overlap", 2, [pair_of(rng, 2046 - 30, 1023, 1023), pair_of(rng, 2046 - 29, 1023, 1023)],
                         lens=[2016, 0], took=(0, 0, 0), through=0))
    long_pair = [pair_of(rng, 400, 300, 300), pair_of(rng, 150, 100, 100)]
    out.append(_scenario("a mate of 300 bases under max_read_len 256: the narrow instance's cut", 2, long_pair, max_read_len=256, lens=[400, 150], took=(0, 0, 0),
                         through=0))
    out.append(_scenario("a mate of 300 bases under max_read_len 300", 2, long_pair, lens=[400, 150], took=(0, 0, 0), through=0))
    # ---- qualities -------------------------------------------------------------------------------------------------------------
    a, b = pair_of(rng, 120, 80, 80)           # 40 faced, positions 40 .. 79 of a
    qa = _flat(20, 80)
    qr = _flat(20, 10) + _flat(21, 10) + _flat(22, 10) + _flat(0, 10) + _flat(30, 40)      # of r: sums 40, 41, 42 and 20 over the faced positions
    out.append(_scenario("agreement below, at and above qual_cap", 2, [(a, b, qa, qr[::-1])], lens=[120], took=(0, 0, 0), through=0))
    out.append(_scenario("agreement, qual_cap 93 and phred 64", 2, [(a, b, bytes(x + 31 for x in qa), bytes(x + 31 for x in qr[::-1]))], lens=[120], took=(0, 0, 0),
                         through=0, qual_base=64, qual_cap=62))
    a, b = pair_of(rng, 140, 100, 100)         # 60 faced, positions 40 .. 99 of a
    at = [45, 55, 65, 75, 85]
    qa, qr = bytearray(_flat(30, 100)), bytearray(_flat(30, 100))
    for i, (pa, pr) in zip(at, ((35, 10), (10, 35), (25, 25), (26, 25), (1, 41))):          # pa > pr, pa < pr, a tie, a difference of 1, 40 apart
        qa[i], qr[i - 40] = 33 + pa, 33 + pr
    qa[50], qr[12] = 32, 20                     # a quality byte below qual_base on an agreeing and on a disagreeing position
    qa[65] = 33 + 25
    dis = (_mutate(a, at), b, bytes(qa), bytes(qr[::-1]))
    out.append(_scenario("disagreements: mate 1 wins, mate 2 wins, a tie, the floor of 2", 2, [dis], lens=[140], took=(2, 2, 1), through=0))
    qa2, qr2 = bytearray(qa), bytearray(qr)
    qa2[45], qr2[5] = 30, 31                    # both below qual_base 40: phred 0 both, a tie; the others 3 : 28, 18 : 18, 19 : 18, 0 : 34
    out.append(_scenario("disagreements under qual_base 40: bytes below it are phred 0", 2, [(dis[0], b, bytes(qa2), bytes(qr2[::-1]))], lens=[140],
                         took=(1, 2, 2), through=0, qual_base=40))
    out.append(_scenario("disagreements without qualities", 2, [dis], quals=False, lens=[140], took=(0, 0, 5), through=0))
    # ---- bytes that are no base ------------------------------------------------------------------------------------------------
    a, b = pair_of(rng, 140, 100, 100)
    r = bytearray(revcomp(b))
    an = bytearray(a)
    an[50] = ord("N")                           # N against a base
    r[20] = ord("N")                            # a base against N (position 60)
    an[70], r[30] = ord("N"), ord("N")          # N against N
    an[80:83] = an[80:83].lower()               # lower case against bases
    r[45:47] = r[45:47].lower()                 # bases against lower case (positions 85, 86)
    an[5], r[95] = ord("n"), ord("-")           # outside the overlap: verbatim
    bn = bytes(r).translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]
    out.append(_scenario("N against a base, N against N, lower case", 2, [(bytes(an), bn)], lens=[140], took=(0, 0, 0), through=0))
    out.append(_scenario("N against a base, N against N, lower case, no qualities", 1, [(bytes(an), bn)], quals=False, lens=[140], took=(0, 0, 0), through=0))
    return out


@functools.lru_cache(maxsize=None)
def all_scenarios():
    return tuple(scenarios())


def lmax_of(max_read_len):
    """the bases of a mate the instance picked by max_read_len looks at"""
    return 256 if max_read_len <= 256 else mm.MAX_LEN


_EXPECTED = {}


def expected(i):
    """(rows, moff, mseq, mqual, tally) of scenario i by the model, computed once -- and checked against what the batch is for"""
    if i not in _EXPECTED:
        s = all_scenarios()[i]
        got = mm.merge_batch(s["seqs"], s["quals"], s["mode"], s["p"], lmax_of(s["max_read_len"]))
        rows, t = got[0], got[4]
        assert rows[:, 0].tolist() == s["lens"], (s["name"], rows[:, 0].tolist())
        assert (t["took_mate1"], t["took_mate2"], t["ties"]) == s["took"], (s["name"], t["took_mate1"], t["took_mate2"], t["ties"])
        assert t["readthrough"] == s["through"], (s["name"], t["readthrough"])
        _EXPECTED[i] = got
    return _EXPECTED[i]
