"""The synthetic batches the trimming tests share (tests/test_read_trim_host.py on the CPU, tests/test_read_trim.py on the GPU),
each named by the edge it hits, and the model's answer for each, computed once (tests/trim_model.py)."""
import functools

import numpy as np

import trim_model as tm

AD = b"AGATCGGAAGAGC"
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 100]     # 100: an even number of reads for the pairs
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def rand_seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes())


def rand_qual(rng, n, lo=2, hi=41):
    return bytes((rng.integers(lo, hi + 1, n) + 33).astype(np.uint8).tobytes())


def pair_of(rng, F, La, Lb, tail=b"T"):
    """the mates of a fragment of F bases read La and Lb bases deep; a mate that runs through reads `tail` repeated behind it"""
    frag = rand_seq(rng, F)
    a = (frag + tail * La)[:La]
    b = (revcomp(frag) + tail * Lb)[:Lb]
    return a, b


def _scenario(name, mode, seqs, quals=None, max_read_len=None, **p):
    return {"name": name, "mode": mode, "seqs": list(seqs), "quals": None if quals is None else list(quals), "p": tm.params(**p),
            "max_read_len": max_read_len if max_read_len is not None else max([len(s) for s in seqs] + [0])}


def _interleave(pairs):
    return [m for pr in pairs for m in pr]


def _halves(pairs):
    return [pr[0] for pr in pairs] + [pr[1] for pr in pairs]


def scenarios():
    rng = np.random.default_rng(20261021)
    out = []
    # ---- lengths, the instance boundary, a wrong max_read_len -------------------------------------------------------------------
    seqs = []
    for L in LENGTHS:
        s = rand_seq(rng, L)
        if L >= 33:
            s = s[:L - 9] + AD[:9]            # an adapter at the end of the longer ones
        seqs.append(s)
    quals = [rand_qual(rng, len(s), 2, 41) for s in seqs]
    for mode in (0, 1, 2):
        for mrl in (256, 257, 1023):
            out.append(_scenario("lengths mode %d max_read_len %d" % (mode, mrl), mode, seqs, quals, mrl, min_len=16))
    # ---- pair offsets ----------------------------------------------------------------------------------------------------------
    pairs = [pair_of(rng, 60, 100, 80),       # d* = -20 < 0, F < La
             pair_of(rng, 80, 100, 80),       # d* = 0, F < La
             pair_of(rng, 100, 100, 80),      # d* = 20 > 0, F = La
             pair_of(rng, 130, 100, 80),      # d* = 50, F > La
             pair_of(rng, 90, 90, 120),       # F = La, mate 2 runs through: d* = -30
             pair_of(rng, 300, 150, 150),     # d* = 150: no overlap at all
             (rand_seq(rng, 100), rand_seq(rng, 77)),      # unrelated mates: no accepted offset
             pair_of(rng, 40, 151, 151),      # a short fragment, both mates run through
             pair_of(rng, 500, 300, 257),     # the wide instance: d* = 243
             pair_of(rng, 1023, 1023, 1023),  # d* = 0 at full length
             pair_of(rng, 29, 60, 60),        # an overlap one below pair_min_overlap: not accepted
             pair_of(rng, 30, 60, 60)]        # ... and exactly at it
    out.append(_scenario("pair offsets interleaved", 2, _interleave(pairs), min_len=0, adapter1=b"", qual_min=0))
    out.append(_scenario("pair offsets in halves", 1, _halves(pairs), min_len=0, adapter1=b"", qual_min=0))
    out.append(_scenario("pair offsets, the option off", 2, _interleave(pairs), min_len=0, adapter1=b"", qual_min=0, pair_overlap=False))
    out.append(_scenario("pair offsets with every cut", 2, _interleave(pairs), [rand_qual(rng, len(s), 10, 41) for s in _interleave(pairs)], min_len=25))
    noisy = []
    for F, La, Lb, nerr in ((70, 100, 100, 7), (70, 100, 100, 8), (120, 100, 100, 3)):     # 70 faced: 7 of 70 is 10 %, 8 is past it
        a, b = pair_of(rng, F, La, Lb)
        a = bytearray(a)
        for i in range(nerr):
            a[5 + 8 * i] = b"ACGT"[(b"ACGT".index(a[5 + 8 * i]) + 1) % 4]
        noisy.append((bytes(a), b))
    noisy.append((pairs[0][0][:50] + b"N" + pairs[0][0][51:], pairs[0][1].lower()[:10] + pairs[0][1][10:]))   # N and lower case in the overlap
    out.append(_scenario("pair mismatches at and past the share", 2, _interleave(noisy), min_len=0, adapter1=b"", qual_min=0))
    # ---- adapters --------------------------------------------------------------------------------------------------------------
    T = b"T" * 200
    reads = [AD + T[:40],                          # d = 0: keep_len 0
             T[:55] + AD[:5],                      # d = L - adapter_min: just accepted
             T[:56] + AD[:4],                      # d = L - adapter_min + 1: not accepted
             T[:30] + AD + T[:20],                 # in the middle
             T[:20] + AD + T[:10] + AD + T[:5],    # two accepted offsets: the smaller wins
             T[:30] + b"AGATNGGAAGAGC" + T[:7],    # an N under the adapter: one position fewer compared
             T[:30] + b"AGATcGGAAGAGC" + T[:7],    # a lower-case base under it
             T[:30] + b"AGATCGGAAGTGC" + T[:7],    # one mismatch of 13: 100 <= 10 * 13, accepted
             T[:30] + b"AGATCGCAAGTGC" + T[:7],    # two of 13: not accepted there
             T[:64], b"", b"A"]
    out.append(_scenario("adapter offsets", 0, reads, min_len=0, qual_min=0))
    for n in (1, 32, 33, 64):
        ad = rand_seq(rng, n)
        other = bytes(b"ACGT"[(b"ACGT".index(x) + 2) % 4] for x in ad)
        reads = [rand_seq(rng, 20) + ad + rand_seq(rng, 15), rand_seq(rng, 31) + ad, rand_seq(rng, 62) + ad[:max(1, n // 2)], ad, other + ad,
                 rand_seq(rng, 250) + ad[:6], rand_seq(rng, 300) + ad + rand_seq(rng, 40)]
        reads = reads + [rand_seq(rng, 50)] * (len(reads) % 2)
        out.append(_scenario("adapter of %d bases" % n, 0, reads, min_len=0, qual_min=0, adapter1=ad, adapter_min=min(n, 5)))
        out.append(_scenario("adapter of %d bases on mate 2 only" % n, 2, reads, min_len=0, qual_min=0, adapter1=b"", adapter2=ad, adapter_min=min(n, 5),
                             pair_overlap=False))
    ad20 = b"ACGTTGCAAGGCTTAGCCAT"
    reads = [b"G" * 40 + _mutate(ad20, 2), b"G" * 40 + _mutate(ad20, 3), b"G" * 40 + ad20]
    out.append(_scenario("adapter mismatch share at and past 10 %", 0, reads, min_len=0, qual_min=0, adapter1=ad20, adapter_min=20))
    out.append(_scenario("adapter mismatch share 0 %", 0, reads, min_len=0, qual_min=0, adapter1=ad20, adapter_min=20, adapter_mm_pct=0))
    out.append(_scenario("adapter mismatch share 50 %, adapter_min 64", 0, reads + [rand_seq(rng, 90) + rand_seq(rng, 64)], min_len=0, qual_min=0,
                         adapter1=rand_seq(rng, 64), adapter_min=64, adapter_mm_pct=50))
    # ---- qualities -------------------------------------------------------------------------------------------------------------
    q = lambda *runs: b"".join(bytes([33 + v]) * n for v, n in runs)
    qs = [q((40, 60)),                              # all high: no cut
          q((2, 60)),                               # all low: cut 0
          q((2, 10), (40, 40), (2, 10)),            # bad head, good middle, bad tail: the early stop keeps the head
          q((40, 30), (20, 30)),                    # a tail exactly at the threshold: ties in S, the larger i wins -- no cut
          q((40, 30), (21, 1), (19, 1), (40, 1), (0, 1), (40, 26)),      # S returns to its maximum further in
          q((40, 59), (2, 1)), q((2, 1), (40, 59)), q((40, 17), (2, 300)), q((30, 1000), (10, 23)), q((40, 16), (19, 16), (21, 16), (19, 17)), b"", q((2, 1))]
    seqs = [rand_seq(rng, len(x)) for x in qs]
    out.append(_scenario("qualities", 0, seqs, qs, min_len=0, adapter1=b""))
    out.append(_scenario("qualities, qual_min 0", 0, seqs, qs, min_len=0, adapter1=b"", qual_min=0))
    out.append(_scenario("qualities, none given", 0, seqs, None, min_len=0, adapter1=b""))
    out.append(_scenario("qualities, phred 64 and threshold 93", 2, seqs, [bytes(min(255, x + 31) for x in s) for s in qs], min_len=0, adapter1=b"",
                         qual_base=64, qual_min=93, pair_overlap=False))
    out.append(_scenario("qualities, a random walk of S over 1023 bases and every byte value", 0, [rand_seq(rng, 1023), rand_seq(rng, 256)],
                         [bytes(np.concatenate([rng.integers(55, 76, 600), rng.integers(33, 95, 400), rng.integers(33, 41, 23)]).astype(np.uint8).tobytes()), bytes(range(1, 257 - 1)).replace(b"\n", b"!") + b"~"],
                         min_len=0, adapter1=b"", qual_min=32))
    # ---- the unit rule ---------------------------------------------------------------------------------------------------------
    reads = [T[:20] + AD, T[:21] + AD, T[:19] + AD, T[:60], T[:60], T[:19] + AD, T[:20], T[:19]]
    for mode in (0, 1, 2):
        out.append(_scenario("min_len at and above keep_len, mode %d" % mode, mode, reads, min_len=20, qual_min=0, pair_overlap=False))
    return out


def _mutate(s, k):
    """s with its bases 3, 10, 17, ... (k of them) changed"""
    s = bytearray(s)
    for j in range(k):
        i = 3 + 7 * j
        s[i] = b"ACGT"[(b"ACGT".index(s[i]) + 1) % 4]
    return bytes(s)


@functools.lru_cache(maxsize=None)
def all_scenarios():
    return tuple(scenarios())


def lmax_of(max_read_len):
    """the bases of a mate the instance picked by max_read_len looks at"""
    return 256 if max_read_len <= 256 else tm.MAX_LEN


_EXPECTED = {}


def expected(i):
    """(rows, keep, tally) of scenario i by the model, computed once"""
    if i not in _EXPECTED:
        s = all_scenarios()[i]
        _EXPECTED[i] = tm.trim_batch(s["seqs"], s["quals"], s["mode"], s["p"], lmax_of(s["max_read_len"]))
    return _EXPECTED[i]
