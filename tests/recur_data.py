"""A data set on which corrections RECUR (tests/test_recur_keys.py asserts that they do, on the oracle; the GPU tests of the
recurrence census run on it): a few transcripts sequenced deep, reads drawn from both strands, a minor allele carried by
about one read in fifteen at a handful of sites -- one of them eight bases from a transcript's end, where many reads end, so
its corrections are clipped -- ordinary random substitutions, and a few N.  Same dict as tests/datasets.py: make()."""
import numpy as np

import synth

K = 23
LENGTH = 100
N_TX = 3
L_TX = 400
SEED = 20260
DEPTH_READS = 2400          # reads (mode 0) or reads over both mates (modes 1 and 2)
MINOR_EVERY = 15            # a read that covers a site carries the minor allele with probability 1 / MINOR_EVERY
ERR = 0.004
RATE = 0.05               # the ERROR_RATE handed to the corrector: at 200-fold depth a k-mer seen a dozen times is an error to it
P_N = 0.002
SITES = [(0, 150), (0, 260), (1, 90), (1, 200), (2, 310), (2, L_TX - 9)]   # (transcript, position); the last one ends reads

COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    COMP[_a] = _b


def _reads(seed, n):
    rng = np.random.Generator(np.random.PCG64(seed))
    tx = [rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), L_TX) for _ in range(N_TX)]
    minor = {}
    for t, p in SITES:
        alt = [c for c in b"ACGT" if c != tx[t][p]]
        minor[(t, p)] = alt[int(rng.integers(0, 3))]
    seqs = np.empty((n, LENGTH), dtype=np.uint8)
    strand = np.zeros(n, dtype=np.int8)
    for i in range(n):
        t = int(rng.integers(0, N_TX))
        # one read in four ends exactly where its transcript does
        s = L_TX - LENGTH if rng.random() < 0.25 else int(rng.integers(0, L_TX - LENGTH + 1))
        r = tx[t][s:s + LENGTH].copy()
        for (st, sp), alt in minor.items():
            if st == t and s <= sp < s + LENGTH and rng.random() < 1.0 / MINOR_EVERY:
                r[sp - s] = alt
        err = rng.random(LENGTH) < ERR
        for p in np.flatnonzero(err):
            r[p] = [c for c in b"ACGT" if c != r[p]][int(rng.integers(0, 3))]
        r[rng.random(LENGTH) < P_N] = ord("N")
        if rng.random() < 0.5:
            r = COMP[r[::-1]]
            strand[i] = 1
        seqs[i] = r
    return seqs, strand


def make(mode=0, seed=SEED, n=DEPTH_READS):
    """dict(k, mfk, rate, mode, keys, counts, seqs1, quals1, seqs2, quals2, strand) -- mode 1: the reads' second half as mate 2,
    mode 2: the reads interleaved (reads 2u and 2u + 1 a pair).  The same reads in every mode, so one table."""
    seqs, strand = _reads(seed, n)
    keys, cnt = synth.count_kmers([seqs], K)
    rows = [r.tobytes() for r in seqs]
    quals = [b"I" * LENGTH] * n
    d = dict(k=K, mfk=4, rate=RATE, mode=mode, keys=keys, counts=cnt, strand=strand, seqs2=None, quals2=None)
    if mode == 1:
        h = n // 2
        d.update(seqs1=rows[:h], quals1=quals[:h], seqs2=rows[h:], quals2=quals[h:])
    else:
        d.update(seqs1=rows, quals1=quals)
    return d


def all_reads(d):
    """the reads of d in arena order (mode 1: mate 1's, then mate 2's)"""
    return list(d["seqs1"]) + (list(d["seqs2"]) if d["mode"] == 1 else [])
