"""The arenas a merge leaves behind, as fixtures: what tests/test_merged_arena.py (GPU) hands from rc_read_merge_device to every
per-read entry point and tests/test_merged_arena_cases.py (CPU) guards.  Pure Python and numpy: nothing here imports the library.

A merged arena looks like no other input of the suite: an unmerged unit is a single NUL byte, so it holds runs of hundreds of
empty reads; its offsets are dense, so d_moff[u] % 16 takes every value; a merged read may have up to 2045 bases; and its quality
bytes are computed ones (qual_base + min(pa + pb, qual_cap) where the mates agree, down to qual_base + 2 where they do not).

Every pair is cut from one fixed-seed random genome of 40 000 bases, so a table counted from the error-free fragments has solid
23-mers and the substitutions sprinkled into the mates are correctable.  The expected merged strings, qualities and offsets are
tests/merge_model.py's, never the device's; every reference of the GPU tests runs on those strings.

arena(name) -> dict:
  "mixed"        mode 2 with qualities, min_overlap 20: the correction tiers' and the quarter-wave layout's edge lengths, a spread
                 of lengths, runs of 1, 63, 64, 65 and 300 unmerged units, a run in front and one behind, no read above 1023 bases
  "mixed_fasta"  the same pairs without qualities (d_qual = d_mqual = NULL)
  "long"         mixed's pairs, three that merge to 1024, 1500 and 2045 bases and three unmerged ones, min_overlap 1
  "unmerged"     5 000 pairs with no acceptable offset: the merged arena is 5 000 NUL bytes"""
import functools

import numpy as np

import merge_model as mm
from seam_arena import canonical
from trim_cases import rand_qual, rand_seq, revcomp

K = 23
SEED = 20261021
GENOME_LEN = 40000
EDGE_LENGTHS = (K - 1, K, K + 1, 160, 161, 320, 321, 1023)
MORE_LONG = (400, 640)                       # more reads of the long correction tier than its two edges
RUNS = (1, 63, 64, 65, 300)
FIRST_RUN, LAST_RUN, LONG_LAST_RUN = 5, 7, 3
LONG_LENGTHS = (1024, 1500, 2045)
N_UNMERGED = 5000
PARAMS = {"mixed": mm.params(min_overlap=20), "mixed_fasta": mm.params(min_overlap=20), "long": mm.params(min_overlap=1), "unmerged": mm.params()}
Q_HIGH = 33 + 40


@functools.lru_cache(maxsize=None)
def genome():
    return rand_seq(np.random.default_rng(SEED), GENOME_LEN)


def _sub(s, p):
    return s[:p] + bytes([b"ACGT"[(b"ACGT".index(s[p]) + 1 + p % 3) % 4]]) + s[p + 1:]


def _setq(q, p, v):
    return q[:p] + bytes([33 + v]) + q[p + 1:]


def _merging_pair(rng, frag, errors, overlap=24):
    """(a, b, qa, qb) of a fragment whose mates overlap by `overlap` bases (by the whole fragment where it is shorter): qualities
    of Q25 to Q40; `errors` substitutions in the part mate 1 covers alone (they stay in the merged read, at Q8); in every third
    pair a disagreement inside the overlap at Q30 : Q30 (a tie: mate 1's wrong base at qual_base + 2) or at Q5 : Q38 (mate 2's
    right base wins); and two positions of the overlap at Q40 + Q40 (the cap)"""
    F = len(frag)
    L = min(F, (F + overlap + 1) // 2)
    a, b = frag[:L], revcomp(frag)[:L]
    qa, qb = rand_qual(rng, L, 25, 40), rand_qual(rng, L, 25, 40)
    d = F - L                                     # mate 1 alone: [0, d); both: [d, L); mate 2 alone: [L, F)
    for p in sorted(set(int(x) for x in rng.integers(0, max(d, 1), errors))) if d > 0 else []:
        a, qa = _sub(a, p), _setq(qa, p, 8)
    if L - d >= 20:
        for p in (d + 3, d + 11):                 # position p of the fragment is base F - 1 - p of mate 2
            qa, qb = _setq(qa, p, 40), _setq(qb, F - 1 - p, 40)
        kind = int(rng.integers(0, 3))
        if kind:
            p = d + 7
            a = _sub(a, p)
            qa, qb = (_setq(qa, p, 30), _setq(qb, F - 1 - p, 30)) if kind == 1 else (_setq(qa, p, 5), _setq(qb, F - 1 - p, 38))
    return a, b, qa, qb


def _unmerged_pair(i):
    """mates that face each other with no agreeing base at any offset (poly-A against poly-A: mate 2 reads as poly-T), or empty"""
    a, b = (b"", b"") if i % 5 == 4 else (b"A" * (i % 13), b"A" * ((7 * i) % 11))
    return a, b, bytes([Q_HIGH]) * len(a), bytes([Q_HIGH]) * len(b)


def _cut(rng, F):
    p = int(rng.integers(0, GENOME_LEN - F + 1))
    return genome()[p:p + F]


@functools.lru_cache(maxsize=None)
def mixed_units():
    """[(kind, fragment or None, (a, b, qa, qb))] in arena order; kind: "run" (unmerged), "frag" (cut from the genome), "foreign"
    (a fragment the genome does not hold: every window of the merged read is weak, and no correction can help)"""
    rng = np.random.default_rng(SEED + 1)
    units, n_run = [], [0]

    def run(n):
        for _ in range(n):
            units.append(("run", None, _unmerged_pair(n_run[0])))
            n_run[0] += 1

    def frag(F, errors=None):
        f = _cut(rng, F)
        errors = (1 + F // 300 if rng.random() < 0.7 else 0) if errors is None else errors
        units.append(("frag", f, _merging_pair(rng, f, errors)))

    run(FIRST_RUN)
    for _ in range(17):                           # 33 bytes each: the merged reads behind them start at every residue of 16
        frag(32, 0)
    edges, runs = list(EDGE_LENGTHS), list(RUNS)
    for i, F in enumerate(edges):
        frag(F, 0 if F < 60 else 1 + F // 300)
        if i % 2 == 0 and runs:
            run(runs.pop(0))
        elif i == len(edges) - 1:
            run(runs.pop())
    frag(100)
    while runs:
        run(runs.pop(0))
        frag(120)
    for i, F in enumerate(rng.integers(40, 301, 70)):
        frag(int(F))
        if i % 9 == 4:
            frag(45)
            run(2 + i % 2)
    for F in MORE_LONG:
        frag(F, 3)
    fr = np.random.default_rng(SEED + 2)
    for F in (90, 200):
        f = rand_seq(fr, F)
        units.append(("foreign", f, _merging_pair(fr, f, 0)))
    run(LAST_RUN)
    return tuple(units)


def _quiet_ends(a, b, n=12):
    """no overlap of 2 .. n bases, at either end, on which the mates agree throughout: what would beat an overlap of one base"""
    r = revcomp(b)
    return all(a[len(a) - v:] != r[:v] and a[:v] != r[len(r) - v:] for v in range(2, n + 1))


@functools.lru_cache(maxsize=None)
def long_units():
    """the pairs that merge to LONG_LENGTHS: mates of 600, 1000 and 1023 bases under min_overlap 1"""
    rng = np.random.default_rng(SEED + 3)
    units = []
    for F, L in zip(LONG_LENGTHS, (600, 1000, 1023)):
        while True:
            f = _cut(rng, F)
            a, b = f[:L], revcomp(f)[:L]
            if 2 * L - F > 12 or _quiet_ends(a, b):
                break
        units.append(("frag", f, (a, b, rand_qual(rng, L, 25, 40), rand_qual(rng, L, 25, 40))))
    return tuple(units)


@functools.lru_cache(maxsize=None)
def unmerged_units():
    """N_UNMERGED pairs with no acceptable offset under the default parameters: most with a mate below min_overlap (empty ones
    among them), every tenth unrelated random mates of 40 to 80 bases"""
    rng = np.random.default_rng(SEED + 4)
    units = []
    for i in range(N_UNMERGED):
        if i % 10 == 3:
            a, b = rand_seq(rng, int(rng.integers(40, 81))), rand_seq(rng, int(rng.integers(40, 81)))
        else:
            a, b = rand_seq(rng, i % 30), rand_seq(rng, (i * 7) % 61)
        units.append(("run", None, (a, b, rand_qual(rng, len(a)), rand_qual(rng, len(b)))))
    return tuple(units)


def long_tail():
    """the unmerged units behind long's last read"""
    return tuple(("run", None, _unmerged_pair(i)) for i in range(LONG_LAST_RUN))


def units_of(name):
    return {"mixed": mixed_units, "mixed_fasta": mixed_units, "unmerged": unmerged_units, "long": lambda: mixed_units() + long_units() + long_tail()}[name]()


@functools.lru_cache(maxsize=None)
def arena(name):
    """the pairs of an arena as read_merge_device takes them (mode 2) and merge_model's answer: {"seqs", "quals" (None: FASTA),
    "p", "max_read_len" (of the mates), "want": (rows, moff, mseq, mqual, tally), "strings", "qstrings" (None: FASTA): the merged
    reads, "max_len": the longest of them}"""
    units = units_of(name)
    seqs = [m for _, _, (a, b, _, _) in units for m in (a, b)]
    quals = None if name == "mixed_fasta" else [m for _, _, (_, _, qa, qb) in units for m in (qa, qb)]
    p = PARAMS[name]
    want = mm.merge_batch(seqs, quals, 2, p)
    moff, n = want[1], len(units)
    strings = [want[2][moff[u]:moff[u + 1] - 1] for u in range(n)]
    qstrings = None if quals is None else [want[3][moff[u]:moff[u + 1] - 1] for u in range(n)]
    assert [len(s) for s in strings] == want[0][:, 0].tolist()
    return dict(name=name, seqs=seqs, quals=quals, p=p, max_read_len=max(len(s) for s in seqs), want=want, strings=strings, qstrings=qstrings,
                max_len=max(len(s) for s in strings))


def runs_of_empty(strings):
    """the lengths of the maximal runs of empty reads, in arena order"""
    out, n = [], 0
    for s in list(strings) + [b"x"]:
        if s:
            if n:
                out.append(n)
            n = 0
        else:
            n += 1
    return out


def fragments(which="all"):
    """the error-free fragments cut from the genome, mixed's and long's; "half": every second one (the screen set)"""
    f = [u[1] for u in mixed_units() + long_units() if u[0] == "frag"]
    return f[0::2] if which == "half" else f


@functools.lru_cache(maxsize=None)
def table_counts(which="all"):
    """{canonical code: count} of the 23-mers of the error-free fragments, fragment i counted 20 + i % 15 times: as if every
    fragment had been sequenced that deep without an error"""
    counts = {}
    for i, f in enumerate(fragments(which)):
        for j in range(len(f) - K + 1):
            c = canonical(f[j:j + K])
            counts[c] = counts.get(c, 0) + 20 + i % 15
    return counts


def table_arrays(which="all"):
    c = table_counts(which)
    codes = np.array(sorted(c), dtype=np.uint64)
    return codes, np.array([c[int(x)] for x in codes], dtype=np.int32)


def strings_counts(strings):
    """{canonical code: occurrences} of the valid windows of the merged reads: what a counter kept from 1 on holds"""
    acgt, d = frozenset(b"ACGT"), {}
    for s in strings:
        for i in range(len(s) - K + 1):
            if acgt.issuperset(s[i:i + K]):
                c = canonical(s[i:i + K])
                d[c] = d.get(c, 0) + 1
    return d


@functools.lru_cache(maxsize=None)
def error_rate():
    """the oracle's ERROR_RATE estimate for the table (main.cpp:310-358), from the table written as a dump"""
    import os
    import tempfile

    import synth
    from oracle import pyoracle as po
    po.build()
    codes, counts = table_arrays()
    T = po.Table(K, len(codes))
    T.put_many(codes, counts)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "table.jf")
        synth.write_dump(path, codes, counts, K)
        return T.error_rate(path)


def dataset(name):
    """the merged reads of an arena as the single-end data set dict datasets.run_oracle takes; FASTA: quality bytes of 0"""
    a = arena(name)
    codes, counts = table_arrays()
    quals = a["qstrings"] if a["qstrings"] is not None else [b"\0" * len(s) for s in a["strings"]]
    return dict(k=K, mfk=4, rate=error_rate(), mode=0, keys=codes, counts=counts, seqs1=a["strings"], quals1=quals, seqs2=None, quals2=None)


@functools.lru_cache(maxsize=None)
def oracle_want(name):
    """(strong, ret, l, m, h, corrected strings) of the oracle on the merged reads"""
    import datasets
    from oracle import pyoracle as po
    po.build()
    d = dataset(name)
    T = po.Table(K, len(d["keys"]))
    T.put_many(d["keys"], d["counts"])
    P = po.make_params(K, d["mfk"], d["rate"], b"H")
    strong = np.array([po.strong_threshold(P, T, s) for s in d["seqs1"]], dtype=np.int32)
    ret, l, m, h, bases = datasets.run_oracle(po, d)
    return strong, ret, l, m, h, po.unpack_reads(bases, po.pack_reads(d["seqs1"])[1])
