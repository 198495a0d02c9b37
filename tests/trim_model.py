"""The trimming contract (include/rcorrector_amd.h: rc_read_trim_device; rcorrector_amd/csrc/rc_trim.h) restated position by
position in plain Python: what k_read_trim, the host program tests/hostmath/read_trim.cpp and tools/read_trim are compared
with.  Nothing here packs words or runs lanes."""
import numpy as np

MAX_LEN = 1023
ACGT = b"ACGT"
COMP = {65: 84, 67: 71, 71: 67, 84: 65}     # of the upper-case bases
DEFAULTS = dict(qual_min=20, qual_base=33, adapter1=b"AGATCGGAAGAGC", adapter2=None, adapter_min=5, adapter_mm_pct=10, pair_overlap=True,
                pair_min_overlap=30, pair_mm_pct=10, min_len=20)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    if p["adapter2"] is None:
        p["adapter2"] = p["adapter1"]
    return p


def cut_quality(qual, L, qual_min, qual_base=33):
    """qual: the quality bytes (None: no qualities)"""
    if qual is None or qual_min == 0:
        return L
    S = [0] * (L + 1)
    for i in range(L - 1, -1, -1):
        S[i] = S[i + 1] + (qual_min - (qual[i] - qual_base))
    i0 = max([i for i in range(L) if S[i] < 0], default=-1)
    best = max(S[i] for i in range(i0 + 1, L + 1))
    return max(i for i in range(i0 + 1, L + 1) if S[i] == best)


def cut_adapter(seq, adapter, adapter_min, adapter_mm_pct):
    L, n = len(seq), len(adapter)
    if n == 0:
        return L
    for d in range(L):
        v = m = 0
        for i in range(d, min(L, d + n)):
            if seq[i] in ACGT:
                v += 1
                m += seq[i] != adapter[i - d]
        if v >= adapter_min and 100 * m <= adapter_mm_pct * v:
            return d
    return L


def pair_offset(a, b, min_overlap, mm_pct):
    """d* of the mate-overlap report over the bases as given, or None: the accepted offset with the largest v, then the smallest
    m, then the smallest d"""
    La, Lb = len(a), len(b)
    if La < min_overlap or Lb < min_overlap:
        return None
    r = [COMP.get(x, 0) for x in reversed(b)]       # (0: not a valid base)
    best = None
    for d in range(max(min_overlap - Lb, -(Lb - 1)), min(La - min_overlap, La - 1) + 1):
        v = m = 0
        for i in range(max(0, d), min(La, d + Lb)):
            if a[i] in ACGT and r[i - d]:
                v += 1
                m += a[i] != r[i - d]
        if v >= min_overlap and 100 * m <= mm_pct * v:
            key = (v, -m, -d)
            if best is None or key > best[0]:
                best = (key, d)
    return None if best is None else best[1]


def trim_unit(seqs, quals, p, lmax=MAX_LEN):
    """the rows (keep_len, cut_qual, cut_adapter, cut_pair) of a unit's mates (one or two), whether it is kept, and whether the
    pair has an accepted offset; quals: None or a quality string per mate; a mate is cut to lmax bases first"""
    seqs = [bytes(s[:lmax]) for s in seqs]
    cp = [len(s) for s in seqs]
    overlapping = False
    if len(seqs) == 2 and p["pair_overlap"]:
        d = pair_offset(seqs[0], seqs[1], p["pair_min_overlap"], p["pair_mm_pct"])
        if d is not None:
            overlapping = True
            La, Lb = cp
            cp = [min(La, d + Lb), min(Lb, Lb + d)]
    rows = []
    for mt, s in enumerate(seqs):
        L = len(s)
        cq = cut_quality(None if quals is None else quals[mt], L, p["qual_min"], p["qual_base"])
        ca = cut_adapter(s, p["adapter2"] if mt else p["adapter1"], p["adapter_min"], p["adapter_mm_pct"])
        rows.append((min(cq, ca, cp[mt]), cq, ca, cp[mt]))
    return rows, all(r[0] >= p["min_len"] for r in rows), overlapping


def units_of(n_reads, mode):
    """the reads of every unit, as the duplicate census's modes have them"""
    if mode == 0:
        return [(r,) for r in range(n_reads)]
    if mode == 1:
        return [(u, n_reads // 2 + u) for u in range(n_reads // 2)]
    return [(2 * u, 2 * u + 1) for u in range(n_reads // 2)]


def empty_tally():
    return {"reads": np.zeros(2, np.uint64), "cut_reads": np.zeros((2, 3), np.uint64), "bases_removed": np.zeros(2, np.uint64),
            "short_reads": np.zeros(2, np.uint64), "units": 0, "units_kept": 0, "pairs_overlapping": 0, "keep_hist": np.zeros((2, 1024), np.uint64)}


def trim_batch(seqs, quals, mode, p, lmax=MAX_LEN, tally=None):
    """rows (n_reads, 4) int32, keep (units,) uint8 and the tally (added to `tally` if given) of a batch of reads"""
    rows = np.zeros((len(seqs), 4), np.int32)
    units = units_of(len(seqs), mode)
    keep = np.zeros(len(units), np.uint8)
    t = empty_tally() if tally is None else tally
    for u, rds in enumerate(units):
        rr, kept, ovl = trim_unit([seqs[r] for r in rds], None if quals is None else [quals[r] for r in rds], p, lmax)
        keep[u] = kept
        t["units"] += 1
        t["units_kept"] += int(kept)
        t["pairs_overlapping"] += int(ovl)
        for mt, (r, row) in enumerate(zip(rds, rr)):
            rows[r] = row
            L = min(len(seqs[r]), lmax)
            t["reads"][mt] += 1
            for c in range(3):
                t["cut_reads"][mt, c] += int(row[1 + c] < L)
            t["bases_removed"][mt] += L - row[0]
            t["short_reads"][mt] += int(row[0] < p["min_len"])
            t["keep_hist"][mt, row[0]] += 1
    return rows, keep, t


def tally_equal(a, b):
    return all(np.array_equal(np.asarray(a[k], np.uint64), np.asarray(b[k], np.uint64)) for k in empty_tally())
