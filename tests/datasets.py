"""Seeded synthetic data sets shared by the CPU and GPU parity tests (tools/synth.py, synth-v1)."""
import numpy as np

import synth

# name -> (k, max_fix_per_k, error_rate, synth kwargs, mode) ; mode 0 single, 1 paired, 2 interleaved
CONFIGS = {
    "se_k23": dict(k=23, mfk=4, rate=0.01, mode=0, kw=dict(seed=101, n=3000, length=100, e=0.01)),
    "pe_k23": dict(k=23, mfk=4, rate=0.01, mode=1, kw=dict(seed=102, n=1500, length=150, e=0.005, paired=True)),
    "il_k23": dict(k=23, mfk=4, rate=0.01, mode=2, kw=dict(seed=103, n=1500, length=150, e=0.005, paired=True)),
    "k31_mc8": dict(k=31, mfk=8, rate=0.01, mode=0, kw=dict(seed=104, n=1500, length=150, e=0.05)),
    "skew": dict(k=23, mfk=4, rate=0.004, mode=0, kw=dict(seed=105, n=3000, length=150, e=0.005, alpha=1.5, bias3=True)),
    "nrich": dict(k=23, mfk=4, rate=0.01, mode=0, kw=dict(seed=107, n=3000, length=100, e=0.01, p_n=0.01)),
    "varlen": dict(k=23, mfk=4, rate=0.01, mode=0, kw=dict(seed=108, n=3000, length=100, e=0.02, var_len=True)),
    "k15": dict(k=15, mfk=4, rate=0.01, mode=0, kw=dict(seed=109, n=2000, length=75, e=0.01, n_tx=50)),
    "k32": dict(k=32, mfk=4, rate=0.01, mode=0, kw=dict(seed=110, n=2000, length=150, e=0.01)),
    "long300": dict(k=23, mfk=4, rate=0.01, mode=0, kw=dict(seed=112, n=400, length=300, e=0.01, n_tx=20, l_tx=1500)),
    "long600_k31": dict(k=31, mfk=4, rate=0.01, mode=1, kw=dict(seed=113, n=150, length=600, e=0.01, n_tx=10, l_tx=1500, paired=True)),
    "max1023": dict(k=23, mfk=4, rate=0.01, mode=0, kw=dict(seed=114, n=80, length=1023, e=0.008, n_tx=4, l_tx=1500, var_len=True)),
    "k11": dict(k=11, mfk=4, rate=0.01, mode=0, kw=dict(seed=115, n=1500, length=60, e=0.01, n_tx=6, l_tx=300)),
    "pe_var": dict(k=23, mfk=4, rate=0.02, mode=1, kw=dict(seed=111, n=1500, length=120, e=0.03, paired=True, var_len=True, p_n=0.005)),
    # 129 k-mers per read: one more than eight count registers per lane hold (rc_quarter.h: the <9, 10> instances)
    "se_151": dict(k=23, mfk=4, rate=0.01, mode=0, kw=dict(seed=116, n=3000, length=151, e=0.01)),
    "pe_151": dict(k=23, mfk=4, rate=0.01, mode=1, kw=dict(seed=117, n=1500, length=151, e=0.006, paired=True)),
    # 146 k-mers per read: the <10, 10> instances
    "pe_160_k15": dict(k=15, mfk=4, rate=0.01, mode=1, kw=dict(seed=118, n=1200, length=160, e=0.006, paired=True, n_tx=60)),
}

# read lengths either side of every tier boundary of rc_api_batch.hip (k = 23: S <= 160 < M <= 278 < L), mates drawn independently
TIER_LENGTHS = [60, 100, 128, 150, 150, 150, 151, 151, 160, 161, 200, 250, 278, 279, 320, 321, 400]


def tier_reads(mode, seed=119, n=1800, k=23):
    """Mixed-length batches: most reads short, some either side of the length tiers, the two mates of a pair of different
    lengths more often than not (a unit is routed by its longer read)."""
    length = max(TIER_LENGTHS)
    s1, q1, s2, q2, _ = synth.make_reads(seed, n, length, e=0.008, paired=mode != 0, n_tx=12, l_tx=1500, frag_len=500)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    lens1 = rng.choice(TIER_LENGTHS, n)
    lens2 = rng.choice(TIER_LENGTHS, n)
    keys, cnt = synth.count_kmers([s1, s2], k, [lens1, lens2])
    r1 = [s1[i, :lens1[i]].tobytes() for i in range(n)]
    qq1 = [q1[i, :lens1[i]].tobytes() for i in range(n)]
    r2 = qq2 = None
    if mode != 0:
        r2 = [s2[i, :lens2[i]].tobytes() for i in range(n)]
        qq2 = [q2[i, :lens2[i]].tobytes() for i in range(n)]
    if mode == 2:
        r1 = [x for p in zip(r1, r2) for x in p]
        qq1 = [x for p in zip(qq1, qq2) for x in p]
        r2 = qq2 = None
    return dict(k=k, mfk=4, rate=0.01, mode=mode, keys=keys, counts=cnt, seqs1=r1, quals1=qq1, seqs2=r2, quals2=qq2)


def adversarial_reads(seed=7, n=600, length=100):
    """Edge cases the reference's screens and k-mer state machine care about (SURVEY §11 fx_edge):
    reads shorter than / equal to k, 6+ N, isolated N, IUPAC letters, poly-A/T tails, all-A."""
    rng = np.random.Generator(np.random.PCG64(seed))
    s1, q1, _, _, _ = synth.make_reads(seed, n, length, e=0.01)
    reads = [s1[i].tobytes() for i in range(n)]
    quals = [q1[i].tobytes() for i in range(n)]
    out_r, out_q = [], []
    for i, (r, q) in enumerate(zip(reads, quals)):
        r = bytearray(r)
        kind = i % 12
        if kind == 0:
            r = r[:int(rng.integers(1, 23))]
        elif kind == 1:
            r = r[:23]
        elif kind == 2:
            for p in rng.choice(length, 7, replace=False):
                r[p] = ord('N')
        elif kind == 3:
            r[int(rng.integers(0, length))] = ord('N')
        elif kind == 4:
            for p in rng.choice(length, 3, replace=False):
                r[p] = rng.choice(list(b"RYKMSWBDHV"))
        elif kind == 5:
            t = int(rng.integers(10, 60))
            r[length - t:] = b"A" * t
        elif kind == 6:
            t = int(rng.integers(10, 60))
            r[:t] = b"T" * t
        elif kind == 7:
            r = bytearray(b"A" * length)
        elif kind == 8:
            for p in range(40, 46):
                r[p] = ord("ACGT"[(b"ACGT".index(r[p]) + 1) % 4]) if r[p] in b"ACGT" else r[p]
        elif kind == 9:
            r[0] = ord('N')
            r[-1] = ord('N')
        elif kind == 10:
            r = r[:24 + int(rng.integers(0, 10))]
        q = bytes(q[:len(r)])
        out_r.append(bytes(r))
        out_q.append(q)
    return out_r, out_q


def polya_boundary_reads(k, seed=4242, n_tx=6, l_tx=400, cover=40, length=100):
    """Reads over transcripts that carry A-rich / T-rich stretches whose k-windows sit right at the two IsPolyA
    thresholds the path uses (ErrorCorrection.cpp:53-71): k - 2 A's or T's (the trusted mask, :870-931, and the veto on
    substitutions, :343 / :577) and k - max(7, k/2) (the mask of GetStrongTrustedThreshold, :1530-1541) -- windows with
    exactly the threshold count, one below and one above, for both letters; 0.5 % substitutions on top."""
    rng = np.random.Generator(np.random.PCG64(seed))
    thr7 = max(7, k // 2)
    txs = []
    for t in range(n_tx):
        tx = rng.integers(0, 4, l_tx).astype(np.uint8)
        letter = 0 if t % 2 == 0 else 3
        other = [c for c in range(4) if c != letter]
        pos = 40
        for want in (k - 2, k - 3, k - 1, k, k - thr7, k - thr7 - 1, k - thr7 + 1):
            w = np.full(k, letter, np.uint8)
            holes = rng.choice(k, k - want, replace=False)
            w[holes] = rng.choice(other, len(holes))
            tx[pos:pos + k] = w
            # (the windows around it hold fewer of the letter: the flanks are random)
            pos += k + 17
        txs.append(tx)
    reads, quals = [], []
    for tx in txs:
        for _ in range(cover * l_tx // length):
            a = int(rng.integers(0, l_tx - length + 1))
            r = tx[a:a + length].copy()
            e = rng.random(length) < 0.005
            r[e] = (r[e] + rng.integers(1, 4, int(e.sum()))) % 4
            if rng.random() < 0.5:
                r = (3 - r)[::-1]
            reads.append(np.frombuffer(b"ACGT", np.uint8)[r])
            quals.append(np.full(length, ord("I"), np.uint8))
    return np.stack(reads), np.stack(quals)


# ---- qv_*: reads on which the base qualities decide what the three closing vetoes of the correction do ----
# (pairwise veto, end-of-read veto, density veto: ErrorCorrection.cpp:1314-1466).  The sets above give every substituted base a
# quality below the threshold and every other base one above it, so no veto ever sees a fix on a high-quality base.  Here clean
# reads get bursts of substitutions shaped for one veto each, and the qualities come from a model of their own.

# the lengths of qv_lengths: either side of the 64-bit words of the veto masks, of the `len > 10` test, of end windows that
# overlap, and of the S / M / L tiers
QV_LENGTHS = [11, 12, 19, 20, 21, 63, 64, 65, 127, 128, 129, 160, 161, 191, 192, 193, 255, 256, 257, 278, 279, 320, 1023]
QV_MODELS = ("high", "inverted", "straddle", "fasta", "low", "signed")
_QV_SEED = {"pair": 8100, "ends": 8200, "dense": 8300, "mixed": 8400, "lengths": 8500, "signed": 8600}


def _substitute(rng, s, err, i, pos):
    for p in pos:
        s[i, p] = synth.NUC[(synth.CODE[s[i, p]] + int(rng.integers(1, 4))) & 3]
        err[i, p] = True


def _burst(rng, family, length, k, mfk):
    """The positions one read's substitutions go to (empty: the read stays clean)."""
    if family == "ends":
        # 2..4 in the first ten and / or the last ten bases, and singles in between (at least 12 bases apart) up to 4..6 in all
        if rng.random() >= 0.7:
            return []
        which = int(rng.integers(0, 3))
        pos = []
        if which != 1:
            pos += list(rng.choice(10, int(rng.integers(2, 5)), replace=False))
        if which != 0:
            pos += list(length - 10 + rng.choice(10, int(rng.integers(2, 5)), replace=False))
        want = max(4, len(pos)) + int(rng.integers(0, 3)) - len(pos)
        slots = rng.permutation(np.arange(16, length - 16, 12))[:want]
        return pos + [int(x) + int(rng.integers(0, 4)) for x in slots]
    if family == "dense":
        # mfk..mfk+3 inside one k-window, anywhere in the read (mfk = 1: 1..3, and 2 in three cases of five: with one fix per
        # window allowed, it is the window with two on which the weights decide)
        if rng.random() >= 0.7:
            return []
        m = int(rng.choice([1, 2, 2, 2, 3])) if mfk == 1 else int(rng.integers(mfk, mfk + 4))
        span = int(rng.integers(m, k + 1))
        a = int(rng.integers(0, length - span + 1))
        return list(a + rng.choice(span, m, replace=False))
    if family in ("mixed", "signed"):
        # 2..5 inside a span of 3..k+3 bases: 30 % at the 5' end, 30 % at the 3' end, the rest anywhere
        if rng.random() >= 0.6:
            return []
        m, where, span = int(rng.integers(2, 6)), rng.random(), int(rng.integers(3, k + 4))
        a = 0 if where < 0.3 else (length - span if where < 0.6 else int(rng.integers(0, length - span)))
        return list(a + rng.choice(span, min(m, span), replace=False))
    if family == "pair":
        return []   # (exactly the two substitutions of a minor haplotype: qv_reads)
    if family == "lengths":
        # 2..4 at each end (drawn separately, so end windows that overlap may share bases), and one more in the middle
        if length < 11 or rng.random() >= 0.9:
            return []
        pos = set(rng.choice(10, int(rng.integers(2, 5)), replace=False).tolist())
        pos |= set((length - 10 + rng.choice(10, int(rng.integers(2, 5)), replace=False)).tolist())
        if length > 40 and rng.random() < 0.5:
            pos.add(int(rng.integers(15, length - 15)))
        return sorted(pos)
    raise KeyError(family)


_QV_READS = {}
# per family: reads (mode 0) or pairs, transcripts, transcript length, share of the reads that carry a minor haplotype
_QV_SHAPE = {"pair": (1500, 8, 500, 0.2), "ends": (1500, 8, 500, 0.0), "dense": (1500, 8, 500, 0.0), "mixed": (1500, 8, 500, 0.06),
             "lengths": (600, 3, 1500, 0.2), "signed": (1000, 8, 500, 0.06)}


def qv_reads(family, k, mfk, mode, shape=None):
    """(seq arrays, error masks, lengths, keys, counts) of one qv_ family, with the exact counts of the reads' own k-mers as the
    table.  The reads are windows of a few deeply covered transcripts, either strand; the two mates of a pair are the two ends of
    a 300-base fragment and get their substitutions independently.  Two kinds of substitution:
      * a minor haplotype: every transcript has pairs of sites 2..k bases apart (an eighth of them k - 1 apart, the last distance
        at which one k-mer covers both, an eighth k apart, the first at which none does), a pair every 7 bases; a read
        that holds a pair at least 12 bases from either end carries, with the family's probability, other bases at both
        sites -- and its unit is then sequenced two or three times, as duplicates of a fragment are: same windows, same
        haplotypes.  So the minor k-mers have counts of 2 or 3, few enough to be distrusted and alike enough for the pairwise
        veto, which weighs the k-mers over one fix against those over both, to fire.  Substitutions drawn per read give
        k-mers nobody else has, and the veto never fires on them.
      * the family's burst (_burst), different in every read, duplicates included.
    shape: (units, transcripts, transcript length, share of minor haplotypes) in place of the family's own (_QV_SHAPE).
    Built once per argument tuple; nothing changes the arrays."""
    key = (family, k, mfk, mode, shape)
    if key in _QV_READS:
        return _QV_READS[key]
    rng = np.random.Generator(np.random.PCG64(_QV_SEED[family] + 37 * k + mfk + 1000 * mode))
    n, n_tx, l_tx, p_var = shape or _QV_SHAPE[family]
    if mfk == 1:
        n = 2000
    paired, frag = mode != 0, 300
    if paired:
        n //= 2
    mates = 2 if paired else 1
    tx = rng.integers(0, 4, size=(n_tx, l_tx), dtype=np.uint8)
    sites = [[] for _ in range(n_tx)]   # per transcript: (first site, second site)
    for t in range(n_tx):
        for a in range(8, l_tx - k - 1, 7):
            u = rng.random()
            dist = k - 1 if u < 0.125 else k if u < 0.25 else int(rng.integers(2, k + 1))
            sites[t].append((a, a + dist))
    # 1. the units: per mate (transcript, window start, reverse strand?, length, minor haplotype or None), each unit once, or
    #    two or three times where a mate carries a minor haplotype
    units = []
    while len(units) < n:
        t, rev = int(rng.integers(0, n_tx)), bool(rng.integers(0, 2))
        ulens = [int(rng.choice(QV_LENGTHS)) if family == "lengths" else 100 for _ in range(mates)]
        span = frag if paired else ulens[0]
        start = int(rng.integers(0, l_tx - span + 1))
        unit = []
        for j, ln in enumerate(ulens):
            rc = rev != (j == 1)
            ws = start + span - ln if rc and paired else start
            inner = [(a, b) for a, b in sites[t] if a - ws >= 12 and b - ws < ln - 12]
            minor = None
            if inner and rng.random() < p_var:
                a, b = inner[int(rng.integers(0, len(inner)))]
                minor = (a - ws, b - ws, (tx[t, a] + rng.integers(1, 4)) & 3, (tx[t, b] + rng.integers(1, 4)) & 3)
            unit.append((t, ws, rc, ln, minor))
        times = 1 + int(rng.integers(1, 3)) if any(m[4] is not None for m in unit) else 1
        units += [unit] * times
    units = units[:n]
    # 2. the reads of every unit, each with a burst of its own
    length = max(QV_LENGTHS) if family == "lengths" else 100
    lens = [np.array([u[j][3] for u in units]) for j in range(mates)]
    seqs = [np.full((n, length), ord("N"), np.uint8) for _ in range(mates)]
    errs = [np.zeros((n, length), bool) for _ in range(mates)]
    for i, unit in enumerate(units):
        for j, (t, ws, rc, ln, minor) in enumerate(unit):
            r = tx[t, ws:ws + ln].copy()
            e = np.zeros(ln, bool)
            if minor is not None:
                r[minor[0]], r[minor[1]] = minor[2], minor[3]
                e[minor[0]] = e[minor[1]] = True
            if rc:
                r, e = (3 - r)[::-1], e[::-1]
            seqs[j][i, :ln], errs[j][i, :ln] = synth.NUC[r], e
            _substitute(rng, seqs[j], errs[j], i, _burst(rng, family, ln, k, mfk))
    keys, cnt = synth.count_kmers(seqs, k, lens)
    for a in seqs + errs + lens + [keys, cnt]:
        a.setflags(write=False)
    _QV_READS[key] = (seqs, errs, lens, keys, cnt)
    return _QV_READS[key]


def qv_quals(model, err, thr, seed):
    """The quality bytes of one arena of reads.  high: all thr + 1.  inverted: thr + 1 on the substituted bases, thr on the
    others (the opposite of what the older sets do).  straddle: uniform in thr - 2 .. thr + 2, so a fifth of the bytes equal the
    threshold (capped at 127: as a signed char, what the comparison works on, 128 is the lowest value there is).  low: all equal
    to the threshold -- the control, on which no quality test is ever true.  fasta: none (qual[0] == 0).  signed: half the
    bytes are thr + 1 or thr + 2, the other half are uniform in 0x80 .. 0xFF, which are negative as signed chars and so below any threshold."""
    rng = np.random.Generator(np.random.PCG64(seed))
    if model == "high":
        return np.full(err.shape, thr + 1, np.uint8)
    if model == "inverted":
        return np.where(err, thr + 1, thr).astype(np.uint8)
    if model == "straddle":
        return rng.integers(thr - 2, min(127, thr + 2) + 1, err.shape).astype(np.uint8)
    if model == "low":
        return np.full(err.shape, thr, np.uint8)
    if model == "fasta":
        return np.zeros(err.shape, np.uint8)
    if model == "signed":
        q = rng.integers(thr + 1, thr + 3, err.shape)
        return np.where(rng.random(err.shape) < 0.5, rng.integers(0x80, 0x100, err.shape), q).astype(np.uint8)
    raise KeyError(model)


def qv_name(family, model, k=23, mfk=None, thr="H"):
    """qv_<family>[_k<k>][_mfk<m>][_q<threshold byte>]/<quality model>"""
    return "qv_%s%s%s%s/%s" % (family, "" if k == 23 else "_k%d" % k, "" if mfk is None else "_mfk%d" % mfk,
                               "" if thr == "H" else "_q%d" % ord(thr), model)


def _qv_names():
    """Each family with the quality models that make sense for it:
      * fasta only where minor haplotypes give the pairwise veto something to weigh (pair, mixed, lengths).  Without qualities the
        other two vetoes see no high-quality base at all, so the pairwise veto is the only one a missing quality array changes:
        on qv_ends and qv_dense, whose substitutions are drawn per read, it never fires, and a fasta member measured 0 to 3
        quality-dependent reads -- no such member can meet the floor of 30.
      * inverted only at k = 23, threshold 'H': it differs from high on the bases that are not substituted, which the vetoes
        look at only where the search proposes a wrong fix; one member per family pins that, qv_lengths (600 reads) has none.
      * qv_dense at max_fix_per_k 1, 3, 4, 5: high (every weight 2) and straddle (weights mixed, bytes on the threshold); the
        full set of models is on the max_fix_per_k = 2 member, the one that the alternative kernel paths run as well.
      * the other k and thresholds: high and straddle (qv_mixed_pe at other k: straddle), the two that differ most."""
    names = [qv_name(f, m) for f in ("pair", "mixed_pe", "mixed_il") for m in ("high", "inverted", "straddle", "fasta", "low")]
    names += [qv_name("ends", m) for m in ("high", "inverted", "straddle", "low")]
    names += [qv_name("dense", m, mfk=2) for m in ("high", "inverted", "straddle", "low")]
    names += [qv_name("dense", m, mfk=mfk) for mfk in (1, 3, 4, 5) for m in ("high", "straddle")]
    names += [qv_name("lengths", m) for m in ("high", "straddle", "fasta", "low")]
    for k in (11, 15, 25, 31, 32):
        names += [qv_name("pair", "high", k=k), qv_name("pair", "straddle", k=k), qv_name("mixed_pe", "straddle", k=k)]
    names += [qv_name("mixed_pe", m, thr=t) for t in "!~" for m in ("high", "straddle")]
    return names + ["qv_signed/signed"]


QV_NAMES = _qv_names()
# the high and inverted members of qv_pair, qv_ends, qv_dense and qv_mixed_*, at every k and threshold: at least 100 reads
# each on which the qualities decide (quality_dependent); at least 30 on every other set but the controls
QV_STRONG = [n for n in QV_NAMES if n.split("/")[1] in ("high", "inverted") and n.split("_")[1].split("/")[0] in ("pair", "ends", "dense", "mixed")]


def qv_make(name, shape=None):
    """shape: see qv_reads (a smaller instance of the same recipe, for a fixture)"""
    base, model = name.split("/")
    parts = base.split("_")[1:]
    opts = {p[0] if p[0] in "kq" else "mfk": int(p.lstrip("kmfq")) for p in parts if p[-1].isdigit()}
    family = [p for p in parts if not p[-1].isdigit()]
    mode = {"pe": 1, "il": 2}.get(family[-1], 0)
    family = family[0]
    k, thr = opts.get("k", 23), opts.get("q", ord("H"))
    mfk = opts.get("mfk", {"pair": 4, "ends": 8, "mixed": 4, "lengths": 4, "signed": 4}.get(family))
    seqs, errs, lens, keys, cnt = qv_reads(family, k, mfk if family == "dense" else 0, mode, shape)
    seed = _QV_SEED[family] + 37 * k + 7
    rows = [[s[i, :ln[i]].tobytes() for i in range(len(s))] for s, ln in zip(seqs, lens)]
    quals = [[q[i, :ln[i]].tobytes() for i in range(len(q))] for q, ln in
             zip([qv_quals(model, e, thr, seed + j) for j, e in enumerate(errs)], lens)]
    r1, q1, r2, q2 = rows[0], quals[0], None, None
    if mode == 1:
        r2, q2 = rows[1], quals[1]
    elif mode == 2:
        r1 = [x for p in zip(*rows) for x in p]
        q1 = [x for p in zip(*quals) for x in p]
    return dict(k=k, mfk=mfk, rate=0.01, mode=mode, keys=keys, counts=cnt, seqs1=r1, quals1=q1, seqs2=r2, quals2=q2,
                badq=bytes([thr]), fasta=model == "fasta", control=model == "low")


def with_quals(d, byte):
    """d with every quality byte set to `byte`"""
    flat = lambda rows: None if rows is None else [bytes([byte]) * len(r) for r in rows]
    return dict(d, quals1=flat(d["seqs1"]), quals2=flat(d["seqs2"]))


def quality_dependent(oracle, d, want=None):
    """The number of reads whose (ret, corrected bases) differ between d and the same reads with every quality byte set to the
    threshold -- that is, with no quality test of any veto ever true.  `want`: the oracle's results on d, where the caller has them."""
    want = run_oracle(oracle, d) if want is None else want
    flat = run_oracle(oracle, with_quals(d, d.get("badq", b"H")[0]))
    n_units = len(d["seqs1"])
    differ = want[0] != flat[0]
    for j, (a, b) in enumerate(zip(want[4:], flat[4:])):
        off = oracle.pack_reads(d["seqs1"] if j == 0 else d["seqs2"])[1].astype(np.int64)
        rows = np.add.reduceat((a != b).astype(np.int64), off[:-1]) > 0
        differ[j * n_units:(j + 1) * n_units] |= rows
    return int(differ.sum())


def for_cli(d, seed=8800):
    """d with the first and the last quality byte of every read redrawn so that the command-line tools, which derive the
    threshold from exactly these bytes (main.cpp:88-128: the lower of the 5 % point of the first bytes, less one, and the 5 %
    point of the last bytes), arrive at the data set's own threshold: first bytes thr + 4, last bytes uniform in thr .. thr + 2.
    Left alone, a set whose bytes all lie within two of the threshold gets a threshold below every one of them."""
    if d.get("fasta", False):
        return d
    rng = np.random.Generator(np.random.PCG64(seed))
    thr = d["badq"][0]
    redraw = lambda quals: None if quals is None else [bytes([thr + 4]) + q[1:-1] + bytes([thr + int(rng.integers(0, 3))]) for q in quals]
    return dict(d, quals1=redraw(d["quals1"]), quals2=redraw(d["quals2"]))


def write_cli_case(d, path, units=None):
    """Data set d (its first `units` reads or pairs) as input files of the command-line tools in directory `path`: dump.jf and
    reads.fq / reads_1.fq + reads_2.fq / reads_il.fq (reads.fa for a set without qualities).  Returns the arguments, -maxcorK as
    the data set says; the tools derive the quality threshold from the reads themselves."""
    import os
    synth.write_dump(os.path.join(path, "dump.jf"), d["keys"], d["counts"], d["k"])
    fasta = d.get("fasta", False)

    def put(name, seqs, quals, tag=lambda i: b""):
        with open(os.path.join(path, name), "wb") as f:
            for i, (s, q) in enumerate(zip(seqs, quals)):
                f.write(b">r%d%s\n%s\n" % (i, tag(i), s) if fasta else b"@r%d%s\n%s\n+\n%s\n" % (i, tag(i), s, q))
    ext = "fa" if fasta else "fq"
    if d["mode"] == 1:
        put("reads_1." + ext, d["seqs1"][:units], d["quals1"][:units], lambda i: b"/1")
        put("reads_2." + ext, d["seqs2"][:units], d["quals2"][:units], lambda i: b"/2")
        args = ["-p", "reads_1." + ext, "reads_2." + ext]
    elif d["mode"] == 2:
        n = None if units is None else 2 * units
        put("reads_il." + ext, d["seqs1"][:n], d["quals1"][:n], lambda i: b"/%d" % (i % 2 + 1))
        args = ["-i", "reads_il." + ext]
    else:
        put("reads." + ext, d["seqs1"][:units], d["quals1"][:units])
        args = ["-r", "reads." + ext]
    return args + ["-k", str(d["k"]), "-c", "dump.jf", "-maxcorK", str(d["mfk"])]


def make(name):
    """Returns dict(k, mfk, rate, mode, keys, counts, seqs1, quals1, seqs2, quals2) as python bytes lists; the qv_ sets also carry
    their threshold byte (badq)."""
    if name.startswith("qv_"):
        return qv_make(name)
    if name.startswith("huge_"):
        return huge_make(name)
    if name.startswith("polya_k"):
        k = int(name[len("polya_k"):])
        s1, q1 = polya_boundary_reads(k)
        keys, cnt = synth.count_kmers([s1], k)
        return dict(k=k, mfk=4, rate=0.0041, mode=0, keys=keys, counts=cnt, seqs1=[r.tobytes() for r in s1],
                    quals1=[q.tobytes() for q in q1], seqs2=None, quals2=None)
    if name in ("tiers_se", "tiers_pe", "tiers_il"):
        return tier_reads({"se": 0, "pe": 1, "il": 2}[name[-2:]])
    if name == "edge":
        r, q = adversarial_reads()
        s1, _, _, _, _ = synth.make_reads(7, 600, 100, e=0.01)
        keys, cnt = synth.count_kmers([s1], 23)
        return dict(k=23, mfk=4, rate=0.01, mode=0, keys=keys, counts=cnt, seqs1=r, quals1=q, seqs2=None, quals2=None)
    c = CONFIGS[name]
    kw = dict(c["kw"])
    seed, n, length = kw.pop("seed"), kw.pop("n"), kw.pop("length")
    s1, q1, s2, q2, lens = synth.make_reads(seed, n, length, **kw)
    keys, cnt = synth.count_kmers([s1, s2], c["k"], [lens, lens] if lens is not None else None)

    def rows(a):
        if a is None:
            return None
        return [a[i, :(length if lens is None else lens[i])].tobytes() for i in range(len(a))]
    r1, qq1, r2, qq2 = rows(s1), rows(q1), rows(s2), rows(q2)
    if c["mode"] == 2:
        r1 = [x for p in zip(r1, r2) for x in p]
        qq1 = [x for p in zip(qq1, qq2) for x in p]
        r2 = qq2 = None
    return dict(k=c["k"], mfk=c["mfk"], rate=c["rate"], mode=c["mode"], keys=keys, counts=cnt,
                seqs1=r1, quals1=qq1, seqs2=r2, quals2=qq2)


def revcomp_codes(codes, k):
    """reverse complement of 2-bit k-mer codes (KmerCode.h:58-71), vectorised"""
    out = np.zeros_like(codes)
    c = codes.copy()
    for _ in range(k):
        out = (out << np.uint64(2)) | (np.uint64(3) - (c & np.uint64(3)))
        c = c >> np.uint64(2)
    return out


def pad_table(keys, cnt, k, pad_to, seed):
    """(keys, counts) padded to pad_to entries with canonical k-mers that are not among `keys` (counts 2..199): a table of the
    size -- and so the layout and the compiled-for-k kernel instance -- of a real one, which changes no read's k-mer counts."""
    if pad_to <= len(keys):
        return keys, cnt
    rng = np.random.Generator(np.random.PCG64(seed))
    mask = np.uint64((1 << (2 * k)) - 1) if k < 32 else np.uint64(0xFFFFFFFFFFFFFFFF)
    fwd = rng.integers(0, 1 << 63, size=pad_to + pad_to // 8, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=pad_to + pad_to // 8, dtype=np.uint64)
    fwd &= mask
    pad = np.unique(np.minimum(fwd, revcomp_codes(fwd, k)))
    pad = rng.permutation(pad[~np.isin(pad, keys)])[:pad_to - len(keys)]
    assert len(keys) + len(pad) == pad_to, "k = %d has too few k-mers to pad a table to %d entries" % (k, pad_to)
    return np.concatenate([keys, pad]), np.concatenate([cnt, rng.integers(2, 200, size=len(pad)).astype(np.int64)])


def k_sweep(k, mode, pad_to=0):
    """The k sweep's data set (tests/test_k_sweep.py): 600 reads (mode 1: pairs) of 100 bases over six transcripts of 400,
    1 % substitutions, the exact counts of their own k-mers as the table.  With pad_to > 0 the table is padded to that many
    entries with canonical k-mers that no read holds (counts 2..199), so that it has the size -- and so the layout and the
    compiled-for-k kernel instance -- of a real one; the oracle gets the same padded table."""
    s1, q1, s2, q2, _ = synth.make_reads(7100 + k, 600, 100, n_tx=6, l_tx=400, e=0.01, paired=mode == 1)
    keys, cnt = synth.count_kmers([s1, s2], k)
    keys, cnt = pad_table(keys, cnt, k, pad_to, 9100 + k)

    def rows(a):
        return None if a is None else [r.tobytes() for r in a]
    return dict(k=k, mfk=4, rate=0.01, mode=mode, keys=keys, counts=cnt, seqs1=rows(s1), quals1=rows(q1), seqs2=rows(s2), quals2=rows(q2))


# ---- huge_*: the k sweep's reads over tables whose counts do not fit a PACKED slot's count field ----
# A PACKED slot keeps a count in 27 - ext bits; the all-ones value is the mark of a count kept in full in the table's prefix
# (rc_common.h: RC_PACKED_OVF_MAX), so with limit = 2^(27 - ext) the counts up to limit - 2 are inline and those from limit - 1
# (the mark's own value) on overflow.  The second cliff is RC_BOUND_STEPS = 65536: a threshold t >= 65536 is beyond the table
# of GetBound's steps (rc_bs_lookup gives "not known").  Regime A keeps every threshold below it, regime B (rate 0.01) does not.
RC_PACKED_OVF_MAX = 4000
RC_BOUND_STEPS = 65536
INT_MAX = (1 << 31) - 1
# member -> k, mode, entries the table is padded to, regime A's rate; `fallback`: more than RC_PACKED_OVF_MAX counts overflow
HUGE = {
    "huge_k23_ext0": dict(k=23, mode=0, pad_to=30_000, rate_a=1e-5),
    "huge_k27_ext8": dict(k=27, mode=1, pad_to=26_400, rate_a=1e-3),
    "huge_k23_small": dict(k=23, mode=0, pad_to=0, rate_a=1e-5),
    "huge_k31_wide": dict(k=31, mode=2, pad_to=0, rate_a=1e-5),
    "huge_k23_fallback": dict(k=23, mode=0, pad_to=30_000, rate_a=1e-5, fallback=True),
}
HUGE_NAMES = ["%s/%s" % (m, r) for m in HUGE for r in "AB"]
HUGE_FALLBACK_PADS = 2200


def packed_rule(k, n, load=0.4):
    """(ext, home buckets) of the PACKED attempt the build makes for n entries (rc_table.hip:
    rc_build_table_from_device_pairs): n / (4 slots * load) + 1 home buckets, at least 64, and the smallest ext with
    buckets << ext >= 2^(2k-32).  The attempt is made while ext <= 8 and stands while at most RC_PACKED_OVF_MAX counts
    overflow; otherwise the table is WIDE."""
    b = max(64, int(n / (4 * load)) + 1)
    ext = 0
    while 2 * k > 32 and (b << ext) < (1 << (2 * k - 32)):
        ext += 1
    return ext, b


def huge_overflowing(counts, ext):
    """how many counts a PACKED table with `ext` extension bits keeps in its prefix"""
    return int((np.asarray(counts, dtype=np.int64) >= (1 << (27 - ext)) - 1).sum())


_HUGE = {}


def huge_make(name):
    """huge_<member>/<regime>: k_sweep's reads (600 reads or pairs of 100 bases), every count of the reads' own k-mers multiplied
    by S = min(limit // 8, INT_MAX // largest count) -- the k-mers seen 8 times or more overflow, the error k-mers (2..3) stay
    inline -- the padding left alone, and four true k-mers (seen 8 times or more) pinned to limit - 2 (the largest inline
    count), limit - 1 (the mark's own value), limit and, without extension bits, INT_MAX.  limit = 2^(27 - ext) of the PACKED
    table the build makes for the member's size; huge_k31_wide would need more than 8 extension bits and is WIDE, and takes the
    limit of a count field without any (it is the member that has INT_MAX in a WIDE slot).  The fall-back member: S = limit // 4,
    so that the counts of 4 or more overflow too, and HUGE_FALLBACK_PADS padding k-mers beyond the limit: more counts than the
    prefix holds, the build has to fall back to WIDE by itself.  The dict also carries ext, limit, scale, the pinned
    (code, count) pairs and the unscaled counts (base_counts)."""
    member, regime = name.split("/")
    if member not in _HUGE:
        c = HUGE[member]
        k = c["k"]
        d = k_sweep(k, 1 if c["mode"] else 0, c["pad_to"])
        own = len(k_sweep(k, 1 if c["mode"] else 0)["keys"])   # (the padding comes behind the reads' own k-mers)
        base = np.asarray(d["counts"], dtype=np.int64)
        ext, _ = packed_rule(k, len(base))
        limit = 1 << (27 - (ext if ext <= 8 else 0))
        top = int(base[:own].max())
        scale = min(limit // (4 if c.get("fallback") else 8), INT_MAX // top)
        cnt = base.copy()
        cnt[:own] *= scale
        pins = [limit - 2, limit - 1, limit] + ([INT_MAX] if ext == 0 or ext > 8 else [])
        deep = np.nonzero(base[:own] >= 8)[0]
        at = deep[np.linspace(0, len(deep) - 1, len(pins) + 2).astype(int)[1:-1]]
        cnt[at] = pins
        if c.get("fallback"):
            cnt[own:own + HUGE_FALLBACK_PADS] = limit + np.arange(HUGE_FALLBACK_PADS)
        assert cnt.max() <= INT_MAX and len(set(at.tolist())) == len(pins)
        if c["mode"] == 2:
            d = dict(d, mode=2, seqs1=[x for p in zip(d["seqs1"], d["seqs2"]) for x in p],
                     quals1=[x for p in zip(d["quals1"], d["quals2"]) for x in p], seqs2=None, quals2=None)
        cnt.setflags(write=False)
        base.setflags(write=False)
        _HUGE[member] = dict(d, counts=cnt, base_counts=base, own=own, ext=ext, limit=limit, scale=scale,
                             pinned=[(int(d["keys"][i]), int(v)) for i, v in zip(at, pins)], rate_a=c["rate_a"])
    d = _HUGE[member]
    return dict(d, rate=d["rate_a"] if regime == "A" else 0.01, regime=regime)


def run_oracle(po, d, threads=4, fn=None):
    """Runs the oracle (or any same-signature batch function) on data set d.
    Returns (ret, l, m, h, corrected_arena1[, corrected_arena2])."""
    T = po.Table(d["k"], len(d["keys"]))
    T.put_many(d["keys"], d["counts"])
    P = po.make_params(d["k"], d["mfk"], d["rate"], d.get("badq", b"H"))
    a, off = po.pack_reads(d["seqs1"])
    qa, _ = po.pack_reads(d["quals1"])
    if d["mode"] == 1:
        a2, off2 = po.pack_reads(d["seqs2"])
        qa2, _ = po.pack_reads(d["quals2"])
        res = po.correct_batch(P, T, 1, a, qa, off, a2, qa2, off2, threads=threads, fn=fn)
        return res + (a, a2)
    res = po.correct_batch(P, T, d["mode"], a, qa, off, threads=threads, fn=fn)
    return res + (a,)


def mason_style_reads(seed=11, n=300, length=100, n_tx=6, l_tx=500, e=0.02):
    """Simulated reads whose headers carry the truth the way the Mason simulator writes it and the
    reference's scorer parses it (verify.cpp:193-232,290-298): haplotype_infix= the true bases on
    the forward strand, edit_string= one letter per read base (M correct, E substituted),
    strand=forward|reverse, exp=high|medium|low|<other>, and for some reads trim=<n>.
    Returns (headers, reads, quals) as lists of bytes; the reads are what a sequencer would give
    (errors included).  Every transcript is covered deeply enough for the corrector to fix most
    substitutions."""
    rng = np.random.Generator(np.random.PCG64(seed))
    tx = synth.NUC[rng.integers(0, 4, size=(n_tx, l_tx), dtype=np.uint8)]
    heads, reads, quals = [], [], []
    for i in range(n):
        t = int(rng.integers(0, n_tx))
        st = int(rng.integers(0, l_tx - length + 1))
        fwd = tx[t, st:st + length].copy()
        rev = bool(rng.integers(0, 2))
        true_read = synth.COMP[fwd[::-1]] if rev else fwd
        m = rng.random(length) < e
        obs = true_read.copy()
        shift = rng.integers(1, 4, size=length, dtype=np.uint8)
        obs[m] = synth.NUC[(synth.CODE[true_read[m]] + shift[m]) & 3]
        edit = np.where(m, ord('E'), ord('M')).astype(np.uint8)
        q = np.where(m, ord('#'), ord('I')).astype(np.uint8)
        exp = [b"high", b"medium", b"low", b"none"][int(rng.integers(0, 4))]
        h = b"@sim.%09d contig=tx%d haplotype=0 length=%d orig_begin=%d strand=%s exp=%s haplotype_infix=%s edit_string=%s" % (
            i, t, length, st, b"reverse" if rev else b"forward", exp, fwd.tobytes(), edit.tobytes())
        if i % 17 == 0:
            h += b" trim=%d" % (i % 5)
        heads.append(h)
        reads.append(obs.tobytes())
        quals.append(q.tobytes())
    return heads, reads, quals


def write_mason_fastq(path, heads, reads, quals):
    with open(path, "wb") as f:
        for h, r, q in zip(heads, reads, quals):
            f.write(h + b"\n" + r + b"\n+\n" + q + b"\n")


def mason_indel_variants(heads, reads, quals):
    """The same reads as a trimming / indel-making corrector could return them: some cut short
    at the 3' end, some with a base dropped or inserted in the middle -- exercises the scorer's
    unequal-length alignment (verify.cpp:58-129) and its -noindel switch."""
    out_r, out_q = [], []
    for i, (r, q) in enumerate(zip(reads, quals)):
        if i % 5 == 1:
            r, q = r[:-3], q[:-3]
        elif i % 5 == 2:
            p = 20 + i % 50
            r, q = r[:p] + r[p + 1:], q[:p] + q[p + 1:]
        elif i % 5 == 3:
            p = 10 + i % 60
            r, q = r[:p] + b"G" + r[p:], q[:p] + b"I" + q[p:]
        out_r.append(r)
        out_q.append(q)
    return heads, out_r, out_q
