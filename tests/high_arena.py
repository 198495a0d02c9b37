"""Small batches placed high in a large arena: the windows tests/test_high_arena.py (GPU) runs the device entry points on and
tests/test_high_arena_cases.py (CPU) guards.

An arena entry point takes nbytes up to 2^32 - 1 and uint32 offsets, and none of them needs d_off[0] == 0: read r is the
NUL-terminated string at d_off[r], and d_off has n_reads + 1 entries.  So a *window* is a few hundred reads written where the
offsets are large -- across 2^31 (`mid`), or up to the arena's last byte (`top`) -- inside an allocation that is otherwise left
as it came.  Offsets are built in int64 and handed over as their uint32 bit pattern.

Nothing here imports torch until a device helper is called."""
import functools

import numpy as np

MID_NBYTES = (1 << 31) + 65536
TOP_NBYTES = (1 << 32) - 1                      # the largest size the library accepts
HALF = 1 << 31
TAIL_LENGTHS = (1022, 150, 33, 17, 16, 15, 14, 9, 5, 3, 1, 0)     # the last reads of `top`, in arena order
PAD = 64                                         # letters in front of and behind a window
TOP_LEADS = tuple(range(16))
MID_LEADS = (0, 5, 15)


def _window(name, reads, nbytes, first):
    """reads: byte strings; first: the arena byte the first read starts at"""
    lens1 = np.array([len(r) + 1 for r in reads], dtype=np.int64)
    off = first + np.concatenate([[0], np.cumsum(lens1)]).astype(np.int64)
    assert first >= PAD and int(off[-1]) <= nbytes, (name, first, int(off[-1]), nbytes)
    assert all(0 not in r for r in reads)
    return {"name": name, "reads": list(reads), "off": off, "nbytes": nbytes, "max_len": int(lens1.max()) - 1}


def top(reads):
    """`reads` end with reads of TAIL_LENGTHS bases; the last read's NUL is the arena's last byte, byte 2^32 - 2"""
    assert tuple(len(r) for r in reads[-len(TAIL_LENGTHS):]) == TAIL_LENGTHS
    return _window("top", reads, TOP_NBYTES, TOP_NBYTES - sum(len(r) + 1 for r in reads))


def top_plain(reads):
    """any reads, the last one's NUL the arena's last byte: a read of full length ends where `top` has its empty read"""
    return _window("top plain", reads, TOP_NBYTES, TOP_NBYTES - sum(len(r) + 1 for r in reads))


def mid_seam(reads, a):
    """read a's NUL is byte 2^31 - 1 and read a + 1 starts at byte 2^31 exactly"""
    w = _window("mid seam", reads, MID_NBYTES, HALF - sum(len(r) + 1 for r in reads[:a + 1]))
    assert w["off"][a + 1] == HALF and a + 1 < len(reads)
    return w


def mid_straddle(reads, s):
    """the bases of read s lie on both sides of byte 2^31, half of them on either"""
    assert len(reads[s]) >= 2
    w = _window("mid straddle", reads, MID_NBYTES, HALF - len(reads[s]) // 2 - sum(len(r) + 1 for r in reads[:s]))
    assert w["off"][s] < HALF < w["off"][s + 1] - 1
    return w


def off_bits(w):
    """the offsets as the uint32 bit pattern the library reads, in the int32 array the callers hand over; the round trip is exact"""
    u = w["off"].astype(np.uint64).astype(np.uint32)
    assert np.array_equal(u.astype(np.int64), w["off"])
    return u.view(np.int32)


def arena_bytes(strings):
    """the window's bytes: every string and a NUL"""
    return np.frombuffer(b"".join(bytes(s) + b"\0" for s in strings), dtype=np.uint8)


def tail_reads(make):
    return [make(L) for L in TAIL_LENGTHS]


# ---- the device side ---------------------------------------------------------------------------------------------------------
def allocate():
    """an uninitialised device buffer that holds an arena of TOP_NBYTES bytes at any lead in 0..15 behind its 16-byte aligned
    start, every 16-byte piece that holds one of the arena's bytes included"""
    import torch
    buf = torch.empty(((TOP_NBYTES + 16 + 15) // 16 * 16,), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf


def put(buf, lead, w, strings=None):
    """writes the window's reads (or `strings`, as long as the reads: qualities, a corrected version) into the arena that starts
    `lead` bytes into buf, PAD letters in front of them and behind them (as far as buf goes); returns the arena's address"""
    import torch
    strings = w["reads"] if strings is None else strings
    assert [len(s) for s in strings] == [len(r) for r in w["reads"]]
    data = arena_bytes(strings)
    first, end = int(w["off"][0]), int(w["off"][-1])
    assert data.size == end - first and 0 <= lead < 16 and lead + w["nbytes"] <= buf.numel()
    buf[lead + first - PAD:lead + first] = ord("A")
    buf[lead + first:lead + end] = torch.from_numpy(data.copy()).cuda()
    buf[lead + end:min(lead + end + PAD, buf.numel())] = ord("A")
    return buf.data_ptr() + lead


def off_tensor(w):
    import torch
    return torch.from_numpy(off_bits(w).copy()).cuda()


# ---- the batches: the existing edge batches in front, the tail reads behind them --------------------------------------------
def _substituted(s, p):
    return s[:p] + bytes([b"ACGT"[(b"ACGT".index(s[p]) + 1) % 4]]) + s[p + 1:]


@functools.lru_cache(maxsize=None)
def table_case():
    """the reads of tests/test_read_depth.py's synthetic arena (k = 23) and, behind them, the tail reads cut from its longest read,
    those of 9 bases or more with their third base substituted (their first windows are weak, at k = 23 and at k = 5); an even number of reads.  Returns (reads,
    {k: {canonical code: count}}): the k = 23 table is the data set's, the k = 5 table holds every 5-mer of the reads as often as it
    occurs in them."""
    from test_read_depth import synthetic
    from test_read_screen import counts_of_reads
    k, front, counts = synthetic()
    G = front[6]
    assert k == 23 and len(G) == 1023

    def make(L):
        s = G[7 * L % 97 if L < 900 else 1:][:L]
        return _substituted(s, 2) if L >= 9 else s
    reads = front + [front[11]] * (len(front) % 2) + tail_reads(make)
    assert len(reads) % 2 == 0
    return reads, {23: counts, 5: counts_of_reads(reads, 5)}


TABLE_MIN_COUNT = {23: 3, 5: 50}     # what the weak, screen and trust profiles call solid: some windows of the tail reads are, some are not
TABLE_MID = (("seam", 20), ("straddle", 6), ("straddle", 21))     # read 6: 1 023 bases and mate 1 of an interleaved pair; 21: 150 bases, mate 2


@functools.lru_cache(maxsize=None)
def trim_case():
    """tests/trim_cases.py's "pair offsets interleaved" and "lengths mode 2 max_read_len 1023" and the tail reads behind them, as
    interleaved pairs with qualities: (reads, quals, params).  Among the last eight reads, the pair of 16 and 15 bases is a
    fragment of 13 (the pair cut), the read of 14 ends with five bases of the adapter, and the read of 9 with low qualities."""
    import trim_cases as tc
    import trim_model as tm
    by_name = {s["name"]: s for s in tc.all_scenarios()}
    rng = np.random.default_rng(4294967295)
    a, b = by_name["pair offsets interleaved"], by_name["lengths mode 2 max_read_len 1023"]
    reads = list(a["seqs"])
    quals = [tc.rand_qual(rng, len(s), 10, 41) for s in reads]
    reads += b["seqs"]
    quals += b["quals"]
    tail = {L: tc.rand_seq(rng, L) for L in TAIL_LENGTHS}
    tail[1022], tail[150] = tc.pair_of(rng, 1100, 1022, 150)
    tail[16], tail[15] = tc.pair_of(rng, 13, 16, 15)
    tail[14] = tail[14][:9] + tc.AD[:5]
    tq = {L: tc.rand_qual(rng, L, 30, 41) for L in TAIL_LENGTHS}
    tq[9] = tq[9][:5] + bytes([33 + 2]) * 4
    reads += [tail[L] for L in TAIL_LENGTHS]
    quals += [tq[L] for L in TAIL_LENGTHS]
    assert len(reads) % 2 == 0
    return reads, quals, tm.params(min_len=16, pair_min_overlap=12)


TRIM_MID = (("seam", 7), ("straddle", 6), ("straddle", 7))     # reads 6 and 7: the mates of a fragment of 130 bases, 100 and 80 deep
TRIM_MID_HALVES = (("seam", 29), ("straddle", 3), ("straddle", 29))     # the same two reads where halves() puts them


def halves(x):
    """a list that goes with trim_case's reads in the order of mode 1: the twelve pairs of "pair offsets" are pairs again -- their
    first mates lead the first half, their second mates the second half -- and the tail reads stay where they are"""
    assert len(x) == 40 + len(TAIL_LENGTHS)
    return x[0:24:2] + x[24:38] + x[1:24:2] + x[38:]


def split(x):
    """a list that goes with trim_case's reads in the order of mode 1 with EVERY pair a pair again: all first mates, then all
    second mates.  The last read is still the empty one; the reads in front of it are the tail's second mates."""
    assert len(x) % 2 == 0
    return x[0::2] + x[1::2]


@functools.lru_cache(maxsize=None)
def overlap_case():
    """the reads of trim_case as the bases as read, and a corrected version of them: every third read of 20 bases or more with
    one base changed a third of the way in"""
    reads = trim_case()[0]
    after = [_substituted(s, len(s) // 3) if i % 3 == 0 and len(s) >= 20 and s[len(s) // 3] in b"ACGT" else s for i, s in enumerate(reads)]
    return reads, after


OVERLAP_MIN = 12


def windows(reads, mids):
    """the windows of a batch: `top`, then the `mid` ones named by mids, each with the leads it is run at"""
    out = [(top(reads), TOP_LEADS)]
    for kind, i in mids:
        out.append(((mid_seam if kind == "seam" else mid_straddle)(reads, i), MID_LEADS))
    return out


def pairs4(before, after, mode):
    """(a before, b before, a after, b after) of every pair, as the mate-overlap model takes them"""
    n = len(before)
    units = [(u, n // 2 + u) for u in range(n // 2)] if mode == 1 else [(2 * u, 2 * u + 1) for u in range(n // 2)]
    return [(before[i], before[j], after[i], after[j]) for i, j in units]


@functools.lru_cache(maxsize=None)
def correct_case():
    """the first 150 pairs of tests/datasets.py's il_k23 (interleaved, 150 bases, k = 23) as the data set dicts the oracle runs
    on: ("plain": those reads alone, so that a read of 150 bases ends at the arena's last byte; "tail": the tail reads, cut from
    the same reads, behind them)"""
    import datasets
    d = datasets.make("il_k23")
    seqs, quals = d["seqs1"][:300], d["quals1"][:300]
    long = b"".join(seqs[:8])
    tail = tail_reads(lambda L: long[:L] if L > 150 else seqs[L][:L])
    return {"plain": dict(d, seqs1=seqs, quals1=quals),
            "tail": dict(d, seqs1=seqs + tail, quals1=quals + [b"I" * len(t) for t in tail])}


# ---- one filled arena: a base batch of about 1 MiB tiled up to 2^32 - 1 bytes -------------------------------------------------
def _tiling(fixed, fillers):
    """(reps, f, B): `reps` copies of a distinct list of `fixed` bytes (NULs counted, the filler pair's two included) and f filler
    bases, f one of `fillers`, are a base batch of B bytes: about 1 MiB, an odd number, and such that whole copies of it leave 2 to
    2 048 bytes of an arena of 2^32 - 1 -- the longest such rest on offer"""
    pick = None
    for reps in range(51, 141, 2):
        for f in fillers:
            B = reps * (fixed + f)
            if B % 2 == 1 and 14 << 16 <= B <= 18 << 16 and 2 <= TOP_NBYTES % B <= 2048:
                if pick is None or TOP_NBYTES % B > TOP_NBYTES % pick[2]:      # (the longest padding read on offer)
                    pick = (reps, f, B)
    assert pick is not None
    return pick


def _tiled_case(reads, quals, reps, B):
    """the dict of a filled arena: the distinct list, its repeats, and the pair of N reads that takes the arena's last bytes"""
    rem = TOP_NBYTES % B
    tail = [b"N" * min(rem - 2, 1023), b"N" * (rem - 2 - min(rem - 2, 1023))]
    assert sum(len(r) + 1 for r in reads) * reps == B and (TOP_NBYTES // B) * B + sum(len(r) + 1 for r in tail) == TOP_NBYTES
    return dict(reads=reads, quals=quals, reps=reps, base_bytes=B, tiles=TOP_NBYTES // B, tail=tail, tail_quals=[b"I" * len(t) for t in tail])


@functools.lru_cache(maxsize=None)
def filled_case():
    """A list of distinct interleaved pairs -- 40 pairs of 37 to 250 bases cut from fragments (some overlap, some run into the
    adapter), the edge lengths of TAIL_LENGTHS, a filler pair -- repeated `reps` times is the base batch: `base_bytes` bytes, about
    1 MiB, an odd number (so every tile has another alignment modulo 16), chosen so that `tiles` copies of it leave 2 to 2 048
    bytes of an arena of 2^32 - 1: the last pair, reads of N of the exact length needed (a batch of pairs has an even number of
    reads, so the padding is a pair).  The models run once, on the distinct list; the expected rows of the arena are
    those, tiled."""
    import trim_cases as tc
    rng = np.random.default_rng(16777215)
    reads = []
    for i in range(40):
        La, Lb = (37, 250) if i == 0 else (250, 37) if i == 1 else (int(x) for x in rng.integers(37, 251, 2))
        reads += tc.pair_of(rng, int(rng.integers(30, 400)), La, Lb, tail=tc.AD)
    reads += [tc.rand_seq(rng, L) for L in TAIL_LENGTHS]
    reps, f, B = _tiling(sum(len(r) + 1 for r in reads) + 2, range(1024))      # (+ 2: the filler pair's NULs)
    reads += [tc.rand_seq(np.random.default_rng(f), f), b""]
    quals = [tc.rand_qual(rng, len(r), 2, 41) for r in reads]
    return _tiled_case(reads, quals, reps, B)


# ---- merging: the trimming batch with its qualities, and a filled arena most of which comes back out ---------------------------
@functools.lru_cache(maxsize=None)
def merge_case():
    """trim_case's reads and qualities as the pairs read_merge_device merges: (reads, quals, params).  The last pairs of `top`:
    1022 and 150 bases merge to 1100 (the wide instance), 16 and 15 to a read-through fragment of 13, 1 and 0 not at all."""
    import merge_model as mm
    reads, quals, _ = trim_case()
    return reads, quals, mm.params(min_overlap=12)


def _noisy(rng, a):
    """a with up to two of its bases substituted, as tests/test_read_merge.py's _noisy does"""
    a = bytearray(a)
    for j in set(rng.integers(0, len(a), int(rng.integers(0, 3))).tolist()):
        a[j] = b"ACGT"[(b"ACGT".index(a[j]) + 1) % 4]
    return bytes(a)


MERGE_FILLER_OVERLAP = (40, 41)     # the filler pair's mates overlap by one of these: the one that makes the merged byte count odd


@functools.lru_cache(maxsize=None)
def merge_filled_case():
    """filled_case's shape for read_merge_device: 40 distinct interleaved pairs of 150 to 250 bases, most of them cut from a
    fragment 30 to 45 bases shorter than the mates together (they merge, and most of the input comes back out), one in eight from
    a fragment of 30 to 140 bases with the adapter behind it (read-through), one in eight from a fragment too long to overlap;
    mate 1 with up to four bases substituted (_noisy, twice), so that the qualities decide bases.  Behind them the reads of
    TAIL_LENGTHS, a filler pair, `reps` copies and the pair of N reads, as in filled_case.  The filler pair merges: its length
    makes the base batch's byte count odd, its overlap the base batch's MERGED byte count (`base_out`), so every copy's input and
    output have another alignment modulo 16.  `want`: merge_model's (rows, moff, mseq, mqual, tally) of the distinct list in
    mode 2, `tail_want` those of the N pair; `params` the model's defaults."""
    import merge_model as mm
    import trim_cases as tc
    rng = np.random.default_rng(2147483647)
    p = mm.params()
    reads = []
    for i in range(40):
        La, Lb = (int(x) for x in rng.integers(150, 251, 2))
        F = int(rng.integers(30, 141)) if i % 8 == 3 else La + Lb + int(rng.integers(20, 200)) if i % 8 == 6 else La + Lb - int(rng.integers(30, 46))
        a, b = tc.pair_of(rng, F, La, Lb, tail=tc.AD)
        reads += [_noisy(rng, _noisy(rng, a)), b]
    reads += [tc.rand_seq(rng, L) for L in TAIL_LENGTHS]
    quals = [tc.rand_qual(rng, len(r), 2, 41) for r in reads]
    reps, f, B = _tiling(sum(len(r) + 1 for r in reads) + 2, range(200, 1024))
    out_fixed = int(mm.merge_batch(reads, quals, 2, p)[1][-1])
    ov = [v for v in MERGE_FILLER_OVERLAP if (out_fixed + f - v + 1) % 2 == 1][0]       # (the filler merges to f - ov bases and a NUL)
    reads += list(tc.pair_of(np.random.default_rng(f), f - ov, f - f // 2, f // 2))
    quals += [tc.rand_qual(rng, len(r), 2, 41) for r in reads[-2:]]
    c = _tiled_case(reads, quals, reps, B)
    want = mm.merge_batch(reads, quals, 2, p)
    assert want[0][-1].tolist() == [f - ov, f - f // 2 - ov, ov, 0] and int(want[1][-1]) == out_fixed + f - ov + 1
    return dict(c, params=p, want=want, base_out=reps * int(want[1][-1]), tail_want=mm.merge_batch(c["tail"], c["tail_quals"], 2, p))
