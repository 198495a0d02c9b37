"""The packed and the resident boundary's device side (rcorrector_amd/csrc/rc_transport.hip) restated in numpy: what the
kernels must compute, from the statements in that file's header and nothing else -- plus the generators of the arenas the tests
run them on and the choice of the sub-ranges tests/test_transport_kernels.py submits.  No GPU and no library in here."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", np.uint8)
_CODE = np.zeros(256, np.uint32)
_CODE[ord("C")], _CODE[ord("G")], _CODE[ord("T")] = 1, 2, 3
_IS_BASE = np.zeros(256, bool)
_IS_BASE[ACGT] = True
_SHIFTS = (30 - 2 * np.arange(16)).astype(np.uint32)
# what a read may hold besides ACGT: N, IUPAC codes, lower case (none of them a base to the packed codes)
OTHER = np.frombuffer(b"NRYKMSWBDHVnacgt", np.uint8)


def round16(n):
    return (int(n) + 15) // 16 * 16


def pack(arena):
    """(words, exc_pos, exc_chr): arena byte p at bits 30 - 2 (p & 15) of word p >> 4, A C G T = 0 1 2 3 and 0 for everything
    else (the NULs, the padding of the last word); the bytes that are neither a base nor a NUL as a list in ascending order."""
    arena = np.asarray(arena, np.uint8)
    pad = np.zeros(round16(arena.size), np.uint8)
    pad[:arena.size] = arena
    words = np.bitwise_or.reduce(_CODE[pad].reshape(-1, 16) << _SHIFTS, axis=1).astype(np.uint32)
    exc_pos = np.nonzero((arena != 0) & ~_IS_BASE[arena])[0].astype(np.uint32)
    return words, exc_pos, arena[exc_pos].copy()


def letters(words):
    """the sixteen letters of every packed word: 16 len(words) bytes"""
    b = np.asarray(words, np.uint32).astype(">u4").view(np.uint8)       # most significant byte first: bases 0..3, 4..7, ... of the words
    return ACGT[((b[:, None] >> np.array([6, 4, 2, 0], np.uint8)) & 3).reshape(-1)]


def unpack(words, nbytes, off, exc):
    """The byte arena of nbytes bytes: the letters of the codes, a NUL behind every read of `off`, then the exceptions
    exc = (positions, letters)."""
    arena = letters(words)[:nbytes].copy()
    off = np.asarray(off, np.int64)
    arena[off[1:] - 1] = 0
    arena[np.asarray(exc[0], np.int64)] = exc[1]
    return arena


def fixes_packed(words, exc_pos, after):
    """(positions ascending, letters): the positions whose byte in `after` is one of ACGT and differs from the letter of its
    packed code, and the exception positions whose byte is 'A' (code 0 is 'A': the packed codes cannot show that one).  The two
    sets never share a position."""
    after = np.asarray(after, np.uint8)
    was = letters(words)[:after.size]
    a = np.nonzero(_IS_BASE[after] & (after != was))[0]
    exc_pos = np.asarray(exc_pos, np.int64)
    b = exc_pos[after[exc_pos] == ord("A")]
    pos = np.concatenate([a, b])
    assert len(np.unique(pos)) == len(pos), "the model lists a position twice"
    pos.sort()
    return pos.astype(np.uint32), after[pos]


def fixes_bytes(orig, after):
    """(positions ascending, letters): every byte of `after` that differs from `orig`, with the new letter"""
    pos = np.nonzero(np.asarray(orig, np.uint8) != np.asarray(after, np.uint8))[0]
    return pos.astype(np.uint32), np.asarray(after, np.uint8)[pos]


# ---- arenas ------------------------------------------------------------------------------------------------------
def read_offsets(rng, nbytes, max_len=150, lone_nul=True):
    """Offsets of reads (bases + NUL) of random lengths that fill nbytes bytes exactly.  With lone_nul one of them is a 1-byte
    read -- a lone NUL -- wherever nbytes has room for it; the first and the last read hold a base where nbytes has room for
    that as well (position 0 and the byte in front of the final NUL are bases then)."""
    rest = int(nbytes)
    lone = lone_nul and rest >= 1
    rest -= 1 if lone else 0
    ends = []
    if rest >= 4:
        ends.append(int(rng.integers(2, min(max_len, rest - 2) + 1)))
        ends.append(int(rng.integers(2, min(max_len, rest - ends[0]) + 1)))
    elif rest >= 2:
        ends.append(rest)
    rest -= sum(ends)
    mid = []
    while rest:
        mid.append(int(rng.integers(1, min(max_len, rest) + 1)))
        rest -= mid[-1]
    if lone:
        mid.insert(int(rng.integers(0, len(mid) + 1)), 1)
    return np.concatenate([[0], np.cumsum(ends[:1] + mid + ends[1:])]).astype(np.uint32)


def random_arena(rng, off, exc_density=0.0, n_exc=None, forced_exc=True):
    """A byte arena over `off`: random bases, a NUL behind every read, and letters outside ACGT at a share exc_density of the
    base positions (1.0: every one -- an all-N arena) or at exactly n_exc of them.  With forced_exc and a density above 0 there is
    one at position 0, one in the last 16-byte word and one directly in front of a NUL, wherever those positions hold a base."""
    off = np.asarray(off, np.int64)
    nbytes = int(off[-1])
    arena = ACGT[rng.integers(0, 4, size=nbytes)]
    arena[off[1:] - 1] = 0
    bases = np.nonzero(arena != 0)[0]
    if n_exc is not None:
        at = rng.choice(bases, size=n_exc, replace=False)
    elif exc_density >= 1.0:
        at = bases
    else:
        at = bases[rng.random(bases.size) < exc_density]
        if exc_density > 0 and forced_exc and bases.size:
            lens = off[1:] - off[:-1]
            longer = np.nonzero(lens >= 2)[0]
            want = [0, int(bases[-1])] + ([int(off[longer[len(longer) // 2] + 1]) - 2] if longer.size else [])
            at = np.union1d(at, [p for p in want if arena[p] != 0])
    at = np.asarray(at, np.int64)
    arena[at] = OTHER[rng.integers(0, OTHER.size, size=at.size)]
    return arena


def other_base(rng, was):
    """for every letter of `was` (ACGT) another base"""
    return ACGT[(_CODE[was] + rng.integers(1, 4, size=np.size(was)).astype(np.uint32)) & 3]


def substitute(rng, arena, density, exc_mode="mixed", spoil=True):
    """What a correction could leave of `arena`: a share `density` of the bases replaced by another base (1.0: every base),
    and the letters outside ACGT treated by exc_mode -- "alone", "A" (all replaced by 'A'), "CGT" (all replaced by one of C G T)
    or "mixed" (the three in turn).  With spoil a few bases and exceptions become letters outside ACGT: never a fix."""
    arena = np.asarray(arena, np.uint8)
    after = arena.copy()
    bases = np.nonzero(_IS_BASE[arena])[0]
    exc = np.nonzero((arena != 0) & ~_IS_BASE[arena])[0]
    hit = bases if density >= 1.0 else bases[rng.random(bases.size) < density]
    after[hit] = other_base(rng, arena[hit])
    turn = {"alone": np.zeros(exc.size, int), "A": np.ones(exc.size, int), "CGT": np.full(exc.size, 2),
            "mixed": np.arange(exc.size) % 3}[exc_mode]
    after[exc[turn == 1]] = ord("A")
    cgt = exc[turn == 2]
    after[cgt] = ACGT[rng.integers(1, 4, size=cgt.size)]
    if spoil and density > 0:
        rest = np.setdiff1d(bases, hit)
        for pool in (rest, exc[turn == 0]):
            if pool.size:
                at = rng.choice(pool, size=min(3, pool.size), replace=False)
                after[at] = OTHER[rng.integers(0, OTHER.size, size=at.size)]
    return after


# ---- sub-ranges of kept arenas (the resident boundary) -----------------------------------------------------------------
def start_at_every_shift(off, lo=0):
    """{s: the first read i >= lo whose offset is s modulo 16}, for every s that occurs"""
    off = np.asarray(off, np.int64)
    found = {}
    for i in range(lo, len(off) - 1):
        found.setdefault(int(off[i] % 16), i)
        if len(found) == 16:
            break
    return found


def paired_cuts(off1, off2, lo=0):
    """Sixteen sub-batches [i, j) of a paired data set: the second mates' range starts at every shift s = off2[i] % 16, and the
    first mates' range is bytes_a = off1[j] - off1[i] long with bytes_a % 16 == (5 s + 3) % 16 -- all sixteen values -- by
    leaving out reads at the end.  {s: (i, j)}, for every s for which such a pair of reads exists."""
    off1, off2 = np.asarray(off1, np.int64), np.asarray(off2, np.int64)
    n = len(off1) - 1
    cuts = {}
    for s, i in start_at_every_shift(off2, lo).items():
        for j in range(n, i, -1):
            if (off1[j] - off1[i]) % 16 == (5 * s + 3) % 16:
                cuts[s] = (i, j)
                break
    return cuts
