"""A synthetic arena aimed at the seams of the kernels that walk an arena tile by tile (rc_device.h: rc_tile_stage and the window
cut of rc_common.h: rc_tile_window), and the canonical code its dictionary is keyed by.  Shared by tests/test_weak_profile.py
(k_weak_planes) and tests/test_probe_seams.py (k_probe, k_count_scan); pure Python and numpy, nothing from the library."""
import numpy as np

_DIGIT = bytes.maketrans(b"ACGT", b"0123")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def canonical(w):
    """canonical code of a window of upper-case ACGT: the smaller of its 2-bit code (A C G T = 0 1 2 3, first base in the
    highest digits) and its reverse complement's"""
    return min(int(w.translate(_DIGIT), 4), int(w.translate(_COMP)[::-1].translate(_DIGIT), 4))


def seam_arena():
    """(reads, dict) at k = 23: reads cut from a 400-base sequence G whose k-mers are the table, and junk that is not in it"""
    rng = np.random.default_rng(20240611)
    k = 23
    letters = np.frombuffer(b"ACGT", np.uint8)
    G = rng.choice(letters, size=400).tobytes()
    junk = lambda n: rng.choice(letters, size=n).tobytes()   # noqa: E731
    counts = {canonical(G[i:i + k]): 5 for i in range(len(G) - k + 1)}
    reads = []
    pos = lambda: sum(len(r) + 1 for r in reads)   # noqa: E731

    def pad_to(start):
        """filler reads (of G and junk, at most 1 000 bases each) so that the next read starts at arena byte `start`"""
        while pos() < start:
            n = min(1000, start - pos() - 1)
            reads.append((G + junk(300) + G + junk(300))[:n])
        assert pos() == start

    for n in (0, 1, 22, 23, 24, 64, 65, 86, 87, 150):
        reads.append(G[7:7 + n])
    reads.append(G + junk(223) + G)                                  # 1 023 bases: 17 plane words, a weak gap in the middle
    assert len(reads[-1]) == 1023
    reads.append(G[0:23] + junk(40))                                 # the only solid window is the first
    reads.append(junk(40) + G[100:123])                              # ... the last
    reads.append(G[0:40] + junk(30) + G[200:240])                    # a weak gap in the middle
    reads.append(b"N" + G[1:100])                                    # N at the first base
    reads.append(G[0:99] + b"N")                                     # ... at the last
    reads.append(G[0:10] + b"N" + G[11:33] + b"N" + G[34:120])       # two N, k apart
    reads.append(G[0:50] + b"a" + G[51:100])                         # lower case is not ACGT to the kernels
    reads.append(junk(22))
    for tile in (4096, 8192):
        pad_to(tile - 46)
        reads.append(G[10:97])                                       # bytes tile - 46 .. tile + 40: straddles tile - 1 / tile / tile + 1
        pad_to(tile + 1024 - 24)                                      # ... and the boundary between two wavefronts' shares of a tile
        reads.append(G[200:287])
    pad_to(3 * 4096 - 88)
    reads.append(G[100:187])                                         # its NUL is the tile's last byte
    reads.append(G[150:237])                                         # starts at a tile's first byte
    pad_to(4 * 4096 - 1)
    reads.append(G[0:87])                                            # its first base is a tile's last byte
    last = G[300:387]
    if (pos() + len(last) + 1) % 16 == 0:
        last += G[387:388]
    reads.append(last)                                               # ends with the arena, whose size is no multiple of 16
    return k, reads, counts
