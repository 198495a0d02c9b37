"""GPU: the kernels of rcorrector_amd/csrc/rc_transport.hip on their own -- k_unpack_bases / k_put_nuls / k_put_exceptions,
k_fix_list / k_fix_exceptions and k_fix_list_bytes through rc_selftest_transport_packed / rc_selftest_transport_bytes (test
support: the production launchers, no table, no correction) -- against tests/transport_model.py at the places where they can be
wrong without a whole correction noticing: every alignment of the kept arenas, the seam between the mates, the padded tail, dense
words and lone fixes at the ends of a 16 KB block, the rounded exception loop, the fix_cap edge, the grid-stride wrap.  A fix list
is compared as a set of (position, letter): the atomics leave its order open.  Then the public boundary with a real correction:
fix_cap == n_fix and n_fix - 1, and resident sub-ranges that start at every offset modulo 16."""
import time

import numpy as np
import pytest

import datasets
import rcorrector_amd
import transport_model as tm
from rcorrector_amd.binding import SELFTEST_ARENA_SLACK, SELFTEST_CANARY, SELFTEST_FIX_SLACK
from test_gpu_parity import _fixes, _packed_inputs, _pe_var_third, _resident_inputs, _table

pytestmark = pytest.mark.gpu

SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 16383, 16384, 16385, 65541]
CANARY32 = SELFTEST_CANARY * 0x01010101
BLOCK_WORDS = 1024   # RC_FIX_WORDS: a workgroup's stretch of k_fix_list / k_fix_list_bytes, thread t takes words 256 q + t of it


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    c = gpu_ctx_factory(23, 4)
    yield c
    c.close()


def _check_list(got, want, cap):
    """got = (n_fix, fix_pos, fix_chr) with the slack, want = the model's (positions ascending, letters): the count is the
    model's, what was written is the model's set without a position twice, and everything behind it is still the canary."""
    n_fix, fix_pos, fix_chr = got
    assert len(fix_pos) == len(fix_chr) == cap + SELFTEST_FIX_SLACK
    assert n_fix == len(want[0]), "n_fix = %d, the model lists %d" % (n_fix, len(want[0]))
    k = min(n_fix, cap)
    assert (fix_pos[k:] == CANARY32).all() and (fix_chr[k:] == SELFTEST_CANARY).all(), "an entry was written behind the list"
    pos, chr_ = fix_pos[:k], fix_chr[:k]
    assert len(np.unique(pos)) == k, "a position is listed twice"
    if k == n_fix:
        o = np.argsort(pos)
        assert np.array_equal(pos[o], want[0]) and np.array_equal(chr_[o], want[1])
    else:   # the first cap entries: distinct members of the model's set
        at = np.searchsorted(want[0], pos)
        assert (at < len(want[0])).all() and np.array_equal(want[0][np.minimum(at, len(want[0]) - 1)], pos) and np.array_equal(want[1][at], chr_)


def _check_unpacked(unpacked, words, nbytes, off, exc):
    r = tm.round16(nbytes)
    assert len(unpacked) == r + SELFTEST_ARENA_SLACK
    assert np.array_equal(unpacked[:nbytes], tm.unpack(words, nbytes, off, exc)), "the unpacked arena differs from the model"
    # what k_fix_list relies on: the padding of the last word reads as the letters of its packed codes
    assert np.array_equal(unpacked[nbytes:r], tm.letters(words)[nbytes:r]), "the padding is not the letters of the packed padding"
    assert (unpacked[r:] == SELFTEST_CANARY).all(), "the unpack wrote behind the arena's last word"


def _run_packed(ctx, rng, arena, off, after, cap=None, check_unpacked=True):
    """arena -> packed (the model's pack, the exception list in random order) -> the kernels -> checked; returns the model's list"""
    words, exc_pos, exc_chr = tm.pack(arena)
    o = rng.permutation(len(exc_pos))
    exc_pos, exc_chr = exc_pos[o], exc_chr[o]
    want = tm.fixes_packed(words, exc_pos, after)
    cap = len(want[0]) + 3 if cap is None else cap
    unpacked, n_fix, fix_pos, fix_chr = ctx.selftest_transport_packed(words, arena.size, off, exc_pos, exc_chr, after, cap)
    if check_unpacked:
        _check_unpacked(unpacked, words, arena.size, off, (exc_pos, exc_chr))
    _check_list((n_fix, fix_pos, fix_chr), want, cap)
    return want


# ---- unpack -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.0, 0.01, 1.0])
@pytest.mark.parametrize("nbytes", SIZES)
def test_unpack(ctx, nbytes, density):
    """k_unpack_bases + k_put_nuls + k_put_exceptions: reads of random lengths with a lone NUL among them, no exceptions / about
    1 % (one at position 0, one in the last word, one in front of a NUL) / an all-N arena.  The first nbytes bytes are the
    model's, the padding up to the next multiple of 16 reads as the letters of the packed padding, nothing is written behind it;
    and an arena nobody changed has no fixes.  The model's pack is the library's (Context.pack_bases)."""
    rng = np.random.default_rng(nbytes * 7 + int(density * 100))
    off = tm.read_offsets(rng, nbytes)
    assert (np.diff(off.astype(np.int64)) == 1).any()           # a 1-byte read: a lone NUL
    arena = tm.random_arena(rng, off, density)
    words, exc_pos, exc_chr = tm.pack(arena)
    bases, ep, ec = ctx.pack_bases(arena)
    assert np.array_equal(bases, words) and np.array_equal(ep, exc_pos) and np.array_equal(ec, exc_chr)
    if density == 0.01 and nbytes >= 15:
        # at position 0, directly in front of a NUL, and in the last word (which, at one byte past a multiple of 16, is the final NUL alone)
        assert exc_pos[0] == 0 and (arena[exc_pos.astype(np.int64) + 1] == 0).any()
        assert nbytes % 16 == 1 or exc_pos[-1] >= (nbytes - 1) // 16 * 16
    if density == 1.0:
        assert len(exc_pos) == int((arena != 0).sum())
    want = _run_packed(ctx, rng, arena, off, arena.copy())
    assert len(want[0]) == 0


# ---- the fix list against the packed codes -----------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.0, 0.005, 0.2, 1.0])
@pytest.mark.parametrize("nbytes", SIZES)
def test_fix_list_packed(ctx, nbytes, density):
    """k_fix_list + k_fix_exceptions: no base / 0.5 % / 20 % / every base replaced, on arenas without exceptions, with about 1 %
    and of nothing but exceptions, the exceptions left alone, all replaced by 'A' (only k_fix_exceptions can see those), all by
    C / G / T (only k_fix_list can) and the three in turn.  Bases and exceptions that become a letter outside ACGT, untouched
    exceptions and NULs are no fixes."""
    rng = np.random.default_rng(nbytes * 11 + int(density * 1000))
    seen = 0
    for exc_density in (0.0, 0.01, 1.0):
        off = tm.read_offsets(rng, nbytes)
        arena = tm.random_arena(rng, off, exc_density)
        for exc_mode in (("alone",) if exc_density == 0.0 else ("alone", "A", "CGT", "mixed")):
            after = tm.substitute(rng, arena, density, exc_mode)
            want = _run_packed(ctx, rng, arena, off, after, check_unpacked=False)
            seen += len(want[0])
            changed = np.nonzero(after != arena)[0]
            silent = np.setdiff1d(changed, want[0].astype(np.int64))     # changed into a letter outside ACGT: no fix
            assert np.isin(after[changed], tm.ACGT).sum() == len(want[0]) and not np.isin(after[silent], tm.ACGT).any()
    assert seen > 0 or nbytes <= 2


def _word_pos(ok, w, count=1):
    """`count` positions of word w at which ok holds"""
    c = np.nonzero(ok[16 * w:16 * w + 16])[0]
    assert c.size >= count, "word %d has %d usable positions" % (w, c.size)
    return [16 * w + int(x) for x in c[:count]]


def _placements(n, ok):
    """name -> positions: the single fixes and the dense patterns of the issue, for an arena of n bytes (more than two 16 KB
    blocks) whose usable positions are ok"""
    full = [w for w in range(256, BLOCK_WORDS) if ok[16 * w:16 * w + 16].all()]
    assert ok[0] and ok[n - 2] and full and n > 2 * 16 * BLOCK_WORDS + 16
    return {
        "the first byte": [0],
        "the last byte before the final NUL": [n - 2],
        "the last, partial word": _word_pos(ok, (n - 1) >> 4),
        "thread 255's first word of block 0": _word_pos(ok, 255),
        "thread 255's last word of block 0": _word_pos(ok, BLOCK_WORDS - 1),
        "the first word of block 1": _word_pos(ok, BLOCK_WORDS),
        "thread 255's last word of block 1": _word_pos(ok, 2 * BLOCK_WORDS - 1),
        "the first word of block 2": _word_pos(ok, 2 * BLOCK_WORDS),
        "sixteen fixes in one word": _word_pos(ok, full[0], 16),
        "lanes 63 and 64 only": _word_pos(ok, 63, 3) + _word_pos(ok, 64, 2) + _word_pos(ok, BLOCK_WORDS + 512 + 63, 1) + _word_pos(ok, BLOCK_WORDS + 512 + 64, 4),
        "lane 63 of every wave": sum((_word_pos(ok, 64 * v + 63, 1 + v) for v in range(4)), []),
        "lane 0 of every wave": sum((_word_pos(ok, 256 + 64 * v, 4 - v) for v in range(4)), []),
    }


PLACEMENTS = ["the first byte", "the last byte before the final NUL", "the last, partial word", "thread 255's first word of block 0",
              "thread 255's last word of block 0", "the first word of block 1", "thread 255's last word of block 1", "the first word of block 2",
              "sixteen fixes in one word", "lanes 63 and 64 only", "lane 63 of every wave", "lane 0 of every wave"]


@pytest.mark.parametrize("where", PLACEMENTS)
def test_fix_list_packed_placed_fixes(ctx, where):
    """Exactly the fixes of one placement and no other, in an arena of four 16 KB blocks and a 5-byte last word: lone fixes at
    the ends of the arena and of a workgroup's stretch, a word whose sixteen bytes are all fixes, fixes in lanes 63 and 64 alone
    (the per-wave totals of the workgroup's scan), in the last / the first lane of each of the four waves."""
    rng = np.random.default_rng(5)
    n = 65541
    off = tm.read_offsets(rng, n, lone_nul=False)
    arena = tm.random_arena(rng, off)
    at = np.array(_placements(n, arena != 0)[where], np.int64)
    after = arena.copy()
    after[at] = tm.other_base(rng, arena[at])
    want = _run_packed(ctx, rng, arena, off, after, check_unpacked=False)
    assert np.array_equal(want[0], np.sort(at))


@pytest.mark.parametrize("n_exc", [0, 1, 63, 64, 65, 255, 256, 257])
def test_fix_exceptions_loop_edges(ctx, n_exc):
    """k_fix_exceptions rounds its loop to whole workgroups so that whole wavefronts reach the ballot: exactly n_exc exceptions
    around the wavefront and the workgroup size; all of them, none, the three treatments in turn, only the first and only the
    last of the list replaced by 'A'; with and without fixes of k_fix_list beside them."""
    rng = np.random.default_rng(100 + n_exc)
    off = tm.read_offsets(rng, 4097)
    arena = tm.random_arena(rng, off, n_exc=n_exc)
    assert int(((arena != 0) & ~np.isin(arena, tm.ACGT)).sum()) == n_exc
    for density in (0.0, 0.05):
        for exc_mode in ("A", "alone", "mixed", "CGT"):
            want = _run_packed(ctx, rng, arena, off, tm.substitute(rng, arena, density, exc_mode), check_unpacked=False)
            if density == 0.0:
                assert len(want[0]) == {"A": n_exc, "alone": 0, "mixed": (n_exc + 1) // 3 + n_exc // 3, "CGT": n_exc}[exc_mode]
    if n_exc:
        # (the list's order is the caller's: the first and the last entry of a list in random order)
        words, exc_pos, exc_chr = tm.pack(arena)
        o = rng.permutation(n_exc)
        exc_pos, exc_chr = exc_pos[o], exc_chr[o]
        for j in sorted({0, n_exc - 1}):
            after = arena.copy()
            after[exc_pos[j]] = ord("A")
            got = ctx.selftest_transport_packed(words, arena.size, off, exc_pos, exc_chr, after, 4)
            _check_list(got[1:], (exc_pos[j:j + 1], after[exc_pos[j:j + 1]]), 4)


# ---- the fix list against bytes ------------------------------------------------------------------------------------
def _pad_like(rng, after, lo, count):
    """count bytes that differ from after[lo + j] where the arena has such a byte and from the canary behind the arena elsewhere:
    what lies around a range of a kept arena, chosen so that every byte of it a kernel wrongly compared would be listed"""
    ref = np.full(count, SELFTEST_CANARY, np.uint8)
    idx = lo + np.arange(count)
    ok = (idx >= 0) & (idx < after.size)
    ref[ok] = after[idx[ok]]
    return ref ^ rng.integers(1, 256, size=count).astype(np.uint8)


def _bytes_inputs(rng, na, shift_a, nb, shift_b, density=0.0, at=None, exc_density=0.01):
    """(orig_a buffer, orig_b buffer or None, after, the model's list): a corrected arena of na + nb bytes and the uncorrected
    ranges it differs from at a share `density` of the bytes, or at the positions `at` alone.  Without `at`, every run whose seam
    lies inside a word has a differing byte on each side of it in that word, and every run with a partial last word one in it."""
    n = na + nb
    off = tm.read_offsets(rng, n, lone_nul=n >= 40)
    after = tm.random_arena(rng, off, exc_density)
    if at is None:
        at = np.nonzero(rng.random(n) < density)[0] if density < 1.0 else np.arange(n)
        forced = []
        if na % 16:
            forced.append(int(rng.integers(na & ~15, na)))                          # the straddling word, first mates' side
            if nb:
                forced.append(int(rng.integers(na, min((na & ~15) + 16, n))))       # ... second mates' side
        if n % 16:
            forced.append(int(rng.integers(n & ~15, n)))                            # the partial last word
        at = np.union1d(at, forced).astype(np.int64)
    else:
        at = np.unique(np.asarray(at, np.int64))
    orig = after.copy()
    orig[at] ^= rng.integers(1, 256, size=at.size).astype(np.uint8)
    buf_a = np.concatenate([_pad_like(rng, after, -shift_a, shift_a), orig[:na], _pad_like(rng, after, na, SELFTEST_ARENA_SLACK)])
    buf_b = np.concatenate([_pad_like(rng, after, na - shift_b, shift_b), orig[na:], _pad_like(rng, after, n, SELFTEST_ARENA_SLACK)]) if nb else None
    want = tm.fixes_bytes(orig, after)
    assert np.array_equal(want[0], at)
    # asserted from the inputs: the seam's word and the last word hold differing bytes
    p = want[0].astype(np.int64)
    if na % 16 and density is not None:
        assert ((p >= (na & ~15)) & (p < na)).any() and (not nb or ((p >= na) & (p < (na & ~15) + 16)).any())
    if n % 16 and density is not None:
        assert (p >= (n & ~15)).any()
    return buf_a, buf_b, after, want


def _run_bytes(ctx, rng, na, shift_a, nb, shift_b, density=0.0, at=None, cap=None):
    buf_a, buf_b, after, want = _bytes_inputs(rng, na, shift_a, nb, shift_b, None if at is not None else density, at)
    cap = len(want[0]) + 3 if cap is None else cap
    _check_list(ctx.selftest_transport_bytes(buf_a, na, shift_a, buf_b, nb, shift_b, after, cap), want, cap)
    return want


BYTES_DENSITIES = [0.0, 0.005, 0.2, 1.0]   # (0.0: the bytes around the seam and in the last word alone)


@pytest.mark.parametrize("shift_a", range(16))
def test_fix_list_bytes_every_shift_of_the_first_range(ctx, shift_a):
    """rc_load16_any on orig_a: every shift_a against every na % 16, nb = 0 -- a few hundred bytes, and fewer than 16."""
    rng = np.random.default_rng(200 + shift_a)
    for r in range(16):
        for density in BYTES_DENSITIES:
            _run_bytes(ctx, rng, 16 * int(rng.integers(20, 60)) + r, shift_a, 0, 0, density)
        if r:
            _run_bytes(ctx, rng, r, shift_a, 0, 0, 0.3)


@pytest.mark.parametrize("shift_b", range(16))
def test_fix_list_bytes_every_shift_of_the_second_range(ctx, shift_b):
    """rc_load16_any on orig_b and the word that straddles the mates: every na % 16 against every shift_b, nb > 0; also na = 0 and
    na < 16 in front of a second range."""
    rng = np.random.default_rng(300 + shift_b)
    for r in range(16):
        for density in BYTES_DENSITIES:
            _run_bytes(ctx, rng, 16 * int(rng.integers(20, 60)) + r, int(rng.integers(0, 16)), int(rng.integers(1, 900)), shift_b, density)
        _run_bytes(ctx, rng, r, int(rng.integers(0, 16)), int(rng.integers(1, 900)), shift_b, 0.3)     # (r == 0: na = 0)
        _run_bytes(ctx, rng, r, int(rng.integers(0, 16)), int(rng.integers(1, 16)), shift_b, 0.0)      # both ranges inside one or two words


@pytest.mark.parametrize("seed", range(6))
def test_fix_list_bytes_random_triples(ctx, seed):
    """fifty seeded random (shift_a, na, shift_b, nb) each, up to a few 16 KB blocks"""
    rng = np.random.default_rng(400 + seed)
    for _ in range(50):
        na, nb = (int(rng.integers(0, 3000)) if rng.random() < 0.8 else int(rng.integers(0, 40000)) for _ in range(2))
        if na + nb == 0:
            na = 1
        _run_bytes(ctx, rng, na, int(rng.integers(0, 16)), nb, int(rng.integers(0, 16)), BYTES_DENSITIES[int(rng.integers(0, 4))])


@pytest.mark.parametrize("where", PLACEMENTS)
def test_fix_list_bytes_placed_fixes(ctx, where):
    """the placements of test_fix_list_packed_placed_fixes, the seam of the mates in the middle of block 1 and off any boundary"""
    rng = np.random.default_rng(6)
    n, na = 65541, 27003
    at = _placements(n, np.ones(n, bool))[where]
    want = _run_bytes(ctx, rng, na, 5, n - na, 11, at=at)
    assert len(want[0]) == len(at)


# ---- capacity ---------------------------------------------------------------------------------------------------
def test_capacity_packed(ctx):
    """n_fix counts every fix and the arrays hold the first cap: cap = F + 1, F, F - 1, 1, 0 on a list of both kernels' fixes"""
    rng = np.random.default_rng(8)
    off = tm.read_offsets(rng, 20011)
    arena = tm.random_arena(rng, off, 0.01)
    after = tm.substitute(rng, arena, 0.002, "mixed")
    words, exc_pos, exc_chr = tm.pack(arena)
    want = tm.fixes_packed(words, exc_pos, after)
    F = len(want[0])
    assert F >= 3 and np.isin(want[0], exc_pos).any() and not np.isin(want[0], exc_pos).all()
    for cap in (F + 1, F, F - 1, 1, 0):
        _run_packed(ctx, rng, arena, off, after, cap=cap, check_unpacked=False)


def test_capacity_bytes(ctx):
    rng = np.random.default_rng(9)
    buf_a, buf_b, after, want = _bytes_inputs(rng, 9001, 3, 11006, 14, 0.002)
    F = len(want[0])
    assert F >= 3
    for cap in (F + 1, F, F - 1, 1, 0):
        _check_list(ctx.selftest_transport_bytes(buf_a, 9001, 3, buf_b, 11006, 14, after, cap), want, cap)


# ---- grid wrap --------------------------------------------------------------------------------------------------
_WRAP = {}


def _wrap_arena():
    """An arena past every launch's grid cap, made with vectorised numpy only: n_cu * 32 workgroup stretches of the fix lists and
    three more and 7 bytes (also past the unpack's n_cu * 64 * 4096 bytes), reads of 63 bases, n_cu * 16 * 256 + 300 exceptions
    in as many reads; a corrected arena with 0.1 % of the bases replaced and the exceptions treated in turn."""
    if not _WRAP:
        import torch
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        n = n_cu * 32 * 16384 + 3 * 16384 + 7
        n_exc = n_cu * 16 * 256 + 300
        rng = np.random.default_rng(12)
        off = np.append(np.arange(0, n - 7, 64), n).astype(np.uint32)        # (the last read is 70 bases)
        arena = tm.ACGT[rng.integers(0, 4, size=n, dtype=np.uint8)]
        arena[off[1:].astype(np.int64) - 1] = 0
        reads = rng.permutation(len(off) - 1)[:n_exc].astype(np.int64)
        exc_pos = reads * 64 + rng.integers(0, 63, size=n_exc)
        arena[exc_pos] = tm.OTHER[rng.integers(0, tm.OTHER.size, size=n_exc)]
        after = arena.copy()
        hit = np.unique(rng.integers(0, n, size=n // 1000))
        hit = hit[np.isin(arena[hit], tm.ACGT)]
        after[hit] = tm.other_base(rng, arena[hit])
        after[exc_pos[0::3]] = ord("A")
        cgt = exc_pos[1::3]
        after[cgt] = tm.ACGT[rng.integers(1, 4, size=cgt.size)]
        _WRAP.update(n_cu=n_cu, n=n, n_exc=n_exc, off=off, arena=arena, after=after)
    return _WRAP


def test_grid_wrap_packed(ctx):
    """The unpack, k_fix_list and k_fix_exceptions past their grid caps (n_cu * 64, n_cu * 32 and n_cu * 16 workgroups): every
    workgroup takes a second stretch, some a third.  About 134 MB and a million exceptions at 256 CUs.
    Measured on an MI355X (256 CUs, 134 266 887 bytes, 1 048 876 exceptions, 830 209 fixes): 1.5 s, of which 0.02 s in the
    library -- the rest is numpy making the arena, which test_grid_wrap_bytes then reuses."""
    t0 = time.perf_counter()
    w = _wrap_arena()
    words, exc_pos, exc_chr = tm.pack(w["arena"])
    assert len(exc_pos) == w["n_exc"] and w["arena"].size == w["n"]
    assert len(words) > w["n_cu"] * 64 * 256 and len(words) > w["n_cu"] * 32 * BLOCK_WORDS and w["n_exc"] > w["n_cu"] * 16 * 256
    want = tm.fixes_packed(words, exc_pos, w["after"])
    cap = len(want[0])
    t1 = time.perf_counter()
    unpacked, n_fix, fix_pos, fix_chr = ctx.selftest_transport_packed(words, w["n"], w["off"], exc_pos, exc_chr, w["after"], cap)
    t2 = time.perf_counter()
    assert np.array_equal(unpacked[:w["n"]], w["arena"]) and (unpacked[tm.round16(w["n"]):] == SELFTEST_CANARY).all()
    assert (unpacked[w["n"]:tm.round16(w["n"])] == ord("A")).all()
    _check_list((n_fix, fix_pos, fix_chr), want, cap)
    print("grid wrap, packed: %d bytes, %d exceptions, %d fixes: %.2f s in the library, %.2f s in all" %
          (w["n"], w["n_exc"], cap, t2 - t1, time.perf_counter() - t0))


def test_grid_wrap_bytes(ctx):
    """k_fix_list_bytes past its grid cap of n_cu * 32 workgroups, on the same arena cut into two ranges at an odd place, both
    off any 16-byte boundary.  Measured on an MI355X (256 CUs): 0.08 s, of which 0.01 s in the library."""
    t0 = time.perf_counter()
    w = _wrap_arena()
    rng = np.random.default_rng(13)
    n, na, shift_a, shift_b = w["n"], w["n"] // 2 + 5, 9, 6
    after, orig = w["after"], w["arena"]
    buf_a = np.concatenate([_pad_like(rng, after, -shift_a, shift_a), orig[:na], _pad_like(rng, after, na, SELFTEST_ARENA_SLACK)])
    buf_b = np.concatenate([_pad_like(rng, after, na - shift_b, shift_b), orig[na:], _pad_like(rng, after, n, SELFTEST_ARENA_SLACK)])
    want = tm.fixes_bytes(orig, after)
    cap = len(want[0])
    assert (n + 15) // 16 > w["n_cu"] * 32 * BLOCK_WORDS and cap > 0
    t1 = time.perf_counter()
    got = ctx.selftest_transport_bytes(buf_a, na, shift_a, buf_b, n - na, shift_b, after, cap)
    t2 = time.perf_counter()
    _check_list(got, want, cap)
    print("grid wrap, bytes: %d bytes, %d fixes: %.2f s in the library, %.2f s in all" % (n, cap, t2 - t1, time.perf_counter() - t0))


# ---- through the public boundary, with a real correction ---------------------------------------------------------------
@pytest.mark.parametrize("transport", ["packed", "resident"])
def test_fix_cap_edges_through_the_public_boundary(gpu_ctx_factory, oracle, transport):
    """fix_cap == n_fix is room enough: the wait succeeds and the list applied to the arena is the oracle's.  fix_cap == n_fix - 1
    (and 0) is not: the wait raises and names both numbers, the slot is free -- the batch goes in again without a wait in between
    -- and the resubmission with room gives the full list and ret / l / m / h as before.  The first third of pe_var."""
    sub, want, want_arena = _pe_var_third(oracle, 0)
    if transport == "packed":
        c = _table(gpu_ctx_factory, sub)
        arena, off, bases, exc_pos, exc_chr, qb = _packed_inputs(c, oracle, sub)
        submit, wait, flying = (lambda **kw: c.submit_packed(0, 1, arena.size, off, bases, qb, exc_pos, exc_chr, **kw)), c.wait_packed, "_inflight_packed"
    else:
        c = gpu_ctx_factory(sub["k"], sub["mfk"])
        arena, off, qb, args = _resident_inputs(c, oracle, sub)
        submit, wait, flying = (lambda **kw: c.submit_resident(0, 1, off, qb, **dict(args, **kw))), c.wait_resident, "_inflight_resident"
    arena = np.asarray(arena).copy()
    want_fixes = _fixes(arena, want_arena)

    def whole(res):
        for w, g, what in zip(want[:4], res[:4], ["ret", "l", "m", "h"]):
            assert np.array_equal(w, g), "%s differs through the %s boundary" % (what, transport)
        assert sorted(zip(res[4].tolist(), res[5].tolist())) == want_fixes
        host = arena.copy()
        c.apply_fixes(host, res[4], res[5])
        assert np.array_equal(host, want_arena)

    submit()
    roomy = wait(0)
    F = len(roomy[4])
    assert F == len(want_fixes) and F >= 3
    whole(roomy)
    submit(fix_cap=F)
    whole(wait(0))
    for cap in (F - 1, 0):
        submit(fix_cap=cap)
        with pytest.raises(rcorrector_amd.RcorrectorError, match=r"%d substitutions, room for %d \(fix_cap\)" % (F, cap)):
            wait(0)
        assert getattr(c, flying)[0][0].n_fix == F     # (the descriptor says how much room the batch needs)
        submit()
        whole(wait(0))
    c.close()


def test_resident_sub_ranges_start_at_every_alignment(gpu_ctx_factory, oracle):
    """varlen's reads i.. as a resident batch, for sixteen i whose offset in the kept arena takes every value modulo 16
    (begin_a = off[i]: orig_a at every shift): ret / l / m / h are the oracle's rows i.., the fix list is the oracle's
    substitutions in those reads.  One oracle run, indexed (tests/test_transport_model.py holds the indexing to the oracle)."""
    d = datasets.make("varlen")
    want = datasets.run_oracle(oracle, d)
    c = gpu_ctx_factory(d["k"], d["mfk"])
    arena, off, _qb, _args = _resident_inputs(c, oracle, d)
    q1, _ = oracle.pack_reads(d["quals1"])
    n = len(off) - 1
    starts = tm.start_at_every_shift(off, n // 2)
    assert sorted(starts) == list(range(16)) and sorted(int(off[i]) % 16 for i in starts.values()) == list(range(16))
    for s, i in sorted(starts.items()):
        begin = int(off[i])
        sub_off = (off[i:].astype(np.int64) - begin).astype(np.uint32)
        c.submit_resident(s % 2, 0, sub_off, c.pack_quality_bits(q1[begin:], b"H"), arena_a=0, begin_a=begin, bytes_a=arena.size - begin)
        ret, l, m, h, fix_pos, fix_chr = c.wait_resident(s % 2)
        for w, g, what in zip(want[:4], (ret, l, m, h), ["ret", "l", "m", "h"]):
            assert np.array_equal(w[i:], g), "%s differs on reads %d.. (shift %d)" % (what, i, s)
        assert sorted(zip(fix_pos.tolist(), fix_chr.tolist())) == _fixes(arena[begin:], want[4][begin:]), "the fix list differs at shift %d" % s
    c.close()


def test_resident_paired_sub_ranges_at_every_alignment_of_the_second_mates(gpu_ctx_factory, oracle):
    """pe_var's pairs [i, j) as a resident batch, for sixteen (i, j): begin_b = off2[i] takes every value modulo 16 (orig_b at
    every shift of its own) and bytes_a = off1[j] - off1[i] every value modulo 16 (the seam of the mates anywhere in its word, by
    leaving out reads at the end)."""
    d = datasets.make("pe_var")
    want = datasets.run_oracle(oracle, d)
    c = gpu_ctx_factory(d["k"], d["mfk"])
    _resident_inputs(c, oracle, d)
    (a1, off1), (a2, off2) = oracle.pack_reads(d["seqs1"]), oracle.pack_reads(d["seqs2"])
    (q1, _), (q2, _) = oracle.pack_reads(d["quals1"]), oracle.pack_reads(d["quals2"])
    o1, o2 = off1.astype(np.int64), off2.astype(np.int64)
    n = len(off1) - 1
    cuts = tm.paired_cuts(off1, off2, n // 2)
    assert sorted(cuts) == list(range(16))
    assert sorted(int(o2[i]) % 16 for i, j in cuts.values()) == sorted(int(o1[j] - o1[i]) % 16 for i, j in cuts.values()) == list(range(16))
    for s, (i, j) in sorted(cuts.items()):
        bytes_a, bytes_b = int(o1[j] - o1[i]), int(o2[j] - o2[i])
        sub_off = np.concatenate([o1[i:j + 1] - o1[i], o2[i + 1:j + 1] - o2[i] + bytes_a]).astype(np.uint32)
        qb = c.pack_quality_bits(np.concatenate([q1[o1[i]:o1[j]], q2[o2[i]:o2[j]]]), b"H")
        c.submit_resident(s % 2, 1, sub_off, qb, arena_a=0, begin_a=int(o1[i]), bytes_a=bytes_a, arena_b=1, begin_b=int(o2[i]), bytes_b=bytes_b)
        ret, l, m, h, fix_pos, fix_chr = c.wait_resident(s % 2)
        idx = np.concatenate([np.arange(i, j), n + np.arange(i, j)])
        for w, g, what in zip(want[:4], (ret, l, m, h), ["ret", "l", "m", "h"]):
            assert np.array_equal(w[idx], g), "%s differs on pairs [%d, %d) (shift %d)" % (what, i, j, s)
        before = np.concatenate([a1[o1[i]:o1[j]], a2[o2[i]:o2[j]]])
        after = np.concatenate([want[4][o1[i]:o1[j]], want[5][o2[i]:o2[j]]])
        assert sorted(zip(fix_pos.tolist(), fix_chr.tolist())) == _fixes(before, after), "the fix list differs at shift %d" % s
    c.close()
