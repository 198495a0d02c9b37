"""GPU: k_norm_select alone (rc_norm_select_device; rcorrector_amd/csrc/rc_norm.hip).  The depth arrays are synthetic and
uploaded as they are -- no table, no reads -- and d_keep and d_tally are compared exactly with tests/norm_model.py: every unit
count at which the launch changes shape, the three modes, the boundary depths, one hot bin on each of the kernel's three
binning paths, max_bin on both sides of the depths, two calls into one tally, a unit base beyond 2^32, guard bytes around
d_keep and guard words behind d_tally, and every refusal."""
import os
import re

import numpy as np
import pytest

import norm_model as nm
import rcorrector_amd

pytestmark = pytest.mark.gpu
RC_STATUS_ARG = -1
TOP = (1 << 31) - 1
GUARD = 64          # bytes in front of and behind d_keep, words behind d_tally
SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rcorrector_amd", "csrc", "rc_norm.hip")).read()
THREADS, BLOCKS_PER_CU, LDS_BINS = (int(re.search(r"#define %s (\d+)" % name, SRC).group(1))
                                    for name in ("RC_NORM_THREADS", "RC_NORM_BLOCKS_PER_CU", "RC_NORM_LDS_BINS"))


@pytest.fixture(scope="module")
def ctx():
    c = rcorrector_amd.Context(k=23, device=0)      # (no table: the selection needs none)
    yield c
    c.sync()
    c.close()


def device_select(ctx, rows, n_units, mode, unit_base, target, min_cov, seed, max_bin, d_tally=None):
    """(keep, d_tally): d_keep between guard bytes, d_tally (a new zeroed one, or the one given) with guard words behind it; both
    guards checked here"""
    import torch
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 4)
    d_depth = torch.from_numpy(rows).cuda() if len(rows) else torch.zeros((1, 4), dtype=torch.int32, device="cuda")
    buf = torch.full((n_units + 2 * GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    words = 4 + 2 * (max_bin + 1)
    if d_tally is None:
        d_tally = torch.zeros((words + GUARD,), dtype=torch.int64, device="cuda")
        d_tally[words:] = -12345
    torch.cuda.synchronize()
    ctx.norm_select_device(d_depth, n_units, mode, unit_base, target, min_cov, seed, max_bin, buf.data_ptr() + GUARD, d_tally)
    ctx.sync()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == 0xAB).all() and (got[GUARD + n_units:] == 0xAB).all(), "a byte outside d_keep[0 .. n_units) was written"
    assert (d_tally[words:].cpu().numpy() == -12345).all(), "a word behind d_tally was written"
    return got[GUARD:GUARD + n_units], d_tally


def check(ctx, rows, n_units, mode, unit_base, target, min_cov, seed, max_bin, what=""):
    keep, d_tally = device_select(ctx, rows, n_units, mode, unit_base, target, min_cov, seed, max_bin)
    want_keep, want_tally, _ = nm.select_np(rows, n_units, mode, unit_base, target, min_cov, seed, max_bin)
    bad = np.nonzero(keep != want_keep)[0]
    assert len(bad) == 0, "%s: unit %d: got %d, want %d (%d units differ)" % (what, bad[0], keep[bad[0]], want_keep[bad[0]], len(bad))
    tally = d_tally.cpu().numpy()[:len(want_tally)]
    bad = np.nonzero(tally != want_tally)[0]
    assert len(bad) == 0, "%s: tally word %d: got %d, want %d (%d words differ)" % (what, bad[0], tally[bad[0]], want_tally[bad[0]], len(bad))
    return want_keep, want_tally


def random_rows(rng, n, target):
    """depth rows of every kind: a quarter without a valid window (a median left in them all the same), medians around the
    target, far above it, and anywhere below 2^31"""
    kind = rng.integers(0, 4, n)
    med = np.where(kind == 0, rng.integers(0, 2 * target + 2, n), np.where(kind == 1, rng.integers(0, 40 * target, n),
                   np.where(kind == 2, rng.integers(0, 1 << 31, n), rng.integers(0, 70000, n))))
    valid = np.where(rng.integers(0, 4, n) == 0, 0, rng.integers(1, 1002, n))
    return np.stack([valid, med // 2, med, med], axis=1).astype(np.int32)


def full_grid():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * BLOCKS_PER_CU * THREADS


# ---- 1. every unit count at which the launch changes shape, the three modes ----------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_unit_counts_around_a_wavefront_a_workgroup_and_the_grid(ctx, mode):
    rng = np.random.default_rng(100 + mode)
    sizes = [0, 1, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, full_grid() - 1, full_grid() + 1]   # (the kernel strides from full_grid() on)
    for n_units in sizes:
        rows = random_rows(rng, n_units * (1 if mode == 0 else 2), 30)
        keep, tally = check(ctx, rows, n_units, mode, 1000003 * n_units, 30, 12, 20250611 + n_units, 255, "mode %d, %d units" % (mode, n_units))
        assert tally[:4].sum() == n_units
        if n_units >= full_grid() - 1:
            assert set(keep.tolist()) == {nm.OVER, nm.KEPT, nm.LOW, nm.NOVALID}


def test_no_units_is_ok_and_launches_nothing(ctx):
    ctx.profile(True)
    ctx.profile_reset()
    L = rcorrector_amd.load_library()
    assert L.rc_norm_select_device(ctx._h, None, 0, 0, 0, 10, 0, 0, 10, None, None) == 0
    assert ctx.profile_get(9) == (0.0, 0)
    check(ctx, random_rows(np.random.default_rng(1), 10, 30), 10, 0, 0, 30, 0, 1, 10)
    ms, launches = ctx.profile_get(9)                       # the selection's timer, behind the screen's
    ctx.profile(False)
    assert launches == 1 and ms > 0 and ctx.profile_get(8)[1] == 0


# ---- 2. the boundary depths ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target,min_cov", [(50, 5), (7, 9), (1, 0), (1, 1), (TOP, 0), (TOP, TOP), (1000, (1 << 32) - 1)])
def test_boundary_depths_in_every_combination_of_valid_mates(ctx, target, min_cov):
    ds = sorted({d for d in (0, 1, min_cov - 1, min_cov, target, target + 1, 2 * target, 3 * target, TOP - 1, TOP) if 0 <= d <= TOP})
    rows = [(va, 0, a, 0) for a in ds for b in ds for va in (0, 3) for vb in (0, 1) for _ in range(2)]       # mate 1 of every unit, each twice
    rows2 = [(vb, 0, b, 0) for a in ds for b in ds for va in (0, 3) for vb in (0, 1) for _ in range(2)]      # mate 2
    n = len(rows)
    assert (3, 0, TOP, 0) in rows and (1, 0, TOP, 0) in rows2                                                  # m1 + m2 + 1 = 2^32 - 1 occurs
    for base in (0, (1 << 32) + 5):
        check(ctx, np.array(rows + rows2), n, 1, base, target, min_cov, 99, 255, "mode 1")
        check(ctx, np.array([r for pair in zip(rows, rows2) for r in pair]), n, 2, base, target, min_cov, 99, 255, "mode 2")
        keep, _ = check(ctx, np.array(rows + rows2), 2 * n, 0, base, target, min_cov, 99, 255, "mode 0")
    assert nm.NOVALID in keep and (nm.KEPT in keep) == (min_cov <= TOP)


# ---- 3. the hot bin: 100 000 units of one depth, on each binning path ----------------------------------------------------------
@pytest.mark.parametrize("depth,max_bin,path", [(200, 255, "an LDS bin"), (LDS_BINS + 904, 10000, "a tail bin: one atomic per wavefront"),
                                                (70000, 65535, "the folding bin"), (LDS_BINS, LDS_BINS, "the folding bin right behind the LDS bins")])
def test_a_hundred_thousand_units_of_one_depth(ctx, depth, max_bin, path):
    n, target = 100000, depth // 4
    rows = np.tile(np.array([[100, 1, depth, depth + 1]], dtype=np.int32), (n, 1))
    keep, tally = check(ctx, rows, n, 0, 0, target, 0, 5, max_bin, path)
    b = min(depth, max_bin)
    assert tally[4 + b] == n and tally[4 + max_bin + 1 + b] == tally[nm.KEPT] and abs(int(tally[nm.KEPT]) - 25000) <= 685   # (five sigma, as the model's)
    # pairs of that depth, every fourth without a valid mate 2, every fifth without any
    rows2 = np.tile(rows, (2, 1))
    rows2[1::8, 0] = 0
    rows2[0::10, 0] = rows2[1::10, 0] = 0
    check(ctx, rows2, n, 2, 7, target, 0, 5, max_bin, path + ", pairs")


# ---- 4. max_bin on both sides of the depths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_bin", [1, 255, LDS_BINS - 1, LDS_BINS, LDS_BINS + 1, 10000, 65535])
def test_depths_on_both_sides_of_max_bin(ctx, max_bin):
    rng = np.random.default_rng(max_bin)
    edge = [0, 1, 2, max_bin - 1, max_bin, max_bin + 1, 2 * max_bin, LDS_BINS - 1, LDS_BINS, LDS_BINS + 1, 65534, 65535, 65536, TOP]
    med = np.concatenate([np.repeat(np.array(edge, dtype=np.int64), 3), rng.integers(0, 2 * max_bin + 2, 20000), rng.integers(0, 1 << 17, 20000)])
    rows = np.stack([np.full(len(med), 7), med, med, med], axis=1).astype(np.int32)
    _, tally = check(ctx, rows, len(med), 0, 0, max(1, max_bin // 2), 1, 3, max_bin)
    before = tally[4:4 + max_bin + 1]
    assert before[max_bin] > 3 and before[:max_bin].sum() > 0 and before.sum() == len(med)        # folded and unfolded units both


# ---- 5. accumulation over batches, the unit base -------------------------------------------------------------------------------
def test_two_calls_into_one_tally_decide_as_one_call_does(ctx):
    rng = np.random.default_rng(5)
    n, cut, base = 30000, 12345, (1 << 32) + 5
    rows = random_rows(rng, 2 * n, 100)                       # mode 2: the cut falls between two pairs
    args = (100, 3, 424242, 10000)
    whole_keep, whole_tally = check(ctx, rows, n, 2, base, *args)
    k1, d_tally = device_select(ctx, rows[:2 * cut], cut, 2, base, *args)
    k2, d_tally = device_select(ctx, rows[2 * cut:], n - cut, 2, base + cut, *args, d_tally=d_tally)
    assert np.array_equal(np.concatenate([k1, k2]), whole_keep) and np.array_equal(d_tally.cpu().numpy()[:len(whole_tally)], whole_tally)
    # the base is part of the draw: the same batch at base 5 keeps other units, and as many within the binomial's reach
    other, _ = check(ctx, rows, n, 2, 5, *args)
    assert not np.array_equal(other, whole_keep) and np.array_equal(other == nm.LOW, whole_keep == nm.LOW)
    assert np.array_equal(other == nm.NOVALID, whole_keep == nm.NOVALID)
    # and a third call with another seed adds to the same words
    k3, d_tally = device_select(ctx, rows, n, 2, base, 100, 3, 1, 10000, d_tally=d_tally)
    t3 = nm.select_np(rows, n, 2, base, 100, 3, 1, 10000)[1]
    assert np.array_equal(d_tally.cpu().numpy()[:len(whole_tally)], whole_tally + t3)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_every_refusal(ctx):
    import torch
    L = rcorrector_amd.load_library()
    d_depth = torch.zeros((16, 4), dtype=torch.int32, device="cuda")
    d_keep = torch.full((8,), 0xAB, dtype=torch.uint8, device="cuda")
    d_tally = torch.zeros((4 + 2 * 11,), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def sel(c=ctx._h, depth=d_depth.data_ptr(), n=8, mode=2, target=10, max_bin=10, keep=d_keep.data_ptr(), tally=d_tally.data_ptr()):
        return L.rc_norm_select_device(c, depth, n, mode, 0, target, 0, 0, max_bin, keep, tally)

    assert sel(c=None) == RC_STATUS_ARG
    assert sel(mode=-1) == RC_STATUS_ARG and sel(mode=3) == RC_STATUS_ARG and b"mode" in L.rc_last_error(ctx._h)
    assert sel(target=0) == RC_STATUS_ARG and sel(target=1 << 31) == RC_STATUS_ARG and b"target" in L.rc_last_error(ctx._h)
    assert sel(target=(1 << 32) - 1) == RC_STATUS_ARG
    assert sel(max_bin=0) == RC_STATUS_ARG and sel(max_bin=65536) == RC_STATUS_ARG and b"max_bin" in L.rc_last_error(ctx._h)
    assert sel(depth=None) == RC_STATUS_ARG and sel(keep=None) == RC_STATUS_ARG and sel(tally=None) == RC_STATUS_ARG
    assert b"null" in L.rc_last_error(ctx._h)
    assert sel(depth=d_depth.data_ptr() + 4) == RC_STATUS_ARG and sel(tally=d_tally.data_ptr() + 4) == RC_STATUS_ARG     # the vector loads, the 64-bit atomics
    assert sel(n=0, mode=5) == RC_STATUS_ARG and sel(n=0, target=0) == RC_STATUS_ARG              # checked whatever n_units is
    assert sel(n=0, depth=None, keep=None, tally=None) == 0
    ctx.sync()
    assert (d_keep.cpu().numpy() == 0xAB).all() and (d_tally.cpu().numpy() == 0).all()             # a refused call writes nothing
    assert sel() == 0 and sel(target=TOP) == 0
    ctx.sync()
    assert (d_keep.cpu().numpy() == nm.NOVALID).all() and d_tally.cpu().numpy().tolist() == [0, 0, 0, 16] + [0] * 22
