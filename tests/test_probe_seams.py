"""GPU: the arena-order kernels that share k_weak_planes' tile (rc_device.h: rc_tile_stage; rc_common.h: rc_tile_window) over the
arena that tests/test_weak_profile.py aims at that tile's seams: k_probe through rc_probe_device, k_count_scan<0> and <1>
through the counter.  tests/seam_arena.py: reads that straddle tile - 1 / tile / tile + 1 and the wavefronts' shares of a tile,
a NUL on a tile's last byte, a read that starts on a tile's first byte, one whose first base is a tile's last byte, an arena
whose size is no multiple of 16, N, lower case, reads shorter than k.  About 17 KB: the smallest arena that has every seam.

Expected values come from the reads and the dictionary in Python, never from the library; every comparison is exact."""
from collections import Counter

import numpy as np
import pytest

import rcorrector_amd
from seam_arena import canonical, seam_arena

pytestmark = pytest.mark.gpu
_ACGT = frozenset(b"ACGT")


def test_probe_device_over_the_seam_arena():
    import torch
    k, reads, counts = seam_arena()
    arena, off = rcorrector_amd.pack_reads(reads)
    assert arena.size % 16 != 0 and arena.size > 4 * 4096
    want = np.full(arena.size, -7, dtype=np.int32)       # a position that starts no k-mer of a read is left alone
    for r, o in zip(reads, off[:-1].tolist()):
        for i in range(len(r) - k + 1):
            w = r[i:i + k]
            want[o + i] = counts.get(canonical(w), 0) if _ACGT.issuperset(w) else 0
    assert (want == 5).any() and (want == 0).any() and (want == -7).sum() > len(reads)
    ctx = rcorrector_amd.Context(k=k, device=0)
    codes = np.array(sorted(counts), dtype=np.uint64)
    ctx.table_build(codes, np.full(len(codes), 5, dtype=np.int32))
    d_seq = torch.from_numpy(arena).cuda()
    d_cnt = torch.full((arena.size,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.probe_device(d_seq, arena.size, d_cnt)
    ctx.sync()
    got = d_cnt.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "arena byte %d: got %d, want %d (%d positions differ)" % (bad[0], got[bad[0]], want[bad[0]], len(bad))
    ctx.close()


@pytest.mark.parametrize("how", ["as_is", "mem_1mb", "mem_1mb_three_times"])
def test_count_reads_device_over_the_seam_arena(how, monkeypatch):
    """as_is / mem_1mb: rc_table_count_reads_device, without and with RC_COUNT_MEM_MB=1 (read when the context is made).  At 17 KB
    the counter plans one slice even then (rc_count.hip: rc_count_plan), so mem_1mb_three_times hands the arena over three times
    (count_begin / count_add / count_finish): three slices, every count three times the Counter's."""
    import torch
    k, reads, _ = seam_arena()
    arena, _ = rcorrector_amd.pack_reads(reads)
    times = 3 if how == "mem_1mb_three_times" else 1
    full = Counter()
    for r in reads:
        for i in range(len(r) - k + 1):
            if _ACGT.issuperset(r[i:i + k]):
                full[canonical(r[i:i + k])] += times
    assert min(full.values()) == times and max(full.values()) > 2 * times
    if how != "as_is":
        monkeypatch.setenv("RC_COUNT_MEM_MB", "1")
    ctx = rcorrector_amd.Context(k=k, device=0)
    d_seq = torch.from_numpy(arena).cuda()
    torch.cuda.synchronize()
    for min_count in (1, 2):
        want = {c: v for c, v in full.items() if v >= min_count}
        if times == 1:
            n = ctx.count_reads_device(d_seq, arena.size, min_count)
        else:
            ctx.count_begin()
            for _ in range(times):
                ctx.count_add(arena)
            n = ctx.count_finish(min_count)
        codes, cnts = ctx.table_export()
        got = dict(zip(codes.tolist(), cnts.tolist()))
        assert n == len(codes) == len(got) == len(want)
        assert got == want, "min_count %d: %d keys differ" % (min_count, len(set(got.items()) ^ set(want.items())))
    ctx.sync()
    ctx.close()
