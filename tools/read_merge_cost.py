#!/usr/bin/env python3
"""What rc_read_merge_device (tools/read_merge) costs per batch, measured on one arena of bench.py's headline shard (config 2:
25 M x 150 bp paired reads, two halves: mode 1) -- its 300-base fragments do not overlap, every offset is scanned and refused, the
merged arena is one NUL per pair -- and on a shard of the same shape whose pairs overlap (--frag, 220-base fragments: every pair
merges), as tools/mate_overlap_cost.py and tools/read_trim_cost.py do.  In one visit, alternating:
  * rc_read_merge_device, the whole call: k_merge_plan, the exclusive scan of the lengths, k_merge_write;
  * rc_read_trim_device with only the pair cut on, on the same arena: the same stage and the same offset scan as k_merge_plan;
  * a device-to-device copy of the bytes k_merge_write reads and writes (both input arenas, the rows, the offsets; the merged
    sequence and quality arenas).
The call is timed as a whole: the three steps run back to back on one stream, so the call minus the pair cut bounds the scan and
the write together from above.  Events around each call on a drained context, a warm-up of each, then the median of --reps runs.
With --parent DIR (a built checkout of the parent commit) it then runs `bench.py --gpus 1 --steps K --warmup 1` -- the benchmark's
step, which runs none of this -- in this tree and in DIR, alternating, --bench-rounds times each, every run a process of its own
on the same GPU.  Prints the lines of profiles/read_merge_cost.txt.

    python tools/read_merge_cost.py [--reads N] [--frag F] [--reps R] [--parent DIR] [--bench-rounds B] [--bench-steps K]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import bench  # noqa: E402
import rcorrector_amd  # noqa: E402
import synth_int  # noqa: E402
from dup_census_cost import bench_step  # noqa: E402
from rcorrector_amd.binding import MERGE_TALLY_WORDS, TRIM_TALLY_WORDS, merge_params, merge_tally_dict, trim_params, trim_tally_dict  # noqa: E402


def shard(P, n, frag, reps, dev):
    L = P["len"]
    gen = synth_int.Synth(P["seed"], L, 30000, 1500, P["alpha"], P["err"], P["paired"], frag_len=frag, bias3=P["bias3"], device=dev)
    ctx = rcorrector_amd.Context(k=P["k"], max_fix_per_k=P["maxcork"], device=0)      # (no table: neither kernel needs one)
    seq, qual = gen.generate(0, n // 2)
    torch.cuda.synchronize()
    nbytes, units = n * (L + 1), n // 2
    off = (torch.arange(n + 1, device=dev, dtype=torch.int64) * (L + 1)).to(torch.int32)
    m_tally = torch.zeros(MERGE_TALLY_WORDS, dtype=torch.int64, device=dev)
    t_tally = torch.zeros(TRIM_TALLY_WORDS, dtype=torch.int64, device=dev)
    m_rows = torch.zeros((units, 4), dtype=torch.int32, device=dev)
    t_rows = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    mseq, mqual = torch.zeros(nbytes, dtype=torch.uint8, device=dev), torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    moff = torch.zeros(units + 1, dtype=torch.int32, device=dev)
    pair_only = trim_params(qual_min=0, adapter1=b"", min_len=0)
    mp = merge_params()

    def event_ms(fn):
        ctx.sync()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        ctx.sync()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    merge = lambda: ctx.read_merge_device(seq, qual, off, n, nbytes, L, 1, mp, m_rows, mseq, mqual, moff, nbytes, m_tally)   # noqa: E731
    trim = lambda: ctx.read_trim_device(seq, None, off, n, nbytes, L, 1, pair_only, t_rows, None, t_tally)                    # noqa: E731
    event_ms(merge)                                             # warm-up: code objects
    event_ms(trim)
    m_tally.zero_()
    t_tally.zero_()
    event_ms(merge)
    event_ms(trim)
    tm, tt = merge_tally_dict(m_tally.cpu().numpy()), trim_tally_dict(t_tally.cpu().numpy())
    assert tm["merged"] == tt["pairs_overlapping"] and tm["pairs"] == tt["units"]      # the same d* accepted in both
    out_bytes = int(moff[units].item()) & 0xFFFFFFFF
    moved = 2 * nbytes + 16 * units + 4 * (units + 1) + 2 * out_bytes
    src, dst = torch.zeros(moved, dtype=torch.uint8, device=dev), torch.zeros(moved, dtype=torch.uint8, device=dev)
    copy = lambda: dst.copy_(src)   # noqa: E731
    event_ms(copy)
    calls = [merge, trim, copy]
    ms = [[], [], []]
    for _ in range(reps):                                       # alternating, so that none has the warmer caches
        for x, c in enumerate(calls):
            ms[x].append(event_ms(c))
    m = [statistics.median(x) for x in ms]
    rng = lambda x: "%.2f..%.2f" % (min(x), max(x))   # noqa: E731
    print("shard: %d reads x %d bases (paired, two halves, %d-base fragments), %d arena bytes; medians of %d runs, events around the call" % (n, L, frag, nbytes, reps))
    print("  rc_read_merge_device, the whole call (plan, scan, write):    %.2f ms per batch (%s)" % (m[0], rng(ms[0])))
    print("  k_read_trim, the pair cut alone, on the same arena:          %.2f ms per batch (%s): the plan's scan" % (m[1], rng(ms[1])))
    print("  the call minus the pair cut (scan of the lengths + write):   %.2f ms" % (m[0] - m[1]))
    print("  device-to-device copy of the %d bytes the write reads and writes: %.2f ms (%s); (call - pair cut) / copy = %.1f" % (moved, m[2], rng(ms[2]), (m[0] - m[1]) / m[2]))
    print("  %d of %d pairs merged, %d read through, %d merged arena bytes, %d of %d faced bases differ: %d to mate 1, %d to mate 2, %d ties" %
          (tm["merged"], tm["pairs"], tm["readthrough"], out_bytes, tm["mismatches"], tm["compared"], tm["took_mate1"], tm["took_mate2"], tm["ties"]))
    sys.stdout.flush()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=None)
    ap.add_argument("--frag", type=int, default=220)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: also compare bench.py's step there and here")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=3)
    a = ap.parse_args()
    P = dict(bench.PRESETS[2])
    n = a.reads or P["reads"]
    dev = torch.device("cuda", 0)
    shard(P, n, 300, a.reps, dev)       # the benchmark's own pairs: they do not overlap, every offset is scanned and refused
    torch.cuda.empty_cache()
    shard(P, n, a.frag, a.reps, dev)    # pairs that overlap
    torch.cuda.empty_cache()
    if a.parent:
        here, there = [], []
        for _ in range(a.bench_rounds):
            here.append(bench_step(ROOT, a.bench_steps))
            there.append(bench_step(os.path.abspath(a.parent), a.bench_steps))
        mh, mt = statistics.median(here), statistics.median(there)
        print("bench.py --gpus 1 --steps %d --warmup 1 (config 2; the step runs none of the new code), ms_per_step, runs alternating on one GPU:" % a.bench_steps)
        print("  this commit: %s  median %.2f  range %.2f..%.2f" % (" ".join("%.2f" % x for x in here), mh, min(here), max(here)))
        print("  its parent:  %s  median %.2f  range %.2f..%.2f" % (" ".join("%.2f" % x for x in there), mt, min(there), max(there)))
        print("  this commit / parent = %.4f (%+.2f %%)" % (mh / mt, (mh / mt - 1.0) * 100.0))


if __name__ == "__main__":
    main()
