#!/usr/bin/env python3
"""What -trust-by-pos / an open trust profile costs, measured on one arena of bench.py's headline shard (config 2: 25 M x 150 bp
paired reads, k = 23): rc_trust_profile_device per batch -- events around the device entry point for the whole call, and the
library's own timers (rc_profile_get's kernels 5 and 6) for its two parts, the planes pass (k_weak_planes) and the accumulate
(k_trust_accumulate + k_trust_reduce) -- beside the batch's correction, with no profile open and with one open.  Median of
--reps.  With --parent DIR (a built checkout of the parent commit) it then runs `bench.py --gpus 1 --steps K --warmup 1` -- the
benchmark's step, no profile open -- in this tree and in DIR, alternating, --bench-rounds times each, every run a process of its
own on the same GPU, and prints every ms_per_step and the ratio of the medians.  Prints the lines of
profiles/trust_profile_cost.txt.

    python tools/trust_profile_cost.py [--reads N] [--reps R] [--parent DIR] [--bench-rounds B] [--bench-steps K]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import bench  # noqa: E402
import rcorrector_amd  # noqa: E402
import synth_int  # noqa: E402
from dup_census_cost import bench_step, timed  # noqa: E402

T_PLANES, T_ACCUMULATE = 5, 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: also compare bench.py's step there and here")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=3)
    a = ap.parse_args()
    P = dict(bench.PRESETS[2])
    n = a.reads or P["reads"]
    L, k = P["len"], P["k"]
    dev = torch.device("cuda", 0)
    gen = synth_int.Synth(P["seed"], L, 30000, 1500, P["alpha"], P["err"], P["paired"], bias3=P["bias3"], device=dev)
    ctx = rcorrector_amd.Context(k=k, max_fix_per_k=P["maxcork"], device=0)
    seq, qual = gen.generate(0, n // 2)
    torch.cuda.synchronize()
    ctx.count_begin()
    ctx.count_add_device(seq, seq.numel())
    n_kmers = ctx.count_finish(2)
    fh = torch.bincount(qual[0::(L + 1)][:1000000].long(), minlength=300)[:300].cpu().numpy().astype(np.int32)
    lh = torch.bincount(qual[L - 1::(L + 1)][:1000000].long(), minlength=300)[:300].cpu().numpy().astype(np.int32)
    ctx.set_run_params(ctx.estimate_error_rate(0.95), ctx.bad_quality_from_hist(fh, lh, min(n, 1000000)))
    nbytes = n * (L + 1)
    off = (torch.arange(n + 1, device=dev, dtype=torch.int64) * (L + 1)).to(torch.int32)
    res = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4)]
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.zeros((2, 5, 2, 1024), dtype=torch.int64, device=dev)

    def correct():
        work.copy_(seq)
        torch.cuda.synchronize()
        ctx.correct_device(1, n, nbytes, L, work, qual, off, *res)
        ctx.sync()

    def profile(arena, version):
        ctx.trust_profile_device(arena, off, n, nbytes, L, 1, counts[version], 1)

    def events(arena, version):
        """ms between two events on the library's stream's side of the call: recorded on torch's stream around a synchronous wait"""
        ms = []
        for _ in range(a.reps):
            ctx.sync()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            profile(arena, version)
            ctx.sync()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms)

    correct()                                                   # warm-up: code objects, scratch
    profile(seq, 0)
    ctx.sync()
    whole_before, whole_after = events(seq, 0), events(work, 1)
    ctx.profile(1)                                              # the split: the library's events around each part
    ctx.profile_reset()
    for _ in range(a.reps):
        profile(seq, 0)
        profile(work, 1)
    ctx.sync()
    (ms_planes, n_planes), (ms_acc, n_acc) = ctx.profile_get(T_PLANES), ctx.profile_get(T_ACCUMULATE)
    ctx.profile(0)
    counts.zero_()
    profile(seq, 0)
    profile(work, 1)
    ctx.sync()
    c = counts.cpu().numpy()                                    # [version][windows, solid5, weak5, solid3, weak3][mate][p]
    closed = timed(correct, ctx.sync, a.reps)
    ctx.trust_profile_begin(1)
    opened = timed(correct, ctx.sync, a.reps)
    got = ctx.trust_profile()
    ctx.trust_profile_end()
    assert int(got["reads"].sum()) == a.reps * n and np.array_equal(got["after"]["weak5"].astype(np.int64), a.reps * c[1, 2])
    print("shard: %d reads x %d bases (paired), k = %d, %d k-mers in the table, %d arena bytes" % (n, L, k, n_kmers, nbytes))
    print("rc_trust_profile_device over the arena as uploaded:  %.2f ms per batch (events around the call, median of %d; best %.2f)" % (whole_before[0], a.reps, whole_before[1]))
    print("rc_trust_profile_device over the arena as corrected: %.2f ms per batch (events around the call, median of %d; best %.2f)" % (whole_after[0], a.reps, whole_after[1]))
    print("  of which the planes pass (k_weak_planes, profile kernel 5):                         %.2f ms per call (%d calls)" % (ms_planes / n_planes, n_planes))
    print("  of which the accumulate (k_trust_accumulate + k_trust_reduce, profile kernel 6):    %.3f ms per call (%d calls)" % (ms_acc / n_acc, n_acc))
    print("rc_correct_device of the batch (copy of the arena included), no profile open: %.2f ms (median of %d); with a profile open: %.2f ms"
          % (closed[0], a.reps, opened[0]))
    for v, tag in enumerate(("before", "after")):
        weak, solid = int(c[v, 2].sum()), int(c[v, 1].sum())
        last = (c[v, 4, :, 0].sum() / max(1, c[v, 0, :, 0].sum()), c[v, 2, :, 0].sum() / max(1, c[v, 0, :, 0].sum()))
        print("%s correction: %d of %d valid windows weak (%.4f); weak share of the reads' last window %.4f, of their first %.4f" % (tag, weak, weak + solid, weak / max(1, weak + solid), last[0], last[1]))
    sys.stdout.flush()
    if a.parent:
        ctx.close()
        del seq, qual, work, counts, res, off, gen
        torch.cuda.empty_cache()
        here, there = [], []
        for _ in range(a.bench_rounds):
            here.append(bench_step(ROOT, a.bench_steps))
            there.append(bench_step(os.path.abspath(a.parent), a.bench_steps))
        mh, mt = statistics.median(here), statistics.median(there)
        print("bench.py --gpus 1 --steps %d --warmup 1 (config 2, no profile open), ms_per_step, runs alternating on one GPU:" % a.bench_steps)
        print("  this commit: %s  median %.2f" % (" ".join("%.2f" % x for x in here), mh))
        print("  its parent:  %s  median %.2f" % (" ".join("%.2f" % x for x in there), mt))
        print("  this commit / parent = %.4f (%+.2f %%)" % (mh / mt, (mh / mt - 1.0) * 100.0))


if __name__ == "__main__":
    main()
