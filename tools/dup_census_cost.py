#!/usr/bin/env python3
"""What -dups / an open duplicate census costs, measured: the two key passes (k_read_keys over one arena of bench.py's headline
shard -- config 2: 25 M x 150 bp paired reads, k = 23 -- as uploaded and as corrected) per batch, and the final sort and census
(rc_dup_census_get) over the keys of that batch.  Wall time around the call and the context's sync, median of --reps.  With
--parent DIR (a built checkout of the parent commit) it then runs `bench.py --gpus 1 --steps K --warmup 1` -- the benchmark's
step, no census open -- in this tree and in DIR, alternating, --bench-rounds times each, every run a process of its own on the
same GPU, and prints every ms_per_step and the ratio of the medians.  Prints the lines of profiles/dup_census_cost.txt.

    python tools/dup_census_cost.py [--reads N] [--reps R] [--parent DIR] [--bench-rounds B] [--bench-steps K]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import bench  # noqa: E402
import rcorrector_amd  # noqa: E402
import synth_int  # noqa: E402


def timed(fn, sync, reps):
    ms = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms)


def bench_step(tree, steps):
    """ms_per_step of one `bench.py` run in `tree` (its last stdout line is the JSON result)"""
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1"], cwd=tree, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600, check=True)
    return float(json.loads(p.stdout.decode().strip().splitlines()[-1])["ms_per_step"])


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
    keys = torch.zeros((n // 2, 2), dtype=torch.int64, device=dev)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def correct():
        work.copy_(seq)
        torch.cuda.synchronize()
        ctx.correct_device(1, n, nbytes, L, work, qual, off, *res)
        ctx.sync()

    correct()                                                   # warm-up: code objects, scratch
    ctx.read_keys_device(seq, off, n, nbytes, 1, keys)
    ctx.sync()
    before = timed(lambda: ctx.read_keys_device(seq, off, n, nbytes, 1, keys), ctx.sync, a.reps)
    after = timed(lambda: ctx.read_keys_device(work, off, n, nbytes, 1, keys), ctx.sync, a.reps)
    closed = timed(correct, ctx.sync, a.reps)
    ctx.dup_census_begin()
    opened = timed(correct, ctx.sync, 1)                        # (one batch with the census open: its keys are the census's)
    ctx.dup_census(10000)
    census = timed(lambda: ctx.dup_census(10000), ctx.sync, a.reps)
    c = ctx.dup_census(10000)
    ctx.dup_census_end()
    print("shard: %d reads x %d bases (paired: %d units), k = %d, %d k-mers in the table, %d arena bytes" % (n, L, n // 2, k, n_kmers, nbytes))
    print("k_read_keys over the arena as uploaded:  %.2f ms per batch (median of %d; best %.2f) = %.0f GB/s of arena" % (before[0], a.reps, before[1], nbytes / before[0] / 1e6))
    print("k_read_keys over the arena as corrected: %.2f ms per batch (median of %d; best %.2f) = %.0f GB/s of arena" % (after[0], a.reps, after[1], nbytes / after[0] / 1e6))
    print("rc_dup_census_get over the %d units' keys (split, two radix passes, run lengths; both versions): %.2f ms (median of %d; best %.2f)"
          % (c["units"], census[0], a.reps, census[1]))
    print("rc_correct_device of the batch (copy of the arena included), no census open: %.2f ms (median of %d); one batch with the census open: %.2f ms"
          % (closed[0], a.reps, opened[0]))
    print("of those units: %d distinct before correction, %d after; most copies of one unit: before %d, after %d"
          % (c["distinct_before"], c["distinct_after"], int(np.nonzero(c["copies_before"])[0].max()), int(np.nonzero(c["copies_after"])[0].max())))
    sys.stdout.flush()
    if a.parent:
        ctx.close()
        del seq, qual, work, keys, res, off, gen
        torch.cuda.empty_cache()
        here, there = [], []
        for _ in range(a.bench_rounds):
            here.append(bench_step(ROOT, a.bench_steps))
            there.append(bench_step(os.path.abspath(a.parent), a.bench_steps))
        mh, mt = statistics.median(here), statistics.median(there)
        print("bench.py --gpus 1 --steps %d --warmup 1 (config 2, no census open), ms_per_step, runs alternating on one GPU:" % a.bench_steps)
        print("  this commit: %s  median %.2f" % (" ".join("%.2f" % x for x in here), mh))
        print("  its parent:  %s  median %.2f" % (" ".join("%.2f" % x for x in there), mt))
        print("  this commit / parent = %.4f (%+.2f %%)" % (mh / mt, (mh / mt - 1.0) * 100.0))


if __name__ == "__main__":
    main()
