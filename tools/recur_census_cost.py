#!/usr/bin/env python3
"""What -recurrent / an open recurrence census costs, measured: the key launch (k_change_keys over one arena of bench.py's
headline shard -- config 2: 25 M x 150 bp paired reads, k = 23 -- as uploaded against as corrected) per batch, beside the
batch's own correction in the same visit, the keys it leaves and the bytes they take, and the final sort and census
(rc_recur_census_get) over the keys of that batch.  Wall time around the call and the context's sync, median of --reps.  With
--parent DIR (a built checkout of the parent commit) it then runs `bench.py --gpus 1 --steps K --warmup 1` -- the benchmark's
step, no census open -- in this tree and in DIR, alternating, --bench-rounds times each, every run a process of its own on the
same GPU, and prints every ms_per_step, both medians and ranges.  Prints the lines of profiles/recur_census_cost.txt.

    python tools/recur_census_cost.py [--reads N] [--reps R] [--parent DIR] [--bench-rounds B] [--bench-steps K]"""
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
    cap = nbytes // 32
    keys = torch.zeros(cap, dtype=torch.int64, device=dev)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)

    def correct():
        work.copy_(seq)
        torch.cuda.synchronize()
        ctx.correct_device(1, n, nbytes, L, work, qual, off, *res)
        ctx.sync()

    correct()                                                   # warm-up: code objects, scratch; `work` holds the corrected arena
    launch = lambda: ctx.change_keys_device(seq, work, off, n, nbytes, keys, cap, counts)   # noqa: E731
    launch()
    ctx.sync()
    changes, contexted, found = [int(x) for x in counts.cpu().numpy()]
    key_ms = timed(launch, ctx.sync, a.reps)
    count_ms = timed(lambda: ctx.change_keys_device(seq, work, off, n, nbytes, keys, 0, counts), ctx.sync, a.reps)
    closed = timed(correct, ctx.sync, a.reps)
    ctx.recur_census_begin()
    opened = timed(correct, ctx.sync, 1)                        # (one batch with the census open: its keys are the census's)
    ctx.recur_census(10000, 5, 1000)
    census = timed(lambda: ctx.recur_census(10000, 5, 1000), ctx.sync, a.reps)
    c = ctx.recur_census(10000, 5, 1000)
    ctx.recur_census_end()
    print("shard: %d reads x %d bases, k = %d, %d k-mers in the table, %d arena bytes" % (n, L, k, n_kmers, nbytes))
    print("k_change_keys, the arena as uploaded against the arena as corrected: %.2f ms per batch (median of %d; best %.2f) = %.0f GB/s of the two arenas"
          % (key_ms[0], a.reps, key_ms[1], 2 * nbytes / key_ms[0] / 1e6))
    print("the same launch with cap = 0 (counting only, nothing written): %.2f ms (best %.2f)" % (count_ms[0], count_ms[1]))
    print("changes %d (%.4f of the bases), contexted %d, keys %d = %d bytes kept per batch; the first launch's buffer holds %d keys"
          % (changes, changes / float(n * L), contexted, found, 8 * found, cap))
    print("rc_recur_census_get over the batch's %d keys (radix sort, run lengths, histogram, top list): %.2f ms (median of %d; best %.2f)"
          % (c["contexted"], census[0], a.reps, census[1]))
    print("rc_correct_device of the batch (copy of the arena included), no census open: %.2f ms (median of %d); one batch with the census open: %.2f ms"
          % (closed[0], a.reps, opened[0]))
    print("of those keys: %d sites, %d of them corrected twice or more (%d changes); most changes at one site: %d; sites corrected 5 times or more: %d"
          % (c["sites"], c["sites_recurrent"], c["changes_at_recurrent"], int(np.nonzero(c["recur"])[0].max()) if c["sites"] else 0, c["n_top"]))
    sys.stdout.flush()
    if a.parent:
        ctx.close()
        del seq, qual, work, keys, res, off, gen
        torch.cuda.empty_cache()
        here, there = [], []
        for _ in range(a.bench_rounds):
            here.append(bench_step(ROOT, a.bench_steps))
            there.append(bench_step(os.path.abspath(a.parent), a.bench_steps))
            print("  (round done: %.2f here, %.2f in the parent)" % (here[-1], there[-1]), file=sys.stderr, flush=True)
        mh, mt = statistics.median(here), statistics.median(there)
        print("bench.py --gpus 1 --steps %d --warmup 1 (config 2, no census open), ms_per_step, runs alternating on one GPU:" % a.bench_steps)
        print("  this commit: %s  median %.2f  range %.2f .. %.2f" % (" ".join("%.2f" % x for x in here), mh, min(here), max(here)))
        print("  its parent:  %s  median %.2f  range %.2f .. %.2f" % (" ".join("%.2f" % x for x in there), mt, min(there), max(there)))
        print("  this commit / parent = %.4f (%+.2f %%); the ranges %s" % (mh / mt, (mh / mt - 1.0) * 100.0,
                                                                          "overlap" if min(here) <= max(there) and min(there) <= max(here) else "do not overlap"))


if __name__ == "__main__":
    main()
