#!/usr/bin/env python3
"""What -overlap / an open mate-overlap session costs, measured on one arena of bench.py's headline shard (config 2: 25 M x 150 bp
paired reads, k = 23) and on a shard of the same shape whose pairs overlap (--frag, 220-base fragments: the benchmark's own
300-base fragments of 150-base reads do not): rc_mate_overlap_device per batch (events around the call), the copy of the arena a
session takes in front of the correction, and the batch's correction with no session open and with one open.  Median of --reps.
With --parent DIR (a built checkout of the parent commit) it then runs `bench.py --gpus 1 --steps K --warmup 1` -- the benchmark's
step, no session open -- in this tree and in DIR, alternating, --bench-rounds times each, every run a process of its own on the
same GPU, and prints every ms_per_step and the ratio of the medians.  Prints the lines of profiles/mate_overlap_cost.txt.

    python tools/mate_overlap_cost.py [--reads N] [--frag F] [--reps R] [--parent DIR] [--bench-rounds B] [--bench-steps K]"""
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
from rcorrector_amd.binding import OVERLAP_WORDS, mate_overlap_dict  # noqa: E402


def shard(P, n, frag, reps, dev):
    L, k = P["len"], P["k"]
    gen = synth_int.Synth(P["seed"], L, 30000, 1500, P["alpha"], P["err"], P["paired"], frag_len=frag, bias3=P["bias3"], device=dev)
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
    work, snap = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.zeros(OVERLAP_WORDS, dtype=torch.int64, device=dev)

    def correct():
        work.copy_(seq)
        torch.cuda.synchronize()
        ctx.correct_device(1, n, nbytes, L, work, qual, off, *res)
        ctx.sync()

    def events(fn):
        ms = []
        for _ in range(reps):
            ctx.sync()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            ctx.sync()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms)

    correct()                                                   # warm-up: code objects, scratch
    ctx.mate_overlap_device(seq, work, off, n, nbytes, L, 1, counts)
    ctx.sync()
    kernel = events(lambda: ctx.mate_overlap_device(seq, work, off, n, nbytes, L, 1, counts))
    copy = events(lambda: snap.copy_(seq))
    counts.zero_()
    ctx.mate_overlap_device(seq, work, off, n, nbytes, L, 1, counts)
    ctx.sync()
    c = mate_overlap_dict(counts.cpu().numpy())
    closed = timed(correct, ctx.sync, reps)
    ctx.mate_overlap_begin()
    opened = timed(correct, ctx.sync, reps)
    got = ctx.mate_overlap()
    ctx.mate_overlap_end()
    assert got["pairs"] == reps * (n // 2) and got["disagree_after"] == reps * c["disagree_after"] and got["introduced"] == reps * c["introduced"]
    print("shard: %d reads x %d bases (paired, %d-base fragments), k = %d, %d k-mers in the table, %d arena bytes" % (n, L, frag, k, n_kmers, nbytes))
    print("  rc_mate_overlap_device, the arena as uploaded against the arena as corrected: %.2f ms per batch (events around the call, median of %d; best %.2f)"
          % (kernel[0], reps, kernel[1]))
    print("  the copy of the arena in front of the correction (device to device):        %.2f ms per batch (median of %d; best %.2f)" % (copy[0], reps, copy[1]))
    print("  rc_correct_device of the batch (copy of the arena included), no session open: %.2f ms (median of %d); with a session open: %.2f ms"
          % (closed[0], reps, opened[0]))
    print("  %d of %d pairs overlap; %d of %d compared bases disagree before correction (%.6f), %d of %d after (%.6f); resolved %d, kept %d, introduced %d"
          % (c["overlapping"], c["pairs"], c["disagree_before"], c["compared_before"], c["disagree_before"] / max(1, c["compared_before"]), c["disagree_after"],
             c["compared_after"], c["disagree_after"] / max(1, c["compared_after"]), c["resolved"], c["kept"], c["introduced"]))
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
        print("bench.py --gpus 1 --steps %d --warmup 1 (config 2, no session open), ms_per_step, runs alternating on one GPU:" % a.bench_steps)
        print("  this commit: %s  median %.2f" % (" ".join("%.2f" % x for x in here), mh))
        print("  its parent:  %s  median %.2f" % (" ".join("%.2f" % x for x in there), mt))
        print("  this commit / parent = %.4f (%+.2f %%)" % (mh / mt, (mh / mt - 1.0) * 100.0))


if __name__ == "__main__":
    main()
