#!/usr/bin/env python3
"""What -depth-tags / -depth / rc_read_depth_into costs per batch, measured: rc_read_depth_device (k_read_depth, rc_profile_get's
kernel 7) over one resident arena of bench.py's headline shard (config 2: 25 M x 150 bp paired reads, k = 23) after correction,
beside the weak-k-mer profile's two launches on the same arena in the same process (kernel 4: it makes the same one probe per
base) and the batch's correction.  A warm-up of each, then the median of --reps runs; every GPU step runs under a time limit
(SIGALRM ends the process).  Prints the lines of profiles/read_depth_cost.txt.

    python tools/read_depth_cost.py [--reads N] [--reps R] [--limit SECONDS]"""
import argparse
import os
import signal
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import bench  # noqa: E402
import rcorrector_amd  # noqa: E402
import synth_int  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds a GPU step may take")
    a = ap.parse_args()

    def step(fn):
        signal.alarm(a.limit)
        r = fn()
        signal.alarm(0)
        return r

    P = dict(bench.PRESETS[2])
    n = a.reads or P["reads"]
    L, k = P["len"], P["k"]
    dev = torch.device("cuda", 0)
    gen = synth_int.Synth(P["seed"], L, 30000, 1500, P["alpha"], P["err"], P["paired"], bias3=P["bias3"], device=dev)
    ctx = rcorrector_amd.Context(k=k, max_fix_per_k=P["maxcork"], device=0)
    seq, qual = step(lambda: gen.generate(0, n // 2))
    torch.cuda.synchronize()

    def count():
        ctx.count_begin()
        ctx.count_add_device(seq, seq.numel())
        return ctx.count_finish(2)

    n_kmers = step(count)
    fh = torch.bincount(qual[0::(L + 1)][:1000000].long(), minlength=300)[:300].cpu().numpy().astype(np.int32)
    lh = torch.bincount(qual[L - 1::(L + 1)][:1000000].long(), minlength=300)[:300].cpu().numpy().astype(np.int32)
    ctx.set_run_params(ctx.estimate_error_rate(0.95), ctx.bad_quality_from_hist(fh, lh, min(n, 1000000)))
    nbytes = n * (L + 1)
    off = (torch.arange(n + 1, device=dev, dtype=torch.int64) * (L + 1)).to(torch.int32)
    res = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4)]
    out = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    wout = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def correct():
        work.copy_(seq)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.correct_device(1, n, nbytes, L, work, qual, off, *res)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    def timed(kernel, call):
        ctx.profile_reset()
        call()
        ctx.sync()
        return ctx.profile_get(kernel)[0]

    depth = lambda: ctx.read_depth_device(work, off, n, nbytes, L, out)            # noqa: E731
    weak = lambda: ctx.weak_profile_device(work, off, n, nbytes, L, wout, 1)       # noqa: E731
    step(correct)                                               # warm-up: code objects, scratch
    step(lambda: (depth(), weak(), ctx.sync()))
    correct_ms = [step(correct) for _ in range(a.reps)]         # (the last one leaves the corrected arena in `work`)
    ctx.profile(True)
    depth_ms, weak_ms = [], []
    for _ in range(a.reps):                                     # alternating, so that neither has the warmer caches
        depth_ms.append(step(lambda: timed(7, depth)))
        weak_ms.append(step(lambda: timed(4, weak)))
    ctx.profile(False)
    d = out.cpu().numpy()
    md, mw, mc = float(np.median(depth_ms)), float(np.median(weak_ms)), float(np.median(correct_ms))
    print("shard: %d reads x %d bases (paired), k = %d, %d k-mers in the table, %d arena bytes; medians of %d runs" % (n, L, k, n_kmers, nbytes, a.reps))
    print("rc_read_depth_device (k_read_depth, profile kernel 7): %.2f ms per batch (runs: %s)" % (md, " ".join("%.2f" % x for x in depth_ms)))
    print("rc_weak_profile_device, both launches (k_weak_planes + k_weak_reduce, profile kernel 4): %.2f ms per batch (runs: %s)"
          % (mw, " ".join("%.2f" % x for x in weak_ms)))
    print("ratio k_read_depth / weak profile: %.2f" % (md / mw))
    print("rc_correct_device, the batch's correction (host clock around the call and its sync): %.2f ms per batch (runs: %s)"
          % (mc, " ".join("%.2f" % x for x in correct_ms)))
    print("k_read_depth per read: %.2f ns; bytes written per base: %.3f (16 bytes per read, nothing else)" % (md * 1e6 / n, 16.0 / L))
    has = d[:, 0] > 0
    print("of the corrected reads: %d with a valid window, %d of them with a median of 0, median of the medians %d, largest q3 %d"
          % (int(has.sum()), int((d[has, 2] == 0).sum()), int(np.sort(d[has, 2])[(int(has.sum()) - 1) // 2]) if has.any() else 0, int(d[:, 3].max())))


if __name__ == "__main__":
    main()
