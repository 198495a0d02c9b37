#!/usr/bin/env python3
"""What tools/read_normalize's selection costs per batch, measured: rc_norm_select_device (k_norm_select, rc_profile_get's kernel
9) over the depths of one resident arena of bench.py's headline shard (config 2: 25 M x 150 bp paired reads = 12.5 M pairs,
k = 23) after correction, beside two yardsticks in the same process: rc_read_depth_device on the same arena (kernel 7: the launch
that makes the selection's input) and a device-to-device copy of the bytes the selection reads and writes (32 B in and 1 B out
per pair).  A warm-up of each, then the median of --reps runs, the three alternating; every GPU step runs under a time limit
(SIGALRM ends the process).  Prints the lines of profiles/read_normalize_cost.txt.

    python tools/read_normalize_cost.py [--reads N] [--reps R] [--target T] [--limit SECONDS]"""
import argparse
import os
import signal
import sys

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
    ap.add_argument("--target", type=int, default=None, help="default: the shard's median pair depth")
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
    depth = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    units, max_bin = n // 2, 10000
    keep = torch.zeros(units, dtype=torch.uint8, device=dev)
    tally = torch.zeros(4 + 2 * (max_bin + 1), dtype=torch.int64, device=dev)
    src, dst = torch.zeros(33 * units, dtype=torch.uint8, device=dev), torch.zeros(33 * units, dtype=torch.uint8, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def correct():
        ctx.correct_device(1, n, nbytes, L, seq, qual, off, *res)
        ctx.sync()

    def timed(kernel, call):
        ctx.profile_reset()
        call()
        ctx.sync()
        return ctx.profile_get(kernel)[0]

    def copy_ms():
        ev[0].record()
        dst.copy_(src)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    step(correct)                                               # (the arena is corrected in place: what the tool is run on)
    step(lambda: (ctx.read_depth_device(seq, off, n, nbytes, L, depth), ctx.sync()))
    med = depth[:, 2].view(units, 2).to(torch.int64)            # (the shard's reads are interleaved pairs: mode 2)
    target = a.target or max(1, int(((med[:, 0] + med[:, 1] + 1) >> 1).median().item()))
    select = lambda: ctx.norm_select_device(depth, units, 2, 0, target, 2, 1, max_bin, keep, tally)   # noqa: E731
    step(lambda: (select(), ctx.sync(), copy_ms()))             # warm-up: code objects
    tally.zero_()
    ctx.profile(True)
    ms = [[], [], []]
    for _ in range(a.reps):                                     # alternating, so that none has the warmer caches
        ms[0].append(step(lambda: timed(9, select)))
        ms[1].append(step(lambda: timed(7, lambda: ctx.read_depth_device(seq, off, n, nbytes, L, depth))))
        ms[2].append(step(copy_ms))
    ctx.profile(False)
    m = [float(np.median(x)) for x in ms]
    t = tally.cpu().numpy() // a.reps
    runs = lambda x: " ".join("%.3f" % v for v in x)   # noqa: E731
    print("shard: %d reads x %d bases = %d pairs (mode 2), k = %d, %d k-mers in the table; medians of %d runs" % (n, L, units, k, n_kmers, a.reps))
    print("k_norm_select (profile kernel 9): %.3f ms per batch (runs: %s)" % (m[0], runs(ms[0])))
    print("k_read_depth on the same arena (profile kernel 7): %.3f ms per batch (runs: %s)" % (m[1], runs(ms[1])))
    print("device-to-device copy of %d bytes (32 B in + 1 B out per pair): %.3f ms (runs: %s)" % (33 * units, m[2], runs(ms[2])))
    print("ratio k_norm_select / k_read_depth: %.4f; k_norm_select / copy: %.2f" % (m[0] / m[1], m[0] / m[2]))
    print("per pair: k_norm_select %.3f ns, k_read_depth %.2f ns; k_norm_select moves %.0f GB/s" % (m[0] * 1e6 / units, m[1] * 1e6 / units,
                                                                                                      33 * units / m[0] / 1e6))
    print("target %d (the median pair depth), min_cov 2, seed 1: kept %d, over %d, low %d, novalid %d of %d pairs; %d distinct depth bins, the fullest holds %d"
          % (target, t[1], t[0], t[2], t[3], units, int((t[4:4 + max_bin + 1] > 0).sum()), int(t[4:4 + max_bin + 1].max())))


if __name__ == "__main__":
    main()
