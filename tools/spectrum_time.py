#!/usr/bin/env python3
"""Times the two k-mer count spectrum kernels on one GPU (run it under `rocprofv3 --kernel-trace --stats` for the kernel
times; the wall-clock figures printed here include the launch, the read-back and the host's share).

  * table scan (k_spectrum_table): synthetic k = 31 tables of about 80 M and 800 M entries with Zipf-like counts, built
    on the device (rc_table_build_device); prints the table's bytes and the wall time per rc_table_spectrum call
  * counted spectrum (k_spectrum_counts, inside count_finish): the headline count -- bench.py preset 2, 25 M x 150 bp
    reads, k = 23 -- finished with the spectrum off and armed, alternately; prints the median of each

    python tools/spectrum_time.py [--sizes 80,800] [--reps 5] [--count-reps 3]
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import rcorrector_amd  # noqa: E402
import synth_int  # noqa: E402


def skewed_table(ctx, n, k, dev):
    """n distinct codes (an odd multiplier is a bijection of the 2k-bit space), counts 2 + floor(u^-1.5) capped at 10^6"""
    mask = (1 << (2 * k)) - 1
    i = torch.arange(n, dtype=torch.int64, device=dev)
    codes = (i * 0x5851F42D4C957F2D) & mask
    g = torch.Generator(device=dev)
    g.manual_seed(n)
    u = torch.rand(n, generator=g, device=dev, dtype=torch.float64).clamp_min(1e-12)
    counts = (2.0 + torch.floor(u.pow(-1.5))).clamp_max(1e6).to(torch.int32)
    del u
    torch.cuda.synchronize()
    ctx.table_build_device(codes, counts, n)
    del codes, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="80,800", help="table entries, millions")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count-reps", type=int, default=3)
    ap.add_argument("--max-bin", type=int, default=10000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for m in [int(x) for x in a.sizes.split(",") if x]:
        ctx = rcorrector_amd.Context(k=31)
        skewed_table(ctx, m * 1_000_000, 31, dev)
        st = ctx.table_stats()
        ts = []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            f, s = ctx.kmer_spectrum("table", a.max_bin)
            if r:
                ts.append(time.perf_counter() - t0)
        print("table %d M entries: %d live, %.3f GB of buckets (layout %d), spectrum call median %.3f ms (wall), total count %d, max %d"
              % (m, s["distinct"], st["bytes"] / 1e9, ctx.table_layout(), 1e3 * statistics.median(ts), s["total"], s["max_count"]),
              flush=True)
        ctx.close()
        torch.cuda.empty_cache()
    if a.count_reps:
        P = dict(reads=25_000_000, len=150, paired=True, k=23, err=0.005, alpha=0.8, seed=1002)
        gen = synth_int.Synth(P["seed"], P["len"], 30000, 1500, P["alpha"], P["err"], P["paired"], device=dev)
        seq, _ = gen.generate(0, P["reads"] // 2)
        torch.cuda.synchronize()
        ctx = rcorrector_amd.Context(k=P["k"])
        t = {0: [], a.max_bin: []}
        for r in range(2 * a.count_reps + 2):
            arm = a.max_bin if r % 2 else 0
            ctx.count_spectrum(arm)
            ctx.count_begin()
            ctx.count_add_device(seq, seq.numel())
            t0 = time.perf_counter()
            n = ctx.count_finish(2)
            dt = time.perf_counter() - t0
            if r >= 2:   # (the first of each: warm-up)
                t[arm].append(dt)
        off, on = statistics.median(t[0]), statistics.median(t[a.max_bin])
        f, s = ctx.kmer_spectrum("counted", a.max_bin)
        print("count_finish 25 M x 150 bp, k 23: %d kept, %d distinct (%d once); median off %.1f ms, armed %.1f ms (%+.2f %%); off %s, armed %s"
              % (n, s["distinct"], s["unique"], 1e3 * off, 1e3 * on, 100.0 * (on - off) / off,
                 ["%.1f" % (1e3 * x) for x in t[0]], ["%.1f" % (1e3 * x) for x in t[a.max_bin]]), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
