#!/usr/bin/env python3
"""What rc_table_compare costs, measured: the benchmark's table (bench.py config 2: 25 M x 150 bp paired reads, k = 23, the
k-mers counted twice or more) against a seeded variant of itself -- the same codes with about a tenth replaced by fresh
ones, counts redrawn (2 + a Zipf-like tail) -- per call and per scanned entry; beside it, in the same visit,
rc_table_spectrum(source 0) on each table (the same scan without the probes: the floor) and the all-one-cell case (the
variant's codes with every count 2 against a second table of the same codes with every count 3: what the LDS corner and
the wavefront's shared add are for).
Wall time around the call (it is complete on return), median of --reps.  With --parent DIR (a built checkout of the
parent commit) it then runs `bench.py --gpus 1 --steps K --warmup 1` in this tree and in DIR, alternating, --bench-rounds
times each, prints every ms_per_step, both medians and ranges, and the fused probe kernel's time per probe from this tree's
own bench lines (roofline.avg_launch_ms over alg_bytes_per_launch / 64).  Prints the lines of profiles/table_compare_cost.txt.

    python tools/table_compare_cost.py [--reads N] [--reps R] [--max-bin B] [--parent DIR] [--bench-rounds B] [--bench-steps K]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import bench  # noqa: E402
import rcorrector_amd  # noqa: E402
import synth_int  # noqa: E402
from dup_census_cost import timed  # noqa: E402


def bench_line(tree, steps):
    """the JSON result line of one `bench.py` run in `tree`"""
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1"], cwd=tree, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600, check=True)
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-bin", type=int, default=255)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: also compare bench.py's step there and here")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=3)
    a = ap.parse_args()
    P = dict(bench.PRESETS[2])
    n, L, k = a.reads or P["reads"], P["len"], P["k"]
    dev = torch.device("cuda", 0)
    gen = synth_int.Synth(P["seed"], L, 30000, 1500, P["alpha"], P["err"], P["paired"], bias3=P["bias3"], device=dev)
    seq, _ = gen.generate(0, n // 2)
    torch.cuda.synchronize()
    ta = rcorrector_amd.Context(k=k)
    ta.count_begin()
    ta.count_add_device(seq, seq.numel())
    n_kmers = ta.count_finish(2)
    del seq, gen
    torch.cuda.empty_cache()
    codes, _ = ta.table_export()
    rng = np.random.default_rng(79)
    fresh = rng.random(len(codes)) < 0.1
    codes = codes.copy()
    codes[fresh] = rng.integers(0, 1 << (2 * k), size=int(fresh.sum()), dtype=np.uint64)
    counts = (2.0 + np.floor(np.maximum(rng.random(len(codes)), 1e-12) ** -1.5)).clip(max=1e6).astype(np.int32)
    tb, flat, flat3 = rcorrector_amd.Context(k=k), rcorrector_amd.Context(k=k), rcorrector_amd.Context(k=k)
    tb.table_build(codes, counts)
    flat.table_build(codes, np.full(len(codes), 2, np.int32))
    flat3.table_build(codes, np.full(len(codes), 3, np.int32))
    del codes, counts
    nothing = lambda: None   # noqa: E731  (table_compare and kmer_spectrum are complete on return)
    for name, x, y in (("spread", ta, tb), ("one cell", flat, flat3)):
        r = x.table_compare(y, a.max_bin)     # warm-up: code objects
        ms = timed(lambda: x.table_compare(y, a.max_bin), nothing, a.reps)
        scanned = r["distinct_a"] + r["distinct_b"]
        sx, sy = x.table_stats(), y.table_stats()
        print("%s: a %d k-mers (layout %d, %.3f GB of buckets), b %d k-mers (layout %d, %.3f GB); shared %d, non-zero cells %d of %d, largest cell %.1f %% of the k-mers"
              % (name, r["distinct_a"], x.table_layout(), sx["bytes"] / 1e9, r["distinct_b"], y.table_layout(), sy["bytes"] / 1e9, r["shared"],
                 int((r["cells"] != 0).sum()), r["cells"].size, 100.0 * float(r["cells"].max()) / max(1, r["distinct_a"] + r["distinct_b"] - r["shared"])))
        print("  rc_table_compare(max_bin %d): %.2f ms per call (median of %d; best %.2f) = %.3f ns per scanned entry (both passes: %d entries, one probe each)"
              % (a.max_bin, ms[0], a.reps, ms[1], 1e6 * ms[0] / scanned, scanned))
        floor = []
        for t in (x, y):
            t.kmer_spectrum("table", a.max_bin)
            floor.append(timed(lambda: t.kmer_spectrum("table", a.max_bin), nothing, a.reps))
        print("  rc_table_spectrum(source 0), the same scans without the probes: a %.2f ms, b %.2f ms (medians; best %.2f, %.2f) = %.3f ns per entry; compare / floor = %.1f"
              % (floor[0][0], floor[1][0], floor[0][1], floor[1][1], 1e6 * (floor[0][0] + floor[1][0]) / scanned, ms[0] / (floor[0][0] + floor[1][0])))
        sys.stdout.flush()
    print("(the table the benchmark counts holds %d k-mers)" % n_kmers)
    if a.parent:
        for t in (ta, tb, flat, flat3):
            t.close()
        torch.cuda.empty_cache()
        here, there = [], []
        for _ in range(a.bench_rounds):
            here.append(bench_line(ROOT, a.bench_steps))
            there.append(bench_line(os.path.abspath(a.parent), a.bench_steps))
            print("  (round done: %.2f here, %.2f in the parent)" % (here[-1]["ms_per_step"], there[-1]["ms_per_step"]), file=sys.stderr, flush=True)
        roof = [h["roofline"] for h in here]
        per_probe = [1e6 * r["avg_launch_ms"] / (r["alg_bytes_per_launch"] / 64.0) for r in roof]
        print("the fused probe kernel in this tree's bench runs: %s ns per probe (avg_launch_ms over alg_bytes_per_launch / 64 probes)"
              % " ".join("%.4f" % x for x in per_probe))
        here, there = [h["ms_per_step"] for h in here], [t["ms_per_step"] for t in there]
        mh, mt = statistics.median(here), statistics.median(there)
        print("bench.py --gpus 1 --steps %d --warmup 1 (config 2, no compare anywhere), ms_per_step, runs alternating on one GPU:" % a.bench_steps)
        print("  this commit: %s  median %.2f  range %.2f .. %.2f" % (" ".join("%.2f" % x for x in here), mh, min(here), max(here)))
        print("  its parent:  %s  median %.2f  range %.2f .. %.2f" % (" ".join("%.2f" % x for x in there), mt, min(there), max(there)))
        print("  this commit / parent = %.4f (%+.2f %%); the ranges %s" % (mh / mt, (mh / mt - 1.0) * 100.0,
                                                                          "overlap" if min(here) <= max(there) and min(there) <= max(here) else "do not overlap"))


if __name__ == "__main__":
    main()
