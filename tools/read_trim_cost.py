#!/usr/bin/env python3
"""What tools/read_trim's kernel costs per batch, measured on one arena of bench.py's headline shard (config 2: 25 M x 150 bp
paired reads, two halves: mode 1) and on a shard of the same shape whose pairs overlap (--frag, 220-base fragments: the
benchmark's own 300-base fragments of 150-base reads do not):
  * rc_read_trim_device with only the pair cut on, beside rc_mate_overlap_device in the same run on the same arena, passed as
    both versions: the same stage and the same offset scan, so the ratio is reported;
  * rc_read_trim_device with all three cuts on (the defaults of tools/read_trim);
  * a device-to-device copy of the bytes the kernel reads and writes (bases, qualities, offsets in; 16 B a read, 1 B a unit out).
Events around each call on a drained context, a warm-up of each, then the median of --reps runs, alternating.  With --parent DIR
(a built checkout of the parent commit) it then runs `bench.py --gpus 1 --steps K --warmup 1` -- the benchmark's step, which runs
none of this -- in this tree and in DIR, alternating, --bench-rounds times each, every run a process of its own on the same GPU.
Prints the lines of profiles/read_trim_cost.txt.

    python tools/read_trim_cost.py [--reads N] [--frag F] [--reps R] [--parent DIR] [--bench-rounds B] [--bench-steps K]"""
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
from rcorrector_amd.binding import OVERLAP_WORDS, TRIM_TALLY_WORDS, mate_overlap_dict, trim_params, trim_tally_dict  # noqa: E402


def shard(P, n, frag, reps, dev):
    L = P["len"]
    gen = synth_int.Synth(P["seed"], L, 30000, 1500, P["alpha"], P["err"], P["paired"], frag_len=frag, bias3=P["bias3"], device=dev)
    ctx = rcorrector_amd.Context(k=P["k"], max_fix_per_k=P["maxcork"], device=0)      # (no table: neither kernel needs one)
    seq, qual = gen.generate(0, n // 2)
    torch.cuda.synchronize()
    nbytes = n * (L + 1)
    off = (torch.arange(n + 1, device=dev, dtype=torch.int64) * (L + 1)).to(torch.int32)
    counts = torch.zeros(OVERLAP_WORDS, dtype=torch.int64, device=dev)
    tally = torch.zeros(TRIM_TALLY_WORDS, dtype=torch.int64, device=dev)
    rows = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    keep = torch.zeros(n // 2, dtype=torch.uint8, device=dev)
    moved = 2 * nbytes + 4 * (n + 1) + 16 * n + n // 2
    src, dst = torch.zeros(moved, dtype=torch.uint8, device=dev), torch.zeros(moved, dtype=torch.uint8, device=dev)
    pair_only = trim_params(qual_min=0, adapter1=b"", min_len=0)
    every_cut = trim_params()

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

    calls = [lambda: ctx.read_trim_device(seq, None, off, n, nbytes, L, 1, pair_only, rows, keep, tally),
             lambda: ctx.mate_overlap_device(seq, seq, off, n, nbytes, L, 1, counts),
             lambda: ctx.read_trim_device(seq, qual, off, n, nbytes, L, 1, every_cut, rows, keep, tally),
             lambda: dst.copy_(src)]
    for c in calls:                                             # warm-up: code objects
        event_ms(c)
    counts.zero_()
    tally.zero_()
    event_ms(calls[0])
    t_pair = trim_tally_dict(tally.cpu().numpy())
    event_ms(calls[1])
    rep = mate_overlap_dict(counts.cpu().numpy())
    assert t_pair["pairs_overlapping"] == rep["overlapping"] and t_pair["units"] == rep["pairs"]      # the same d* accepted in both
    tally.zero_()
    event_ms(calls[2])
    t_all = trim_tally_dict(tally.cpu().numpy())
    ms = [[], [], [], []]
    for _ in range(reps):                                       # alternating, so that none has the warmer caches
        for x, c in enumerate(calls):
            ms[x].append(event_ms(c))
    m = [statistics.median(x) for x in ms]
    rng = lambda x: "%.2f..%.2f" % (min(x), max(x))   # noqa: E731
    print("shard: %d reads x %d bases (paired, two halves, %d-base fragments), %d arena bytes; medians of %d runs, events around the call" % (n, L, frag, nbytes, reps))
    print("  k_read_trim, the pair cut alone (no qualities, no adapter):  %.2f ms per batch (%s)" % (m[0], rng(ms[0])))
    print("  k_mate_overlap on the same arena, passed as both versions:   %.2f ms per batch (%s); k_read_trim / k_mate_overlap = %.3f" % (m[1], rng(ms[1]), m[0] / m[1]))
    print("  k_read_trim, all three cuts (q 20, the 13-base adapter on both mates, the pair cut): %.2f ms per batch (%s)" % (m[2], rng(ms[2])))
    print("  device-to-device copy of the %d bytes it reads and writes:    %.2f ms (%s); all three cuts / copy = %.1f" % (moved, m[3], rng(ms[3]), m[2] / m[3]))
    print("  the pair cut alone: %d of %d pairs overlap, %d + %d reads cut, %d bases removed" %
          (t_pair["pairs_overlapping"], t_pair["units"], t_pair["cut_reads"][0][2], t_pair["cut_reads"][1][2], int(t_pair["bases_removed"].sum())))
    print("  all three cuts: reads cut by quality %d + %d, by adapter %d + %d, by pair %d + %d; %d of %d pairs kept at min_len 20, %d bases removed" %
          (t_all["cut_reads"][0][0], t_all["cut_reads"][1][0], t_all["cut_reads"][0][1], t_all["cut_reads"][1][1], t_all["cut_reads"][0][2], t_all["cut_reads"][1][2],
           t_all["units_kept"], t_all["units"], int(t_all["bases_removed"].sum())))
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
