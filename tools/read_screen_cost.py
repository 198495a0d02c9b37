#!/usr/bin/env python3
"""What tools/read_screen / rc_read_screen_into costs per batch, measured: rc_read_screen_device (k_read_screen, rc_profile_get's
kernel 8) over one resident arena of bench.py's headline shard (config 2: 25 M x 150 bp paired reads, k = 23) after correction,
against the run's own table (every window a hit) and against a small unrelated table (nearly every window a miss), beside
rc_read_depth_device on the same arena in the same process (kernel 7: the yardstick -- it makes the same one probe per base into
the run's own table).  A warm-up of each, then the median of --reps runs, the three alternating; every GPU step runs under a
time limit (SIGALRM ends the process).  Prints the lines of profiles/read_screen_cost.txt.

    python tools/read_screen_cost.py [--reads N] [--reps R] [--limit SECONDS]"""
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
    out = [torch.zeros((n, 4), dtype=torch.int32, device=dev) for _ in range(3)]
    # the unrelated set: the k-mers of 200 000 random bases, as a reference set's -- each once
    other = rcorrector_amd.Context(k=k, device=0)
    rnd = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(7).integers(0, 4, size=200000)]
    other.count_begin()
    other.count_add(np.concatenate([rnd, np.zeros(1, np.uint8)]))
    n_other = step(lambda: other.count_finish(1))

    def correct():
        ctx.correct_device(1, n, nbytes, L, seq, qual, off, *res)
        ctx.sync()

    def timed(kernel, call):
        ctx.profile_reset()
        call()
        ctx.sync()
        return ctx.profile_get(kernel)[0]

    calls = [(8, lambda: ctx.read_screen_device(ctx, seq, off, n, nbytes, L, out[0], min_count=1)),
             (8, lambda: ctx.read_screen_device(other, seq, off, n, nbytes, L, out[1], min_count=1)),
             (7, lambda: ctx.read_depth_device(seq, off, n, nbytes, L, out[2]))]
    step(correct)                                               # (the arena is corrected in place: what a registration would see)
    for _, call in calls:                                       # warm-up: code objects
        step(lambda: (call(), ctx.sync()))
    ctx.profile(True)
    ms = [[], [], []]
    for _ in range(a.reps):                                     # alternating, so that none has the warmer caches
        for i, (kernel, call) in enumerate(calls):
            ms[i].append(step(lambda: timed(kernel, call)))
    ctx.profile(False)
    med = [float(np.median(x)) for x in ms]
    own, far, depth = (o.cpu().numpy() for o in out)
    runs = lambda x: " ".join("%.2f" % v for v in x)   # noqa: E731
    print("shard: %d reads x %d bases (paired), k = %d, %d k-mers in the table, %d arena bytes; medians of %d runs" % (n, L, k, n_kmers, nbytes, a.reps))
    print("k_read_screen against the run's own table (profile kernel 8): %.2f ms per batch (runs: %s)" % (med[0], runs(ms[0])))
    print("k_read_screen against an unrelated table of %d k-mers (profile kernel 8): %.2f ms per batch (runs: %s)" % (n_other, med[1], runs(ms[1])))
    print("k_read_depth on the same arena (profile kernel 7): %.2f ms per batch (runs: %s)" % (med[2], runs(ms[2])))
    print("ratio k_read_screen / k_read_depth: own table %.3f, unrelated table %.3f" % (med[0] / med[2], med[1] / med[2]))
    print("k_read_screen per read: %.2f ns (own table), %.2f ns (unrelated table); k_read_depth %.2f ns" % tuple(m * 1e6 / n for m in med))
    print("own table: %d of %d valid windows are hits, %d reads all hits; unrelated table: %d hits in %d reads; valid windows equal to k_read_depth's: %s"
          % (int(own[:, 1].sum()), int(own[:, 0].sum()), int(((own[:, 1] == own[:, 0]) & (own[:, 0] > 0)).sum()), int(far[:, 1].sum()),
             int((far[:, 1] > 0).sum()), bool((own[:, 0] == depth[:, 0]).all() and (far[:, 0] == depth[:, 0]).all())))


if __name__ == "__main__":
    main()
