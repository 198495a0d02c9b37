#!/usr/bin/env python3
"""What -weak-ends / rc_weak_profile_into costs per batch, measured: rc_weak_profile_device (both launches, rc_profile_get's
kernel 4) over one arena of bench.py's headline shard (config 2: 25 M x 150 bp paired reads, k = 23) after correction, beside
the probe work of the correction itself on the same arena (kernel 0: the fused probe + threshold launch,
k_probe_threshold_list).  Both probe every base of the arena once.  Prints the lines of profiles/weak_profile_cost.txt.

    python tools/weak_profile_cost.py [--reads N] [--reps R]"""
import argparse
import os
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
    out = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def correct():
        work.copy_(seq)
        torch.cuda.synchronize()
        ctx.correct_device(1, n, nbytes, L, work, qual, off, *res)
        ctx.sync()

    correct()                                                   # warm-up: code objects, scratch
    ctx.weak_profile_device(work, off, n, nbytes, L, out, 1)
    ctx.sync()
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(a.reps):
        correct()
    probe_ms, probe_n = ctx.profile_get(0)
    ctx.profile_reset()
    for _ in range(a.reps):
        ctx.weak_profile_device(work, off, n, nbytes, L, out, 1)
    ctx.sync()
    weak_ms, weak_n = ctx.profile_get(4)
    ctx.profile(False)
    w = out.cpu().numpy()
    plane_bytes = 2 * ((nbytes + 4095) // 4096) * 512
    print("shard: %d reads x %d bases (paired), k = %d, %d k-mers in the table, %d arena bytes" % (n, L, k, n_kmers, nbytes))
    print("fused probe + threshold launch of the correction (k_probe_threshold_list, profile kernel 0): %.2f ms per batch (%d launches in %d batches)"
          % (probe_ms / a.reps, probe_n, a.reps))
    print("rc_weak_profile_device, both launches (k_weak_planes + k_weak_reduce, profile kernel 4): %.2f ms per batch (%d calls in %d batches)"
          % (weak_ms / a.reps, weak_n, a.reps))
    print("bytes written per base: bit planes %.3f + results %.3f (16 bytes per read) = %.3f; k_probe's counts would be 4"
          % (plane_bytes / (n * L), 16.0 / L, plane_bytes / (n * L) + 16.0 / L))
    print("of the corrected reads at min_count 1: %d weak windows, %d reads with a bad prefix, %d with a bad suffix, %d without a solid k-mer"
          % (int(w[:, 0].sum(dtype=np.int64)), int((w[:, 1] > 0).sum()), int((w[:, 2] > 0).sum()), int((w[:, 3] == L).sum())))


if __name__ == "__main__":
    main()
