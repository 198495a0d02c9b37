#!/usr/bin/env python3
"""What `-histo-after` (the recount session, rc_recount_begin ... rc_recount_finish) costs, on one GPU.

  cli    (default) writes the headline shape -- bench.py preset 2: 25 M x 150 bp pairs, k = 23 -- as two FASTQ files once, then
         runs `rcorrector -p a b -k 23` (no -c: one pass, the bases counted and corrected in HBM) --reps times each without
         and with `-histo-after`, RC_COUNT_TIMING=1 and RC_TIMING=1 set: prints every run's whole-process time, the
         counting phase's time (`[rc count timing] finish`), the recount's (`[rc recount timing]`), the medians, the
         overhead (c) - (b) and its ratio to the counting time.  --binary PATH times another build (the parent commit's)
         the same way with --plain-only, for (a).
  finish recount_finish alone over the same reads in HBM, --reps times: run this one under
         `rocprofv3 --kernel-trace --stats -- python tools/recount_time.py finish` for k_census' own time; prints the distinct
         k-mers probed, so that bytes/s = distinct * 64 / kernel time (a 64-byte bucket per probe) can be put next to the
         probe kernel's figure of profiles/r6_*.

Every GPU step (each `rcorrector` run, the finish loop) is a child process under its own `timeout`; the chain stops at the
first one that fails.

    python tools/recount_time.py [cli|finish] [--reads 25000000] [--reps 3] [--dir DIR] [--binary PATH] [--limit SECONDS]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
P = dict(len=150, k=23, err=0.005, alpha=0.8, seed=1002)


def step(cmd, limit, env=None):
    """one GPU step: a child under `timeout`; anything but success ends the chain"""
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        sys.stderr.write(p.stderr.decode(errors="replace")[-4000:])
        sys.exit("recount_time: `%s` ended with status %d: stopping here" % (" ".join(cmd[:3]), p.returncode))
    return dt, p


def write_reads(a):
    """child process: the headline reads as FASTQ (qualities 'I'), generated on the GPU piece by piece"""
    import numpy as np
    import torch
    import synth_int
    dev = torch.device("cuda:0")
    gen = synth_int.Synth(P["seed"], P["len"], 30000, 1500, P["alpha"], P["err"], True, device=dev)
    L, n_pairs, piece = P["len"], a.reads // 2, 1 << 20
    qual = b"I" * L
    with open(os.path.join(a.dir, "r_1.fq"), "wb") as f1, open(os.path.join(a.dir, "r_2.fq"), "wb") as f2:
        for lo in range(0, n_pairs, piece):
            m = min(piece, n_pairs - lo)
            seq, _ = gen.generate(lo, m)   # first mates, then second mates, L + 1 bytes a read
            s = seq.cpu().numpy().reshape(2 * m, L + 1)[:, :L]
            for f, rows, tag in ((f1, s[:m], b"/1"), (f2, s[m:], b"/2")):
                rec = np.empty((m, 2 * L + 16 + 4), dtype=np.uint8)   # "@%012d/1\n" seq "\n+\n" qual "\n"
                ids = np.char.zfill(np.arange(lo, lo + m).astype("S12"), 12)
                rec[:, 0] = ord("@")
                rec[:, 1:13] = np.frombuffer(ids.tobytes(), dtype=np.uint8).reshape(m, 12)
                rec[:, 13:15] = np.frombuffer(tag, dtype=np.uint8)
                rec[:, 15] = 10
                rec[:, 16:16 + L] = rows
                rec[:, 16 + L:19 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
                rec[:, 19 + L:19 + 2 * L] = np.frombuffer(qual, dtype=np.uint8)
                rec[:, 19 + 2 * L] = 10
                f.write(rec.tobytes())


def finish_loop(a):
    """child process: recount_finish alone over the headline reads in HBM"""
    import torch
    import rcorrector_amd
    import synth_int
    dev = torch.device("cuda:0")
    gen = synth_int.Synth(P["seed"], P["len"], 30000, 1500, P["alpha"], P["err"], True, device=dev)
    seq, _ = gen.generate(0, a.reads // 2)
    torch.cuda.synchronize()
    ctx = rcorrector_amd.Context(k=P["k"])
    ctx.count_begin()
    ctx.count_add_device(seq, seq.numel())
    ctx.count_finish(2)
    ts = []
    for r in range(a.reps + 1):
        ctx.recount_begin(10000)
        ctx.recount_add_device(seq, seq.numel())
        t0 = time.perf_counter()
        f, s = ctx.recount_finish()
        if r:
            ts.append(time.perf_counter() - t0)
    st = ctx.table_stats()
    print("recount_finish %d x %d bp, k %d: %d distinct k-mers probed (%d once, %d not in the table of %d entries, %.3f GB, layout %d); "
          "median %.1f ms (wall) %s" % (a.reads, P["len"], P["k"], s["distinct"], s["unique"], s["absent_distinct"], st["entries"], st["bytes"] / 1e9,
                                        ctx.table_layout(), 1e3 * statistics.median(ts), ["%.1f" % (1e3 * x) for x in ts]), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="cli", choices=["cli", "finish", "_write", "_finish"])
    ap.add_argument("--reads", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "recount_time"))
    ap.add_argument("--binary", default=os.path.join(ROOT, "rcorrector_amd", "rcorrector"))
    ap.add_argument("--plain-only", action="store_true", help="only runs without -histo-after (a build that does not know the flag)")
    ap.add_argument("--limit", type=int, default=240, help="seconds a GPU step may take")
    a = ap.parse_args()
    if a.what == "_write":
        return write_reads(a)
    if a.what == "_finish":
        return finish_loop(a)
    me = [sys.executable, os.path.abspath(__file__)]
    common = ["--reads", str(a.reads), "--reps", str(a.reps), "--dir", a.dir]
    if a.what == "finish":
        _, p = step(me + ["_finish"] + common, a.limit, dict(os.environ, RC_COUNT_TIMING="1"))
        sys.stdout.write("".join(ln + "\n" for ln in p.stderr.decode(errors="replace").splitlines() if ln.startswith("[rc ")))
        sys.stdout.write(p.stdout.decode())
        return
    os.makedirs(a.dir, exist_ok=True)
    f1, f2 = os.path.join(a.dir, "r_1.fq"), os.path.join(a.dir, "r_2.fq")
    if not (os.path.exists(f1) and os.path.exists(f2)):
        step(me + ["_write"] + common, a.limit)
    env = dict(os.environ, RC_COUNT_TIMING="1", RC_TIMING="1", RC_QUIET="1")
    times = {False: [], True: []}
    count_s, recount_s = [], []
    for r in range(2 * (a.reps + 1)):   # (the first of each: warm-up -- the page cache, the code objects)
        flag = bool(r % 2)
        if flag and a.plain_only:
            continue
        cmd = [a.binary, "-p", f1, f2, "-k", str(P["k"]), "-od", a.dir] + (["-histo-after", os.path.join(a.dir, "after.histo")] if flag else [])
        dt, p = step(cmd, a.limit, env)
        err = p.stderr.decode(errors="replace")
        m = re.search(r"\[rc count timing\] finish ([0-9.]+) s", err)
        m2 = re.search(r"\[rc recount timing\] finish ([0-9.]+) s.*", err)
        print("run %d %s: %.3f s whole process; counting finish %s s%s" % (r, "-histo-after" if flag else "plain", dt, m.group(1) if m else "?",
                                                                          ("; " + m2.group(0)) if m2 else ""), flush=True)
        if r >= 2:
            times[flag].append(dt)
            if m:
                count_s.append(float(m.group(1)))
            if m2:
                recount_s.append(float(m2.group(1)))
    if a.plain_only:
        print("%s: median without the flag %.3f s %s" % (a.binary, statistics.median(times[False]), ["%.3f" % x for x in times[False]]), flush=True)
        return
    b, c = statistics.median(times[False]), statistics.median(times[True])
    cnt = statistics.median(count_s) if count_s else float("nan")
    print("%s: median without the flag %.3f s %s, with -histo-after %.3f s %s: overhead %.3f s (%+.1f %%); counting phase %.3f s, recount finish %.3f s; "
          "overhead / counting = %.2f" % (os.path.basename(a.binary), b, ["%.3f" % x for x in times[False]], c, ["%.3f" % x for x in times[True]], c - b,
                                         100.0 * (c - b) / b, cnt, statistics.median(recount_s) if recount_s else float("nan"), (c - b) / cnt), flush=True)
    for line in open(os.path.join(a.dir, "after.histo")).read().splitlines()[:3]:
        print("after.histo:", line)


if __name__ == "__main__":
    main()
