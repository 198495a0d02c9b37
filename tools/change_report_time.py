#!/usr/bin/env python3
"""What the correction report (rc_change_report_begin ... rc_change_report_get, `rcorrector -report`) costs, on one GPU.

  step   (default) the headline shape -- bench.py preset 2: 25 M x 150 bp pairs, k = 23 -- generated in HBM, the table counted
         from it, then rc_correct_device over the whole shard --reps times each with the report off and armed, interleaved in one
         process (every step starts from a fresh copy of the uncorrected reads; the copy is outside the timed span): prints
         every step's time, the medians, the changes found, and the algorithmic bytes of the report kernel (two arena reads,
         the offsets, one quality byte per changed base) and of the snapshot copy (the arena read and written).  Run it under
         `rocprofv3 --kernel-trace --stats -- python tools/change_report_time.py _step` for k_change_report's
         own time and the copy's (the runtime runs the device-to-device copy as the kernel `__amd_rocclr_copyBuffer`, so it is in the
         kernel trace; a memory-copy trace does not list it); bytes / time is then the achieved rate to put next to the streaming rate of the machine.
  cli    writes the same reads as two FASTQ files once (tools/recount_time.py's writer), then runs `rcorrector -p a b -k 23`
         (no -c: one pass, the reads counted and corrected in HBM) --reps times each without and with `-report`: whole-process
         times and their medians.  --binary PATH --plain-only times another build (the parent commit's) the same way.

Every GPU step (the step loop, each `rcorrector` run) is a child process under its own `timeout`; the chain stops at the first
one that fails.

    python tools/change_report_time.py [step|cli] [--reads 25000000] [--reps 5] [--dir DIR] [--binary PATH] [--plain-only] [--limit SECONDS]
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import recount_time  # noqa: E402  (the headline shape P, the FASTQ writer, the guarded child step)

P = recount_time.P


def step_loop(a):
    """child process: rc_correct_device over the headline shard, report off / armed"""
    import torch
    import rcorrector_amd
    import synth_int
    dev = torch.device("cuda:0")
    gen = synth_int.Synth(P["seed"], P["len"], 30000, 1500, P["alpha"], P["err"], True, device=dev)
    seq, qual = gen.generate(0, a.reads // 2)   # first mates, then second mates, len + 1 bytes a read
    L, n = P["len"], (a.reads // 2) * 2
    nbytes = seq.numel()
    off = torch.arange(0, n + 1, dtype=torch.int64, device=dev).mul_(L + 1).to(torch.int32)
    torch.cuda.synchronize()
    ctx = rcorrector_amd.Context(k=P["k"])
    ctx.count_begin()
    ctx.count_add_device(seq, nbytes)
    ctx.count_finish(2)
    ctx.set_run_params(ctx.estimate_error_rate(), b"5")
    work = torch.empty_like(seq)
    res = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4)]
    times = {False: [], True: []}
    changes = 0
    for r in range(2 * (a.reps + 1)):   # (the first of each kind: warm-up)
        armed = bool(r % 2)
        work.copy_(seq)
        torch.cuda.synchronize()
        if armed:
            ctx.change_report_begin()
        t0 = time.perf_counter()
        ctx.correct_device(1, n, nbytes, L, work, qual, off, *res)
        ctx.sync()
        dt = time.perf_counter() - t0
        if armed:
            rep = ctx.change_report()
            changes = int(rep["changes"].sum())
            assert changes == int((work != seq).sum().item()) and int(rep["reads"].sum()) == n
            ctx.change_report_end()
        print("step %d report %s: %.2f ms" % (r, "armed" if armed else "off", 1e3 * dt), flush=True)
        if r >= 2:
            times[armed].append(dt)
    b, c = statistics.median(times[False]), statistics.median(times[True])
    kernel_bytes = 2 * nbytes + 4 * (n + 1) + 4 * n + changes
    print("correct_device %d x %d bp, k %d: report off %.2f ms, armed %.2f ms (medians of %d): +%.2f ms (%+.1f %%); %d changed bases in %d reads of %d bytes; "
          "k_change_report reads %d bytes (two arenas, offsets, ret, a quality byte per change), the snapshot copy moves %d (read + write)"
          % (n, L, P["k"], 1e3 * b, 1e3 * c, a.reps, 1e3 * (c - b), 100.0 * (c - b) / b, changes, n, nbytes, kernel_bytes, 2 * nbytes), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="step", choices=["step", "cli", "_step"])
    ap.add_argument("--reads", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "recount_time"))
    ap.add_argument("--binary", default=os.path.join(ROOT, "rcorrector_amd", "rcorrector"))
    ap.add_argument("--plain-only", action="store_true", help="only runs without -report (a build that does not know the flag)")
    ap.add_argument("--limit", type=int, default=240, help="seconds a GPU step may take")
    a = ap.parse_args()
    if a.what == "_step":
        return step_loop(a)
    me = [sys.executable, os.path.abspath(__file__)]
    common = ["--reads", str(a.reads), "--reps", str(a.reps), "--dir", a.dir]
    if a.what == "step":
        _, p = recount_time.step(me + ["_step"] + common, a.limit)
        sys.stdout.write(p.stdout.decode())
        return
    os.makedirs(a.dir, exist_ok=True)
    f1, f2 = os.path.join(a.dir, "r_1.fq"), os.path.join(a.dir, "r_2.fq")
    if not (os.path.exists(f1) and os.path.exists(f2)):
        recount_time.step([sys.executable, os.path.join(HERE, "recount_time.py"), "_write", "--reads", str(a.reads), "--dir", a.dir], a.limit)
    env = dict(os.environ, RC_QUIET="1")
    times = {False: [], True: []}
    for r in range(2 * (a.reps + 1)):   # (the first of each: warm-up -- the page cache, the code objects)
        flag = bool(r % 2)
        if flag and a.plain_only:
            continue
        cmd = [a.binary, "-p", f1, f2, "-k", str(P["k"]), "-od", a.dir] + (["-report", os.path.join(a.dir, "report.tsv")] if flag else [])
        dt, _ = recount_time.step(cmd, a.limit, env)
        print("run %d %s: %.3f s whole process" % (r, "-report" if flag else "plain", dt), flush=True)
        if r >= 2:
            times[flag].append(dt)
    b = statistics.median(times[False])
    if a.plain_only:
        print("%s: median without the flag %.3f s %s" % (a.binary, b, ["%.3f" % x for x in times[False]]), flush=True)
        return
    c = statistics.median(times[True])
    print("%s: median without the flag %.3f s %s, with -report %.3f s %s: overhead %.3f s (%+.1f %%)"
          % (os.path.basename(a.binary), b, ["%.3f" % x for x in times[False]], c, ["%.3f" % x for x in times[True]], c - b, 100.0 * (c - b) / b), flush=True)
    for line in open(os.path.join(a.dir, "report.tsv")).read().splitlines()[:4]:
        print("report.tsv:", line)


if __name__ == "__main__":
    main()
