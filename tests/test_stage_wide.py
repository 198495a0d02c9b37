"""How k_single brings a read into LDS: sixteen bases per lane through rc_stage16 / rc_pack16m (rc_common.h) and the
counts as int4, instead of a byte per lane per pass.  (k_correct keeps its byte-wise rc_load_read: the same staging there
was measured and gained nothing -- profiles/stage_wide_ab.txt; the batches below still hold it to the oracle.)

CPU: tests/hostmath/stage_wide.cpp, the helper against a byte-at-a-time restatement with rc_base_code on a heap arena of
exactly nbytes bytes -- every o mod 16, every len 0..160, every nbytes mod 4, the read at the very end of the arena --
built plain and with -fsanitize=address,undefined (a load outside the arena stops the program).

GPU: ret / l / m / h and the corrected bases of rc_correct_device against the oracle on batches whose reads start at every
offset modulo 16 (ragged lengths 23..160, single-end and paired), with N's and lowercase letters, 150-base pairs at k = 23,
k = 31 with -maxcorK 8 over a PACKED table with extension bits (the EXT instances), an arena whose length is no multiple
of 4 with the last read at its end, and batches of 1 and 2 reads.  Every batch must give both kernels work: k_single's
timer runs and the instrumented k_correct is handed reads (each batch is corrected twice: by the kernels a plain run uses
and by the instrumented k_correct instance; both must equal the oracle)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import datasets
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostmath", "stage_wide.cpp")
WHAT = ["ret", "l", "m", "h", "bases"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_stage16_equals_a_byte_at_a_time_restatement(tmp_path, flags):
    exe = str(tmp_path / "stage_wide")
    subprocess.run(["g++", "-std=c++17"] + flags + ["-I", os.path.join(ROOT, "rcorrector_amd", "csrc"), SRC, "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("ok "), out


# ---- GPU -----------------------------------------------------------------------------------------------------------

def _rows(a, lens):
    return [a[i, :int(lens[i])].tobytes() for i in range(len(a))]


def _spoil(reads, seed):
    """a few N's and lowercase letters: one read in 25 gets one to three of them"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for r in reads:
        if rng.random() < 0.04:
            b = bytearray(r)
            for p in rng.choice(len(b), int(rng.integers(1, 4)), replace=False):
                b[p] = ord("N") if rng.random() < 0.5 else ord(chr(b[p]).lower())
            r = bytes(b)
        out.append(r)
    return out


def _pad_table(keys, cnt, k, pad_to, seed):
    """k-mers no read holds, so that the table has the size -- and so the layout -- of a real one (datasets.k_sweep)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    mask = np.uint64((1 << (2 * k)) - 1)
    m = pad_to + pad_to // 8
    fwd = (rng.integers(0, 1 << 63, size=m, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=m, dtype=np.uint64)) & mask
    pad = np.unique(np.minimum(fwd, datasets.revcomp_codes(fwd, k)))
    pad = rng.permutation(pad[~np.isin(pad, keys)])[:pad_to - len(keys)]
    return np.concatenate([keys, pad]), np.concatenate([cnt, rng.integers(2, 200, size=len(pad)).astype(np.int64)])


def _batch(name):
    """dict(k, mfk, rate, mode, keys, counts, seqs1, quals1, seqs2, quals2) of the named batch"""
    if name in ("ragged_se", "ragged_pe", "ragged_se_nl", "ragged_pe_nl"):
        paired = "_pe" in name
        n = 1500 if paired else 3000
        s1, q1, s2, q2, _ = synth.make_reads(52001 + paired, n, 160, e=0.015, paired=paired, n_tx=40)
        rng = np.random.Generator(np.random.PCG64(52011 + paired))
        l1, l2 = rng.integers(23, 161, n), rng.integers(23, 161, n)   # 151-byte strides never occur: every offset mod 16 does
        keys, cnt = synth.count_kmers([s1, s2], 23, [l1, l2])
        r1, qq1 = _rows(s1, l1), _rows(q1, l1)
        r2, qq2 = (_rows(s2, l2), _rows(q2, l2)) if paired else (None, None)
        if name.endswith("_nl"):
            r1 = _spoil(r1, 52021)
            r2 = _spoil(r2, 52022) if paired else None
        return dict(k=23, mfk=4, rate=0.01, mode=1 if paired else 0, keys=keys, counts=cnt, seqs1=r1, quals1=qq1, seqs2=r2, quals2=qq2)
    if name == "pe150":
        s1, q1, s2, q2, _ = synth.make_reads(52031, 1500, 150, e=0.01, paired=True, n_tx=40)
        keys, cnt = synth.count_kmers([s1, s2], 23)
        keys, cnt = _pad_table(keys, cnt, 23, 30_000, 52032) if len(keys) < 30_000 else (keys, cnt)   # (PACKED, ext 0: the k = 23 instance)
        full = np.full(1500, 150)
        return dict(k=23, mfk=4, rate=0.01, mode=1, keys=keys, counts=cnt, seqs1=_rows(s1, full), quals1=_rows(q1, full),
                    seqs2=_rows(s2, full), quals2=_rows(q2, full))
    if name == "k31":
        s1, q1, _, _, _ = synth.make_reads(52041, 2000, 150, e=0.02, n_tx=40)
        keys, cnt = synth.count_kmers([s1], 31)
        keys, cnt = _pad_table(keys, cnt, 31, 6_800_000, 52042)   # >= 2^22 home buckets: PACKED with 8 extension bits
        full = np.full(2000, 150)
        return dict(k=31, mfk=8, rate=0.01, mode=0, keys=keys, counts=cnt, seqs1=_rows(s1, full), quals1=_rows(q1, full), seqs2=None, quals2=None)
    if name in ("odd_arena", "one", "two"):
        s1, q1, _, _, _ = synth.make_reads(52051, 2000, 150, e=0.015, n_tx=40)
        keys, cnt = synth.count_kmers([s1], 23)
        lens = np.full(2000, 150)
        lens[-1] = 149          # 1999 x 151 + 150 bytes: 3 mod 4, the last read's NUL on the arena's last byte
        r, q = _rows(s1, lens), _rows(q1, lens)
        if name != "odd_arena":   # the first reads that both kernels would work on: chosen with the oracle below
            return dict(k=23, mfk=4, rate=0.01, mode=0, keys=keys, counts=cnt, seqs1=r, quals1=q, seqs2=None, quals2=None, pick=1 if name == "one" else 2)
        return dict(k=23, mfk=4, rate=0.01, mode=0, keys=keys, counts=cnt, seqs1=r, quals1=q, seqs2=None, quals2=None)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(batch, the oracle's results on it): computed once, left unchanged"""
    from oracle import pyoracle
    pyoracle.build()
    pyoracle.lib()
    d = _batch(name)
    if "pick" in d:
        # batches of 1 and 2 reads: reads with one substitution in the middle (k_single's kind) cannot give k_correct work
        # too, so the first read is one the oracle corrects in several places (k_correct's) and the second one it
        # corrects in exactly one (k_single's candidate); a batch of one is the first of them
        full = datasets.run_oracle(pyoracle, d)
        many = int(np.nonzero(full[0] >= 2)[0][0])
        single = int(np.nonzero(full[0] == 1)[0][0])
        idx = [many, single][:d["pick"]]
        d = dict(d, seqs1=[d["seqs1"][i] for i in idx], quals1=[d["quals1"][i] for i in idx])
    want = datasets.run_oracle(pyoracle, d)
    for a in want:
        a.setflags(write=False)
    return d, want


def _device_arrays(d):
    import torch
    from oracle import pyoracle as po
    dev = torch.device("cuda", 0)
    a, off = po.pack_reads(d["seqs1"])
    qa, _ = po.pack_reads(d["quals1"])
    if d["mode"] == 1:   # reads [0, n/2) are the mates of [n/2, n): the second arena behind the first
        a2, off2 = po.pack_reads(d["seqs2"])
        qa2, _ = po.pack_reads(d["quals2"])
        off = np.concatenate([off[:-1], off2 + off[-1]])
        a, qa = np.concatenate([a, a2]), np.concatenate([qa, qa2])
    n = len(off) - 1
    max_len = int(np.diff(off.astype(np.int64)).max()) - 1
    return dev, n, max_len, torch.from_numpy(a.copy()).to(dev), torch.from_numpy(qa.copy()).to(dev), torch.from_numpy(off.astype(np.int32)).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged_se", "ragged_pe", "ragged_se_nl", "ragged_pe_nl", "pe150", "k31", "odd_arena", "one", "two"])
def test_correct_device_matches_oracle_with_wide_staging(oracle, name):
    import torch
    import rcorrector_amd
    d, want = _case(name)
    want_bases = np.concatenate(want[4:])
    assert int((want[0] > 0).sum()) >= 1
    dev, n, max_len, seq, qual, off = _device_arrays(d)
    nbytes = int(seq.numel())
    assert nbytes == len(want_bases)
    if name == "odd_arena":
        assert nbytes % 4 != 0 and int(off[-1].item()) == nbytes
    if name.startswith("ragged"):
        assert len(set((off.cpu().numpy().astype(np.int64) % 16).tolist())) == 16
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    ctx.table_build(d["keys"], d["counts"])
    ctx.set_run_params(d["rate"], b"H")
    if name == "k31":
        assert ctx.table_layout() == 1 and ctx.table_stats()["buckets"] < 1 << (2 * d["k"] - 32), "not the EXT instances"
    for prof in (1, 2):   # 1: the kernels of a plain run, timed; 2: the instrumented k_correct, which counts the reads it is handed
        work = seq.clone()
        res = [torch.full((n,), -77, dtype=torch.int32, device=dev) for _ in range(4)]
        ctx.profile(prof)
        ctx.profile_reset()
        ctx.correct_device(d["mode"], n, nbytes, max_len, work, qual, off, *res)
        ctx.sync()
        got = [r.cpu().numpy() for r in res] + [work.cpu().numpy()]
        for w, g, what in zip(list(want[:4]) + [want_bases], got, WHAT):
            bad = np.nonzero(w != g)[0]
            assert len(bad) == 0, "%s differs (%s, profile %d) at %s: want %s got %s" % (what, name, prof, bad[:5], w[bad[:5]], g[bad[:5]])
        if prof == 1:
            ms_single, _ = ctx.profile_get(3)
            print("%s: k_single %.4f ms" % (name, ms_single))
            assert ms_single > 0, "k_single did not run"
        else:
            listed, _, _ = ctx.profile_correct_counters()
            print("%s: k_correct was handed %d of %d reads" % (name, listed, n))
            assert listed > 0, "k_correct was handed no read"
    ctx.profile(False)
    ctx.close()
