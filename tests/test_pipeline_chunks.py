"""The chunked pipeline of rc_correct_device (rc_api_batch.hip: rc_correct_pipelined): the fused probe + threshold kernel
launched chunk by chunk over the locality list on the context's stream, each chunk's compactions, k_single and k_correct on
a follower stream behind it.  RC_PIPELINE_CHUNKS=<C> (read when a context is made) forces C chunks at any batch size.

CPU: tests/hostmath/timer_pool.cpp, the kernel timers' deferred event pairs (rc_timer_pool.h) against a stub back end --
pool full, resolved twice, reset while pairs are pending -- built plain and with -fsanitize=address,undefined.

GPU: tiny batches with RC_LOCALITY=force.  Every case compares ret / l / m / h and the corrected bases with the oracle AND
with a context of the same kind at RC_PIPELINE_CHUNKS=0, and rc_debug_routes (cls, cand, and the runs of the candidates)
with that context's: results and routing are functions of a read's unit alone, whatever the chunks.  The reads' order in the
locality list is the min-hash order, which no test controls; the cases that need an idle chunk get it by construction: a
batch whose reads are error-free but for one pair, run with one tile per chunk, so that every chunk but one has empty
k_single / k_correct lists -- the first and the last ones too unless that pair sorts there, and two batches with different
pairs are run.

That the pipeline ran at all is asserted through rc_debug_pipeline (batches run as a pipeline, non-empty chunks launched): a
comparison of "C chunks" with "no chunks" holds trivially where the batch did not qualify and ran whole."""
import functools
import os
import subprocess

import numpy as np
import pytest

import datasets
import synth
import test_stage_wide as tsw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostmath", "timer_pool.cpp")
WHAT = ["ret", "l", "m", "h", "bases"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_timer_pool_against_a_stub(tmp_path, flags):
    exe = str(tmp_path / "timer_pool")
    subprocess.run(["g++", "-std=c++17"] + flags + ["-I", os.path.join(ROOT, "rcorrector_amd", "csrc"), SRC, "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("ok "), out


# ---- GPU -----------------------------------------------------------------------------------------------------------

def _clean_but_one(seed, which):
    """1 000 error-free 150-base pairs and one substitution in each mate of pair `which`; the table counts the error-free reads"""
    s1, q1, s2, q2, _ = synth.make_reads(seed, 1000, 150, e=0.0, paired=True, n_tx=30)
    keys, cnt = synth.count_kmers([s1, s2], 23)
    keys, cnt = tsw._pad_table(keys, cnt, 23, 30_000, seed + 1) if len(keys) < 30_000 else (keys, cnt)
    for s, p in ((s1, 70), (s2, 81)):
        s[which, p] = synth.NUC[(synth.CODE[s[which, p]] + 1) & 3]
    full = np.full(1000, 150)
    return dict(k=23, mfk=4, rate=0.01, mode=1, keys=keys, counts=cnt, seqs1=tsw._rows(s1, full), quals1=tsw._rows(q1, full),
                seqs2=tsw._rows(s2, full), quals2=tsw._rows(q2, full))


def _batch(name):
    if name in ("pe150", "k31", "two"):
        return tsw._case(name)[0]
    pe = tsw._case("pe150")[0]
    if name == "se150":    # the same reads, every read on its own
        return dict(pe, mode=0, seqs1=pe["seqs1"] + pe["seqs2"], quals1=pe["quals1"] + pe["quals2"], seqs2=None, quals2=None)
    if name == "il150":    # the same pairs, interleaved in one arena
        il = lambda a, b: [x for ab in zip(a, b) for x in ab]
        return dict(pe, mode=2, seqs1=il(pe["seqs1"], pe["seqs2"]), quals1=il(pe["quals1"], pe["quals2"]), seqs2=None, quals2=None)
    if name == "few":      # 20 pairs: 40 reads, three tiles
        return dict(pe, seqs1=pe["seqs1"][:20], quals1=pe["quals1"][:20], seqs2=pe["seqs2"][:20], quals2=pe["quals2"][:20])
    if name == "long":     # one read of 200 bases among them: the batch is tiered, the pipeline must stand aside
        s1, q1, _, _, _ = synth.make_reads(53001, 1, 200, e=0.01, n_tx=1)
        return dict(pe, mode=0, seqs1=pe["seqs1"] + [s1[0].tobytes()], quals1=pe["quals1"] + [q1[0].tobytes()], seqs2=None, quals2=None)
    if name == "clean_a":
        return _clean_but_one(53011, 123)
    if name == "clean_b":
        return _clean_but_one(53021, 777)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(batch, the oracle's results on it): computed once, left unchanged; the batches of test_stage_wide are shared with it"""
    if name in ("pe150", "k31", "two"):
        return tsw._case(name)
    from oracle import pyoracle
    pyoracle.build()
    pyoracle.lib()
    d = _batch(name)
    want = datasets.run_oracle(pyoracle, d)
    for a in want:
        a.setflags(write=False)
    return d, want


def _context(monkeypatch, d, env, chunks):
    import rcorrector_amd
    for key in ("RC_NO_SINGLE", "RC_K3_LOCAL", "RC_PIPELINE_GRID_DIV"):
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv("RC_LOCALITY", "force")          # (all of them are read when the context is made)
    monkeypatch.setenv("RC_PIPELINE_CHUNKS", str(chunks))
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    ctx.table_build(d["keys"], d["counts"])
    ctx.set_run_params(d["rate"], b"H")
    return ctx


def _launch(ctx, d, arrays):
    import torch
    dev, n, max_len, seq, qual, off = arrays
    work = seq.clone()
    res = [torch.full((n,), -77, dtype=torch.int32, device=dev) for _ in range(4)]
    ctx.correct_device(d["mode"], n, int(seq.numel()), max_len, work, qual, off, *res)
    return res, work


def _fetch(res, work):
    return [r.cpu().numpy() for r in res] + [work.cpu().numpy()]


def _equal(want, got, label):
    for w, g, what in zip(want, got, WHAT):
        bad = np.nonzero(w != g)[0]
        assert len(bad) == 0, "%s: %s differs at %s: want %s got %s" % (label, what, bad[:5], w[bad[:5]], g[bad[:5]])


def reads_per_tile(max_len, wave_tiles=False):
    """rc_fused_tiles (rc_correct.hip) restated: a read takes its bases, the NUL and up to 6 bytes of alignment, max_len + 8 bytes
    of a tile of 2 816 bytes (8 of them not the reads'), at most RC_PLIST_MAX_READS = 64 reads, in whole passes of 16 rows; the
    4 096-byte tile where it holds 32 reads and the small one does not.  150 bases: 2808 // 158 = 17 -> 16 reads a tile; 100
    bases: 2808 // 108 = 26 -> 16, but 4088 // 108 = 37 -> 32, so the 4 096-byte instance with 32.  wave_tiles: the instance of
    RC_FUSED_WAVE_TILES=1 (4 reads), taken for reads of at most 128 k-mers over a table without extension bits -- the caller's to know."""
    fit = lambda tile: min((tile - 8) // (max_len + 8), 64) & ~15
    assert max_len <= 160, "the fused kernel holds reads of up to 160 bases"
    if wave_tiles:
        return 4
    return fit(4096) if fit(2816) < 32 <= fit(4096) else fit(2816)


def chunks_expected(n, rpt, chunks):
    """the non-empty chunks of n reads in tiles of rpt, cut at tile_at(c) = n_tiles * c // chunks (rc_correct_pipelined): every
    chunk where there are at least as many tiles, else one per tile"""
    return min(chunks, (n + rpt - 1) // rpt)


def _routes(ctx, n, tiered):
    if tiered:   # (rc_debug_routes describes whole batches only)
        return None
    cls, cand, runs = ctx.debug_routes(n)
    return cls, cand, np.where(cand != 0, runs, 0)   # (runs: the candidates' only)


def _check(monkeypatch, name, chunks, env=None, profile=False, tiered=False):
    d, want = _case(name)
    want = list(want[:4]) + [np.concatenate(want[4:])]
    arrays = tsw._device_arrays(d)
    n = arrays[1]
    out = {}
    for c in (0, chunks):
        ctx = _context(monkeypatch, d, env or {}, c)
        if profile:
            ctx.profile(True)
            ctx.profile_reset()
        res, work = _launch(ctx, d, arrays)
        ctx.sync()
        out[c] = (_fetch(res, work), _routes(ctx, n, tiered), [ctx.profile_get(kd) for kd in range(4)] if profile else None)
        # the pipeline ran for the chunked context and for no other: one batch, every non-empty chunk launched once
        ran = (0, 0) if c == 0 or tiered else (1, chunks_expected(n, reads_per_tile(arrays[2]), c))
        assert ctx.debug_pipeline() == ran, "%s, RC_PIPELINE_CHUNKS=%d: (batches, chunks) run as a pipeline are %r, expected %r" % (name, c, ctx.debug_pipeline(), ran)
        ctx.close()
    _equal(want, out[chunks][0], "%s, %d chunks, against the oracle" % (name, chunks))
    _equal(out[0][0], out[chunks][0], "%s, %d chunks, against no chunks" % (name, chunks))
    if not tiered:
        for a, b, what in zip(out[0][1], out[chunks][1], ["cls", "cand", "runs"]):
            assert np.array_equal(a, b), "%s, %d chunks: the routes' %s differ from those without chunks" % (name, chunks, what)
    return d, want, out


@pytest.mark.gpu
@pytest.mark.parametrize("name,chunks", [("pe150", 2), ("pe150", 3), ("pe150", 7), ("se150", 3), ("il150", 3), ("few", 7), ("k31", 3), ("two", 2)])
def test_chunked_pipeline_equals_oracle_and_unchunked(oracle, monkeypatch, name, chunks):
    d, want, _ = _check(monkeypatch, name, chunks)
    n = len(want[0])
    assert int((want[0] > 0).sum()) >= 1
    if name in ("pe150", "se150", "il150"):
        assert n == 3000 and n % 16 != 0, "the last tile is to be a partial one"
    if name == "few":
        assert (n + 15) // 16 < chunks, "some chunks are to be empty"
    if name == "k31":
        assert d["mfk"] == 8


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["clean_a", "clean_b"])
def test_chunks_with_nothing_to_correct(oracle, monkeypatch, name):
    """one tile per chunk, one pair with errors in the whole batch: every chunk but that pair's has empty lists"""
    d, want = _case(name)
    pair = {"clean_a": 123, "clean_b": 777}[name]
    assert np.nonzero(want[0] > 0)[0].tolist() == [pair, 1000 + pair]
    _check(monkeypatch, name, (2000 + 15) // 16)
    _check(monkeypatch, name, 2)


@pytest.mark.gpu
def test_a_tiered_batch_switches_the_pipeline_off(oracle, monkeypatch):
    _check(monkeypatch, "long", 3, tiered=True)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"RC_NO_SINGLE": "1"}, {"RC_K3_LOCAL": "1"}, {"RC_PIPELINE_GRID_DIV": "2"}], ids=["no_single", "k3_local", "half_grids"])
def test_chunked_pipeline_under_the_knobs(oracle, monkeypatch, env):
    _check(monkeypatch, "pe150", 3, env=env)


@pytest.mark.gpu
def test_profiling_counts_one_launch_per_call(oracle, monkeypatch):
    _, _, out = _check(monkeypatch, "pe150", 3, profile=True)
    for c, (_, _, prof) in out.items():
        for kd in (0, 2, 3):
            ms, launches = prof[kd]
            assert launches == 1 and ms > 0, "%d chunks: kernel kind %d reports %r ms in %r launches" % (c, kd, ms, launches)


@pytest.mark.gpu
def test_two_calls_back_to_back_without_a_sync(oracle, monkeypatch):
    """the follower's buffers are reused across the join: the second call's kernels queue behind the first call's follower"""
    d1, want1 = _case("pe150")
    d2, want2 = _case("se150")
    a1, a2 = tsw._device_arrays(d1), tsw._device_arrays(d2)
    ctx = _context(monkeypatch, d1, {}, 3)
    r1 = _launch(ctx, d1, a1)
    r2 = _launch(ctx, d2, a2)
    r3 = _launch(ctx, d1, a1)
    ctx.sync()
    batches, chunks = ctx.debug_pipeline()
    assert batches == 3 and chunks == 9, "three batches of 188, 188 and 188 tiles in three chunks each: %r" % ((batches, chunks),)
    _equal(list(want1[:4]) + [np.concatenate(want1[4:])], _fetch(*r1), "first call")
    _equal(list(want2[:4]) + [np.concatenate(want2[4:])], _fetch(*r2), "second call")
    _equal(list(want1[:4]) + [np.concatenate(want1[4:])], _fetch(*r3), "third call")
    ctx.close()
