"""Correction on k-mer counts too large for a PACKED table slot, and on thresholds beyond the table of GetBound's steps.

Two cliffs (tests/datasets.py: huge_make):
  * the mark: a PACKED slot keeps a count in 27 - ext bits, the all-ones value stands for "the count is in the table's prefix"
    (rc_common.h: RC_PACKED_OVF_MAX), and every device probe that meets it has to resolve it (rc_device.h:
    rc_packed_overflow_count) at a call site of its own -- the fused probe + threshold kernel's one-bucket exit and its
    straggler walk, the quad probe, the EXT and non-EXT instances, the filtered lookups of k_correct, k_single, k_kmer_info,
    the per-read entry points, the observers.  A site that forgot would use limit - 1 for every such count;
  * RC_BOUND_STEPS = 65536: a threshold t >= 65536 has no entry in the inverse of GetBound (rc_bs_lookup: "not known"), so
    k_single gives up its condition (4), rc_alt_run takes no nodes on left searches, and the threshold rows evaluate
    GetBound.  Regime A keeps every threshold below it (so that the routes are the model's), regime B (rate 0.01) does not.

The five members x two regimes, on the CPU oracle (entries / overflowing / ext / layout, reads with ret > 0 / < 0, the largest
threshold in regime A / B):
    huge_k23_ext0      30 000 / 1 893 / 0 / PACKED   377 / 0 of   600   22 355 / 21 502 642
    huge_k27_ext8      26 400 / 1 797 / 8 / PACKED   716 / 4 of 1 200    7 651 /     73 038
    huge_k23_small      2 388 / 1 893 / 4 / PACKED   377 / 0 of   600      615 /    486 513
    huge_k31_wide       3 565 / 1 700 / - / WIDE     692 / 7 of 1 200   22 355 / 21 502 642
    huge_k23_fallback  30 000 / 4 277 / 0 / WIDE     377 / 0 of   600   22 355 / 21 502 642
(test_the_huge_sets_are_what_they_are_for pins these conditions without a GPU; tests/test_hostsim.py runs the ten through
the lane-serial build, tests/test_oracle_vs_ref.py two of them through the reference binary.)  Every comparison is exact."""
import functools

import numpy as np
import pytest

import datasets
from seam_arena import canonical

MEMBERS = list(datasets.HUGE)
PACKED_MEMBERS = ["huge_k23_ext0", "huge_k27_ext8", "huge_k23_small"]
WHAT = ["ret", "l", "m", "h", "seq1", "seq2"]
# reads whose largest count stays below the limit (the oracle's h): none at k = 23; one pair mate each at k = 27 and k = 31, a
# read with so many substitutions that every k-mer of it is an error k-mer (h = 2 S): the oracle's numbers, asserted as they are
H_BELOW_LIMIT = {"huge_k27_ext8": 1, "huge_k31_wide": 1}


def _po():
    from oracle import pyoracle
    pyoracle.build()
    pyoracle.lib()
    return pyoracle


def _reads(d):
    return d["seqs1"] + (d["seqs2"] or [])


@functools.lru_cache(maxsize=None)
def _case(name):
    """(data set, the oracle's results, its strong threshold and first weak threshold per read): computed once, shared, unchanged"""
    po = _po()
    d = datasets.make(name)
    want = datasets.run_oracle(po, d)
    T, P = _oracle_table(name)
    strong = np.array([po.strong_threshold(P, T, s) for s in _reads(d)], dtype=np.int64)
    bound = np.array([po.lib().rco_get_bound_int(P, int(s)) if s > 0 else 0 for s in strong], dtype=np.int64)
    for a in want + (strong, bound):
        a.setflags(write=False)
    return d, want, strong, bound


def _oracle_table(name):
    """(table, parameters) for the oracle's per-read functions; made per caller, so that no table outlives the tests"""
    po = _po()
    d = datasets.make(name)
    T = po.Table(d["k"], len(d["keys"]))
    T.put_many(d["keys"], d["counts"])
    return T, po.make_params(d["k"], d["mfk"], d["rate"], b"H")


@functools.lru_cache(maxsize=None)
def _dict_counts(member):
    """({canonical code: count}, the count of every window of every read) of a member, from the dict alone"""
    d = datasets.make(member + "/A")
    counts = dict(zip(np.asarray(d["keys"]).tolist(), np.asarray(d["counts"]).tolist()))
    memo, k = {}, d["k"]
    rows = []
    for s in _reads(d):
        row = np.empty(len(s) - k + 1, dtype=np.int64)
        for i in range(len(row)):
            w = s[i:i + k]
            c = memo.get(w)
            if c is None:
                c = memo[w] = counts.get(canonical(w), 0)
            row[i] = c
        rows.append(row)
    return counts, rows


def _expected_layout(d, env=None):
    """(layout, ext, home buckets) the build's rule gives this table under `env`: datasets.packed_rule at the load in force,
    PACKED while ext <= 8 and at most RC_PACKED_OVF_MAX counts overflow at that ext"""
    env = env or {}
    ext, home = datasets.packed_rule(d["k"], len(d["keys"]), float(env.get("RC_TABLE_LOAD", 0.4)))
    packed = env.get("RC_TABLE_LAYOUT") != "wide" and ext <= 8 and datasets.huge_overflowing(d["counts"], ext) <= datasets.RC_PACKED_OVF_MAX
    return (1, ext, home) if packed else (0, 0, 0)


def _ctx(d, env, monkeypatch):
    """a context made under env (the knobs are read when the context is made, RC_K2_WAVE_PER_READ at every call: env stays set
    for the test), with d's table and parameters; asserts the layout and ext it runs on.  Returns (ctx, layout, ext)."""
    import rcorrector_amd
    for kk, v in env.items():
        monkeypatch.setenv(kk, v)
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    ctx.table_build(d["keys"], d["counts"])
    ctx.set_run_params(d["rate"], b"H")
    layout, ext, home = _expected_layout(d, env)
    st = ctx.table_stats()
    assert st["entries"] == len(d["keys"])
    assert ctx.table_layout() == layout, "%s under %s: layout %d, the build's rule gives %d (ext %d)" % (d["k"], env, ctx.table_layout(), layout, ext)
    if layout == 1:   # home buckets plus the buckets the last chains run on into: this is what pins ext
        assert home < st["buckets"] <= home + 33
    return ctx, layout, ext


def _ids(envs):
    return ["+".join("%s=%s" % kv for kv in e.items()) or "default" for e in envs]


# ---- CPU: the data sets are what they are for ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", datasets.HUGE_NAMES)
def test_the_huge_sets_are_what_they_are_for(name):
    """Conditions on the inputs, checked on the oracle alone (tests/test_quality_datasets.py does the same for the qv_ sets)."""
    d, want, strong, bound = _case(name)
    member = name.split("/")[0]
    layout, ext, _ = _expected_layout(d)
    n_ovf = datasets.huge_overflowing(d["counts"], d["ext"] if d["ext"] <= 8 else 0)
    print("%s: %d entries, %d overflowing, ext %d, layout %d, ret > 0 / < 0 on %d / %d of %d reads, largest threshold %d" % (
        name, len(d["keys"]), n_ovf, d["ext"], layout, int((want[0] > 0).sum()), int((want[0] < 0).sum()), len(want[0]), int(bound.max())))
    assert len(d["keys"]) <= 52_000 and len(d["seqs1"]) in (600, 1200)
    if member == "huge_k23_fallback":
        assert n_ovf > datasets.RC_PACKED_OVF_MAX and layout == 0 and d["ext"] == 0
    elif member == "huge_k31_wide":
        assert d["ext"] > 8 and layout == 0
    else:
        assert 1000 <= n_ovf <= datasets.RC_PACKED_OVF_MAX and layout == 1
        assert (ext, member) in ((0, "huge_k23_ext0"), (8, "huge_k27_ext8"), (4, "huge_k23_small"))
    # the pinned counts are in the table and in the reads
    counts, rows = _dict_counts(member)
    pins = [c for _, c in d["pinned"]]
    assert pins[:3] == [d["limit"] - 2, d["limit"] - 1, d["limit"]] and (pins[3:] == [datasets.INT_MAX]) == (d["ext"] == 0 or d["ext"] > 8)
    seen = np.concatenate(rows)
    for code, c in d["pinned"]:
        assert counts[code] == c and (seen == c).sum() >= 8
    # the error k-mers stay inline, the k-mers seen 8 times or more overflow, the padding is as k_sweep made it
    base, cnt, own = d["base_counts"], np.asarray(d["counts"]), d["own"]
    assert (cnt[:own][base[:own] <= 3] < d["limit"] - 1).all() and int((base[:own] <= 3).sum()) > 100
    at = np.isin(np.asarray(d["keys"][:own]), [c for c, _ in d["pinned"]])
    assert (cnt[:own][(base[:own] >= 8) & ~at] >= d["limit"]).all()
    pads = slice(own + (datasets.HUGE_FALLBACK_PADS if member == "huge_k23_fallback" else 0), None)
    assert np.array_equal(cnt[pads], base[pads]) and (len(cnt) == own or cnt[pads].max() < 200)
    # every read has a count at or beyond the limit, and at least a third of the reads are corrected
    assert int((want[3] < d["limit"]).sum()) == H_BELOW_LIMIT.get(member, 0)
    assert int((want[0] > 0).sum()) >= len(want[0]) // 3
    # the regime: every threshold below RC_BOUND_STEPS, or some beyond it
    if name.endswith("/A"):
        assert bound.max() < datasets.RC_BOUND_STEPS and strong.max() >= d["limit"]
    else:
        assert bound.max() >= datasets.RC_BOUND_STEPS and int((bound >= datasets.RC_BOUND_STEPS).sum()) >= 10


# ---- a. probes -----------------------------------------------------------------------------------------------------------------

PROBE_ENVS = [{}, {"RC_LOCALITY": "force"}, {"RC_LOCALITY": "force", "RC_NO_FUSE": "1"}, {"RC_LOCALITY": "force", "RC_PROBE_QUAD": "1"},
              {"RC_TABLE_LOAD": "0.85"}, {"RC_LOCALITY": "force", "RC_TABLE_LOAD": "0.85"},
              {"RC_TABLE_FILTER": "force", "RC_TABLE_FILTER_KIND": "plain"}, {"RC_TABLE_FILTER": "force", "RC_TABLE_FILTER_KIND": "core"}]


@pytest.mark.gpu
@pytest.mark.parametrize("env", PROBE_ENVS, ids=_ids(PROBE_ENVS))
@pytest.mark.parametrize("member", MEMBERS)
def test_probes_resolve_the_mark(member, env, monkeypatch):
    """rc_probe_device position by position against the dict, rc_strong_threshold_device against the oracle at both rates.
    At load 0.85 the table has fewer home buckets -- one extension bit more at k = 23 (the limit halves, the counts of 4 S
    and more overflow as well), more than eight at k = 27 (WIDE) -- and chains that run on: overflowed k-mers behind a
    continue flag go through the straggler walk."""
    import torch
    d, _, strong_a, _ = _case(member + "/A")
    _, rows = _dict_counts(member)
    ctx, layout, ext = _ctx(d, env, monkeypatch)
    if layout == 1:
        assert datasets.huge_overflowing(d["counts"], ext) >= 1000
    seqs = _reads(d)
    arena, off = _po().pack_reads(seqs)
    d_seq = torch.from_numpy(arena).cuda()
    d_cnt = torch.full((len(arena),), -7, dtype=torch.int32, device="cuda")
    ctx.probe_device(d_seq, len(arena), d_cnt)
    ctx.sync()
    got = d_cnt.cpu().numpy()
    want = np.full(len(arena), -7, dtype=np.int64)
    for o, row in zip(off[:-1].tolist(), rows):
        want[o:o + len(row)] = row
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%s under %s: %d counts differ, first at arena byte %d: got %d, the dict has %d" % (member, env, len(bad), bad[0], got[bad[0]], want[bad[0]])
    d_off = torch.from_numpy(off.astype(np.int32)).cuda()
    for regime in "AB":
        dd, _, strong, _ = _case(member + "/" + regime)
        ctx.set_run_params(dd["rate"], b"H")
        d_strong = torch.full((len(seqs),), -7, dtype=torch.int32, device="cuda")
        ctx.strong_threshold_device(d_seq, d_off, len(seqs), arena.size, 100, d_strong)
        ctx.sync()
        g = d_strong.cpu().numpy()
        bad = np.nonzero(g != strong)[0]
        assert len(bad) == 0, "%s/%s under %s: strong threshold of read %d is %d, the oracle's %d (%d differ)" % (member, regime, env, bad[0], g[bad[0]], strong[bad[0]], len(bad))
    ctx.close()


# ---- b. correction -------------------------------------------------------------------------------------------------------------

def _correct(ctx, d):
    po = _po()
    a, off = po.pack_reads(d["seqs1"])
    qa, _ = po.pack_reads(d["quals1"])
    if d["mode"] == 1:
        a2, off2 = po.pack_reads(d["seqs2"])
        qa2, _ = po.pack_reads(d["quals2"])
        return ctx.correct_batch(1, a, qa, off, a2, qa2, off2) + (a, a2)
    return ctx.correct_batch(d["mode"], a, qa, off) + (a,)


def _assert_results(want, got, tag):
    for w, g, what in zip(want, got, WHAT):
        bad = np.nonzero(w != g)[0]
        assert len(bad) == 0, "%s: %s differs at %s (the oracle's %s, got %s)" % (tag, what, bad[:5], w[bad[:5]], g[bad[:5]])


CORRECT_ENVS = [{}, {"RC_NO_SINGLE": "1"}, {"RC_K3_GENERIC": "1"}, {"RC_NO_ALT": "1"}, {"RC_K2_WAVE_PER_READ": "1"}, {"RC_TABLE_FILTER": "search"},
                {"RC_TABLE_LAYOUT": "wide"}]
# (RC_TABLE_LAYOUT=wide on the two members that are WIDE by themselves would be the default case again)
CORRECT_CASES = [(n, e) for n in datasets.HUGE_NAMES for e in CORRECT_ENVS
                 if not (e.get("RC_TABLE_LAYOUT") == "wide" and n.split("/")[0] in ("huge_k31_wide", "huge_k23_fallback"))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,env", CORRECT_CASES, ids=["%s-%s" % (n, i) for (n, e), i in zip(CORRECT_CASES, _ids([e for _, e in CORRECT_CASES]))])
def test_correct_batch_matches_the_oracle_on_huge_counts(name, env, monkeypatch):
    """correct_batch (ret, l, m, h, bases) on the five members in both regimes, under the knobs that change who probes.
    Regime B is parity only: which kernel finishes a read there is not modelled (tests/k2s_model.py looks GetBound's inverse up
    without a limit, it has no RC_BOUND_STEPS), so a k_single that declined every read beyond the cliff would pass here; that it
    finishes reads below it is test_each_kernel_finishes_reads_with_overflowed_kmers."""
    d, want, _, _ = _case(name)
    ctx, _, _ = _ctx(d, env, monkeypatch)
    _assert_results(want, _correct(ctx, d), "%s under %s" % (name, env))
    reads, cors = ctx.summary()
    assert reads == len(want[0]) and cors == int(want[0][want[0] > 0].sum())
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["standalone", "fused"])
@pytest.mark.parametrize("member", MEMBERS)
def test_each_kernel_finishes_reads_with_overflowed_kmers(member, path, monkeypatch):
    """Regime A, through rc_debug_routes as tests/test_routing.py reads it: the device's route of every read equals the model's
    (T: the threshold kernel, S: k_single, the rest k_correct), with the model's results -- and the model, on the CPU, sends
    reads that hold an overflowed k-mer down each of the three.  The floors are the model's numbers, not the device's."""
    import test_routing as R
    d, want, _, _ = _case(member + "/A")
    exp, want_r = R._expect(d)
    _assert_results(want, want_r, member)
    _, rows = _dict_counts(member)
    marked = np.array([bool((row >= d["limit"] - 1).any()) for row in rows])
    model = np.array([e["route"] for e in exp])
    floors = {r: int(((model == r) & marked).sum()) for r in ("T", "S", "other")}
    print("%s: the model's T / S / other among the reads with an overflowed k-mer: %s" % (member, floors))
    assert min(floors.values()) >= 1, floors
    got = R._run(d, monkeypatch, R.PATHS[path])
    assert got["layout"] == _expected_layout(d)[0]
    routes = np.array(R._check(d, exp, want, got, "%s %s" % (member, path)))
    for r in ("T", "S"):
        assert int(((routes == r) & marked).sum()) == floors[r]
    assert int((np.isin(routes, ["D", "C"]) & marked).sum()) == floors["other"]


# ---- c. transports and entry points --------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["A", "B"])
def test_transports_on_the_table_with_eight_extension_bits(regime, monkeypatch):
    """huge_k27_ext8 through the packed and the resident boundary and rc_correct_device"""
    import torch
    from test_gpu_parity import _packed_inputs, _resident_inputs
    po = _po()
    d, want, _, _ = _case("huge_k27_ext8/" + regime)
    want_arena = np.concatenate(want[4:])
    n_fix = int(want[0][want[0] > 0].sum())
    ctx, layout, ext = _ctx(d, {}, monkeypatch)
    assert (layout, ext) == (1, 8)
    arena, off, bases, exc_pos, exc_chr, qb = _packed_inputs(ctx, po, d)
    before = arena.copy()
    ctx.submit_packed(0, d["mode"], arena.size, off, bases, qb, exc_pos, exc_chr)
    res = ctx.wait_packed(0)
    _assert_results(want[:4], res[:4], "packed boundary")
    ctx.apply_fixes(arena, res[4], res[5])
    assert np.array_equal(arena, want_arena) and len(res[4]) == n_fix
    # rc_correct_device: the pair as an interleaved batch in device memory
    il = [x for p in zip(d["seqs1"], d["seqs2"]) for x in p]
    a, o = po.pack_reads(il)
    qa, _ = po.pack_reads([x for p in zip(d["quals1"], d["quals2"]) for x in p])
    work = torch.from_numpy(a).cuda()
    out = [torch.full((len(il),), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    ctx.correct_device(2, len(il), a.size, 100, work, torch.from_numpy(qa).cuda(), torch.from_numpy(o.astype(np.int32)).cuda(), *out)
    ctx.sync()
    n1 = len(d["seqs1"])
    order = np.arange(2 * n1).reshape(2, n1).T.ravel()   # interleaved read j is read order[j] of the paired batch
    for w, g, what in zip(want[:4], out, WHAT):
        assert np.array_equal(w[order], g.cpu().numpy()), "%s differs through rc_correct_device" % what
    cor = po.unpack_reads(work.cpu().numpy(), o)
    assert cor[0::2] == po.unpack_reads(want[4], po.pack_reads(d["seqs1"])[1]) and cor[1::2] == po.unpack_reads(want[5], po.pack_reads(d["seqs2"])[1])
    ctx.close()
    import rcorrector_amd
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    host, off, qb, args = _resident_inputs(ctx, po, d)
    assert ctx.table_layout() == 1 and ctx.table_stats()["entries"] == len(d["keys"])
    ctx.submit_resident(0, d["mode"], off, qb, **args)
    res = ctx.wait_resident(0)
    _assert_results(want[:4], res[:4], "resident boundary")
    ctx.apply_fixes(host, res[4], res[5])
    assert np.array_equal(host, want_arena) and len(res[4]) == n_fix
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [m + "/" + r for m in PACKED_MEMBERS for r in "AB"])
def test_per_read_entry_points_on_overflowed_counts(name, monkeypatch):
    """the first 100 reads through rc_strong_threshold_read, rc_correct_read and rc_kmer_info_read (k_correct with the front
    end inside, k_kmer_info) against the oracle's per-read functions"""
    from test_per_read import _three_calls
    po = _po()
    d, want, _, _ = _case(name)
    T, P = _oracle_table(name)
    ctx, layout, _ = _ctx(d, {}, monkeypatch)
    assert layout == 1
    rets = [_three_calls(po, ctx, P, T, d["seqs1"][i], d["quals1"][i], "%s read %d" % (name, i)) for i in range(100)]
    ctx.close()
    assert sum(r[0] > 0 for r in rets) >= 30 and min(r[4] for r in rets) >= d["limit"]
    if d["mode"] == 0:   # (a pair's mate is corrected with the pair's threshold in the batch: only single reads must agree with it)
        cor = po.unpack_reads(want[4], po.pack_reads(d["seqs1"])[1])
        for i, r in enumerate(rets):
            assert r == (want[0][i], cor[i], want[1][i], want[2][i], want[3][i]), "%s read %d: per read and as a batch differ" % (name, i)


# ---- d. observers on an overflow table -----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("member", PACKED_MEMBERS)
def test_observers_compare_resolved_counts(member, monkeypatch):
    """weak_profile_device and trust_profile_device with min_count either side of the mark and of a true k-mer's scaled count
    -- a slot's mark compared unresolved would call every overflowed k-mer weak at min_count = limit and beyond -- and
    read_depth_device's quartiles, against the host models of tests/test_weak_profile.py, test_trust_profile.py and
    test_read_depth.py"""
    import test_read_depth as D
    import test_trust_profile as TP
    import test_weak_profile as W
    d, _, _, _ = _case(member + "/A")
    counts, rows = _dict_counts(member)
    ctx, layout, ext = _ctx(d, {}, monkeypatch)
    assert layout == 1 and ext == d["ext"]
    seqs = _reads(d)
    arena, off = _po().pack_reads(seqs)
    true = int(np.median(np.concatenate(rows)))   # a true k-mer's count: most windows of most reads are true k-mers
    assert true > d["limit"] and true % d["scale"] == 0
    memo = {}
    for mc in (d["limit"] - 1, d["limit"], true, true + 1):
        want = W.restate_all(seqs, d["k"], counts, mc)
        assert 0 < int((want[:, 0] > 0).sum())
        W.assert_profile(W.device_profile(ctx, arena, off, mc), want, "%s min_count %d" % (member, mc))
        got = TP.as_counts(TP.device_counts(ctx, arena, off, d["mode"], mc))
        TP.assert_counts(got, TP.restate_reads(seqs, d["mode"], d["k"], counts, mc, memo), "%s min_count %d" % (member, mc))
    assert not np.array_equal(W.restate_all(seqs, d["k"], counts, d["limit"] - 1), W.restate_all(seqs, d["k"], counts, true + 1))
    want = D.restate_all(seqs, d["k"], counts)
    # (the model's own numbers: a median at or beyond the limit on 524 / 1 004 / 524 reads, q1 < median < q3 on 540 / 1 042 / 541)
    assert int((want[:, 2] >= d["limit"]).sum()) >= len(seqs) // 2
    assert int(((want[:, 1] < want[:, 2]) & (want[:, 2] < want[:, 3])).sum()) >= len(seqs) // 2
    D.assert_depth(D.device_depth(ctx, arena, off), want, member)
    ctx.close()


# ---- e. how the table got there ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("member", MEMBERS)
def test_a_loaded_dump_is_the_built_table(member, monkeypatch, tmp_path):
    """load_jfdump of the member's dump: the layout, digest and lookups of table_build"""
    import rcorrector_amd
    import synth
    d, _, _, _ = _case(member + "/A")
    built, layout, _ = _ctx(d, {}, monkeypatch)
    path = str(tmp_path / "dump.jf")
    synth.write_dump(path, d["keys"], d["counts"], d["k"])
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    assert ctx.load_jfdump(path) == len(d["keys"])
    assert ctx.table_layout() == layout and ctx.table_stats() == built.table_stats()
    assert ctx.table_digest() == built.table_digest()
    keys = np.asarray(d["keys"][:d["own"]])
    assert np.array_equal(ctx.lookup(keys), np.asarray(d["counts"][:d["own"]]).astype(np.int32))
    assert np.array_equal(built.lookup(keys), np.asarray(d["counts"][:d["own"]]).astype(np.int32))
    codes, cnt = ctx.table_export()
    order = np.argsort(codes)
    want_order = np.argsort(np.asarray(d["keys"]))
    assert np.array_equal(codes[order], np.asarray(d["keys"])[want_order]) and np.array_equal(cnt[order], np.asarray(d["counts"])[want_order].astype(np.int32))
    ctx.close()
    built.close()


@pytest.mark.gpu
def test_a_counted_table_keeps_a_count_beyond_the_mark():
    """The counter's own way to such a table: k = 25, the k sweep's reads plus as many all-A reads of 1 023 bases (999
    windows each) as it takes the poly-A k-mer past the limit of the table that results.  count_finish keeps the table PACKED,
    lookup returns the exact count, rc_kmer_info_read of an all-A read reports it as h."""
    import rcorrector_amd
    k = 25
    d = datasets.k_sweep(k, 0)
    own, _ = _po().pack_reads(d["seqs1"])
    ext, home = datasets.packed_rule(k, len(d["keys"]) + 1)   # (the sweep's k-mers and the poly-A one)
    assert 0 < ext <= 8
    limit = 1 << (27 - ext)
    n_a = limit // 999 + 2
    polya, _ = _po().pack_reads([b"A" * 1023] * n_a)
    ctx = rcorrector_amd.Context(k=k, device=0)
    ctx.count_begin()
    ctx.count_add(own)
    ctx.count_add(polya)
    n = ctx.count_finish(2)
    st = ctx.table_stats()
    assert n == len(d["keys"]) + 1 == st["entries"]
    assert ctx.table_layout() == 1 and home < st["buckets"] <= home + 33
    assert 999 * n_a >= limit and 999 * (n_a - 2) < limit
    assert ctx.lookup(np.array([0], dtype=np.uint64)).tolist() == [999 * n_a]
    assert np.array_equal(ctx.lookup(np.asarray(d["keys"])), np.asarray(d["counts"]).astype(np.int32))
    ctx.set_run_params(0.01, b"H")
    po = _po()
    T = po.Table(k, n)
    T.put_many(np.concatenate([np.asarray(d["keys"]), np.zeros(1, np.uint64)]), np.concatenate([np.asarray(d["counts"]), [999 * n_a]]))
    info = ctx.kmer_info_read(b"A" * 100)
    assert info == po.kmer_information(po.make_params(k, 4, 0.01, b"H"), T, b"A" * 100) and info[2] == 999 * n_a
    ctx.close()
