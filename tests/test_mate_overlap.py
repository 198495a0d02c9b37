"""GPU: the mate-overlap report (include/rcorrector_amd.h: rc_mate_overlap) against the numpy restatement of its definitions in
tests/test_mate_overlap_host.py: the device entry point on pairs built for the edges, two versions that differ, error-free
synthetic pairs, a session on every transport, the argument and state errors, and the command line."""
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import rcorrector_amd
import synth
import test_mate_overlap_host as mho
import test_observers_together as tot
from rcorrector_amd.binding import OVERLAP_WORDS, mate_overlap_dict
from test_recount import packed, unit_cuts
from test_recount_cli import fixture_args
from test_weak_profile_cli import outputs, run

pytestmark = pytest.mark.gpu
RC_STATUS_ARG, RC_STATUS_STATE = -1, -4
_cache = {}


def bare_ctx():
    return rcorrector_amd.Context(k=23, max_fix_per_k=4, device=0)


def layout(pairs, mode, which):
    """the reads of one version (which = 0: before, 2: after) in the order of `mode`"""
    a, b = [p[which] for p in pairs], [p[which + 1] for p in pairs]
    return a + b if mode == 1 else [x for ab in zip(a, b) for x in ab]


def on_device(arena, lead):
    """a copy of `arena` that starts `lead` bytes behind a 16-byte boundary of device memory, letters in front of and behind it"""
    import torch
    a = np.frombuffer(arena, np.uint8)
    buf = torch.full((lead + a.size + 64,), ord("A"), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if a.size:
        buf[lead:lead + a.size] = torch.from_numpy(a.copy()).cuda()
    return buf


def device_counts(ctx, pairs4, mode, lead=0, same=False, min_overlap=30, pct=10, counts=None, max_len=None):
    """rc_mate_overlap_device over the pairs' two versions; returns (the counts as a dict, the device counts)"""
    import torch
    before, off = mho.arena_of(layout(pairs4, mode, 0))
    after, off2 = mho.arena_of(layout(pairs4, mode, 2))
    assert np.array_equal(off, off2)
    t_b, t_a = on_device(before, lead), on_device(after, (lead + 5) % 16)   # (the two arenas need not share an alignment)
    t_off = torch.from_numpy(off.astype(np.int32)).cuda()
    if counts is None:
        counts = torch.zeros(OVERLAP_WORDS, dtype=torch.int64, device="cuda")
    if max_len is None:
        max_len = int(np.diff(off.astype(np.int64)).max()) - 1
    torch.cuda.synchronize()
    p_b = t_b.data_ptr() + lead
    ctx.mate_overlap_device(p_b, p_b if same else t_a.data_ptr() + (lead + 5) % 16, t_off, len(off) - 1, len(before), max_len, mode, counts,
                            min_overlap, pct)
    ctx.sync()
    return mate_overlap_dict(counts.cpu().numpy()), counts


def edge4(max_len):
    """the edge pairs with an edited copy as their corrected version, and the restatement of both ways to call the kernel"""
    if max_len not in _cache:
        rng = np.random.default_rng(11 + max_len)
        pairs4 = mho.corrected(rng, mho.edge_pairs(rng, max_len))
        _cache[max_len] = (pairs4, mho.brute(pairs4), mho.brute([(a, b, a, b) for a, b, _, _ in pairs4]))
    return _cache[max_len]


# ---- 1. / 2. the device entry point against the restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1, 15])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("max_len", [256, 1023], ids=["narrow", "wide"])
def test_device_equals_the_restatement(max_len, mode, lead):
    pairs4, want, want_same = edge4(max_len)
    mho.check_identities(want)
    mho.assert_fixture_has_the_named_changes(want)   # an N -> base and a base -> lower case at faced positions, not left to chance
    ctx = bare_ctx()   # (no table: the report needs none)
    got, _ = device_counts(ctx, pairs4, mode, lead, same=True)
    mho.assert_equal_counts(got, want_same, "d_before == d_after:")
    for b, a in (("compared_before", "compared_after"), ("disagree_before", "disagree_after")):
        assert got[b] == got[a]
    assert got["resolved"] == got["introduced"] == 0 and got["kept"] == got["disagree_before"] and got["pairs_same"] == got["overlapping"]
    assert np.array_equal(got["disagree5_before"], got["disagree5_after"])
    got, _ = device_counts(ctx, pairs4, mode, lead)
    mho.assert_equal_counts(got, want, "two versions:")
    mho.check_identities(got, lost=want["_extra"]["lost"])
    assert got["resolved"] > 0 and got["introduced"] > 0 and got["kept"] > 0 and got["pairs_worsened"] > 0
    assert got["min_overlap"] == 0 and got["max_mismatch_pct"] == 0      # (the device call leaves the two parameters alone)
    ctx.close()


def test_a_second_call_adds_and_no_reads_leave_the_counts_alone():
    pairs4, want, _ = edge4(256)
    ctx = bare_ctx()
    _, counts = device_counts(ctx, pairs4, 1)
    got, counts = device_counts(ctx, pairs4, 2, lead=3, counts=counts)
    for n in mho.SCALARS:
        assert got[n] == 2 * want[n], n
    for n in mho.ARRAYS:
        assert np.array_equal(got[n], 2 * want[n]), n
    ctx.mate_overlap_device(None, None, None, 0, 0, 0, 1, counts)
    ctx.sync()
    again = mate_overlap_dict(counts.cpu().numpy())
    mho.assert_equal_counts(again, got)
    ctx.close()


def test_other_thresholds_and_a_wrong_max_read_len():
    pairs4, _, _ = edge4(256)
    ctx = bare_ctx()
    for mo, pct in ((1, 0), (17, 50), (1023, 10)):
        got, _ = device_counts(ctx, pairs4, 2, min_overlap=mo, pct=pct)
        mho.assert_equal_counts(got, mho.brute(pairs4, mo, pct), "min %d pct %d:" % (mo, pct))
    # the narrow instance over mates of up to 1023 bases: every mate is cut to 256 bases, nothing is indexed outside
    long4, _, _ = edge4(1023)
    got, _ = device_counts(ctx, long4, 1, max_len=100)
    mho.assert_equal_counts(got, mho.brute([tuple(s[:256] for s in four) for four in long4]), "cut to 256:")
    ctx.close()


# ---- 3. error-free synthetic pairs ------------------------------------------------------------------------------------------
def test_error_free_pairs_give_the_generators_fragment_lengths():
    ctx = bare_ctx()
    for length, frag in ((100, 150), (150, 220), (75, 75)):
        s1, _, s2, _, _ = synth.make_reads(31 + frag, 400, length, e=0, paired=True, frag_len=frag)
        pairs4 = [(a.tobytes(), b.tobytes()) * 2 for a, b in zip(s1, s2)]
        got, _ = device_counts(ctx, pairs4, 1, same=True)
        want_frag = np.zeros(2048, np.uint64)
        want_frag[frag] = 400
        assert np.array_equal(got["frag"], want_frag)
        assert got["overlapping"] == got["pairs"] == 400 and got["disagree_before"] == got["disagree_after"] == 0
        assert got["compared_before"] == 400 * (2 * length - frag)
    ctx.close()


# ---- 4. a session on every transport ----------------------------------------------------------------------------------------
def session_data():
    if "session" not in _cache:
        s1, q1, s2, q2, _ = synth.make_reads(7301, 300, 100, n_tx=6, l_tx=400, e=0.01, paired=True, frag_len=150)
        rows = lambda x: [r.tobytes() for r in x]   # noqa: E731
        _cache["session"] = dict(k=23, mfk=4, mode=1, bad_q=b"H", seqs1=rows(s1), quals1=rows(q1), seqs2=rows(s2), quals2=rows(q2))
    return _cache["session"]


def session_ctx(d, resident):
    """a table counted from the data set's own reads (count >= 2); resident: its two arenas stay in HBM"""
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    a1, off1 = rcorrector_amd.pack_reads(d["seqs1"])
    a2, off2 = rcorrector_amd.pack_reads(d["seqs2"])
    ctx.count_keep(resident)
    ctx.count_begin()
    ctx.count_add(a1)
    ctx.count_add(a2)
    ctx.count_finish(2)
    ctx.set_run_params(0.01, d["bad_q"])
    return ctx, (off1, off2)


def run_session(transport, armed, single_end_too=False):
    """three batches in slots 0, 1, 2 (or one after the other); returns the batches' outputs and what the armed observers saw"""
    d = session_data()
    ctx, kept = session_ctx(d, transport == "resident")
    ctx.set_slot_lanes(True)
    if "overlap" in armed:
        ctx.mate_overlap_begin()
    if "report" in armed:
        ctx.change_report_begin()
    out = {"batches": []}
    cuts = unit_cuts(d, 3)
    if transport == "correct_batch":
        for lo, hi in cuts:
            args = packed(rcorrector_amd, d, lo, hi)[4]
            res = ctx.correct_batch(d["mode"], *args)
            out["batches"].append((np.concatenate(args[0::3]),) + tuple(res))
        if single_end_too:   # a batch that is known to be single-end: skipped silently
            a, off = rcorrector_amd.pack_reads(d["seqs1"][:50])
            qa, _ = rcorrector_amd.pack_reads(d["quals1"][:50])
            ctx.correct_batch(0, a, qa, off)
    else:
        states = {slot: tot.submit(transport, ctx, d, kept, slot, lo, hi) for slot, (lo, hi) in enumerate(cuts)}
        for slot in sorted(states):
            out["batches"].append(tot.finish(transport, ctx, slot, states[slot]))
    if "overlap" in armed:
        out["overlap"] = ctx.mate_overlap()
        ctx.mate_overlap_end()
    if "report" in armed:
        out["report"] = ctx.change_report()
        ctx.change_report_end()
    out["summary"], out["digest"] = ctx.summary(), ctx.table_digest()
    ctx.close()
    return out


def session_want(batches):
    """the restatement over (input bases, corrected bases as returned)"""
    d = session_data()
    key = b"".join(b[0].tobytes() for b in batches)
    if key not in _cache:
        pairs4 = []
        for (lo, hi), b in zip(unit_cuts(d, 3), batches):
            cor = bytes(b[0]).split(b"\0")[:-1]
            n = hi - lo
            assert len(cor) == 2 * n
            pairs4 += [(d["seqs1"][lo + i], d["seqs2"][lo + i], cor[i], cor[n + i]) for i in range(n)]
        _cache[key] = mho.brute(pairs4)
    return _cache[key]


def plain_run(transport):
    if ("plain", transport) not in _cache:
        _cache["plain", transport] = run_session(transport, ())
    return _cache["plain", transport]


@pytest.mark.parametrize("transport", ["correct_batch", "slots_lanes_on", "packed", "resident"])
def test_a_session_counts_every_batch_once_and_changes_nothing(transport):
    got = run_session(transport, ("overlap",), single_end_too=transport == "correct_batch")
    plain = run_session(transport, (), single_end_too=transport == "correct_batch") if transport == "correct_batch" else plain_run(transport)
    tot.assert_same(got["batches"], plain["batches"], "corrected reads and ret / l / m / h")
    assert got["summary"] == plain["summary"] and got["digest"] == plain["digest"]
    want = session_want(got["batches"])
    mho.assert_equal_counts(got["overlap"], want, transport)
    mho.check_identities(got["overlap"], lost=want["_extra"]["lost"])
    assert want["_extra"]["lost"] == 0               # (a correction writes one of ACGT: no valid base becomes invalid)
    o = got["overlap"]
    assert o["pairs"] == 300 and o["overlapping"] > 290 and o["resolved"] > 50 and o["disagree_after"] < o["disagree_before"]
    assert o["min_overlap"] == 30 and o["max_mismatch_pct"] == 10 and int(o["frag"][150]) > 290


def test_a_session_beside_the_change_report_takes_one_snapshot_and_changes_neither():
    both = run_session("packed", ("overlap", "report"))
    report_alone = run_session("packed", ("report",))
    tot.assert_same(both["report"], report_alone["report"], "the change report")
    tot.assert_same(both["batches"], plain_run("packed")["batches"], "corrected reads and ret / l / m / h")
    mho.assert_equal_counts(both["overlap"], session_want(both["batches"]), "beside the report")
    assert int(both["report"]["changes"].sum()) > 0


# ---- 5. argument and state errors ------------------------------------------------------------------------------------------
def test_argument_and_state_errors():
    import torch
    L = rcorrector_amd.load_library()
    ctx = bare_ctx()
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    off = torch.zeros(8, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(OVERLAP_WORDS, dtype=torch.int64, device="cuda")
    p, o, c = buf.data_ptr(), off.data_ptr(), cnt.data_ptr()

    def dev(before=p, after=p, d_off=o, n=2, nbytes=4, max_len=1, mode=1, mo=30, pct=10, counts=c):
        return L.rc_mate_overlap_device(ctx._h, before, after, d_off, n, nbytes, max_len, mode, mo, pct, counts)
    assert dev() == 0
    for kw in (dict(mode=0), dict(mode=3), dict(mode=-1), dict(n=3), dict(mo=0), dict(mo=1024), dict(pct=-1), dict(pct=51), dict(nbytes=1 << 32),
               dict(before=None), dict(after=None), dict(d_off=None), dict(counts=None)):
        assert dev(**kw) == RC_STATUS_ARG, kw
        assert b"mate_overlap_device" in L.rc_last_error(ctx._h)
    assert dev(n=0, before=None, after=None, d_off=None, counts=None) == 0
    ctx.sync()
    assert int(cnt.sum()) == 1     # (the one pair of two empty reads: pairs = 1, nothing else)
    for mo, pct in ((0, 10), (1024, 10), (30, -1), (30, 51)):
        assert L.rc_mate_overlap_begin(ctx._h, mo, pct) == RC_STATUS_ARG
    assert L.rc_mate_overlap_get(ctx._h, None) == RC_STATUS_STATE and L.rc_mate_overlap_end(ctx._h) == RC_STATUS_STATE
    with pytest.raises(rcorrector_amd.RcorrectorError):
        ctx.mate_overlap()
    ctx.mate_overlap_begin(25, 5)
    assert L.rc_mate_overlap_begin(ctx._h, 30, 10) == RC_STATUS_STATE and L.rc_mate_overlap_get(ctx._h, None) == RC_STATUS_ARG
    got = ctx.mate_overlap()
    assert got["min_overlap"] == 25 and got["max_mismatch_pct"] == 5 and got["pairs"] == 0 and not got["frag"].any()
    ctx.mate_overlap_end()
    ctx.mate_overlap_begin()          # (a second session after the first has ended)
    ctx.mate_overlap_end()
    ctx.close()


# ---- 6. the command line ---------------------------------------------------------------------------------------------------
def parse_report(text):
    c = {"frag": np.zeros(2048, np.uint64)}
    for n in mho.ARRAYS[1:]:
        c[n] = np.zeros((2, 1024), np.uint64)
    for ln in text.decode().splitlines():
        t = ln.split("\t")
        if t[0] == "frag":
            c["frag"][int(t[1])] = int(t[2])
        elif t[0] == "pos5":
            for n, v in zip(mho.ARRAYS[1:], t[3:]):
                c[n][int(t[1]) - 1, int(t[2])] = int(v)
        elif len(t) == 3:
            c["%s_%s" % (t[0], t[1])] = int(t[2])
        else:
            c[t[0]] = int(t[1])
    return c


@pytest.mark.parametrize("name", ["fx_pe_k23", "fx_il_k23"])
def test_overlap_file_and_nothing_else(name, tmp_path):
    out = str(tmp_path / "overlap.tsv")
    args = fixture_args(name)
    p = run(name, tmp_path / "with", args, ["-batch", "100", "-overlap", out])
    p0 = run(name, tmp_path / "without", args, ["-batch", "100"])
    text = open(out, "rb").read()
    c = parse_report(text)
    assert text.startswith(b"min_overlap\t30\nmax_mismatch_pct\t10\npairs\t") and c["min_overlap"] == 30 and c["max_mismatch_pct"] == 10
    mho.check_identities(c, lost=0)                  # (a correction writes one of ACGT: no valid base becomes invalid)
    n_reads = sum(open(os.path.join(gu.GOLDEN, name, a), "rb").read().count(b"\n") // 4 for a in args if a.endswith(".fq"))
    assert c["pairs"] == n_reads // 2 > 0
    assert p.stdout == p0.stdout and p.stderr.startswith(p0.stderr) and p.stderr[len(p0.stderr):].startswith(b"Mate overlap (at least 30 bases")
    assert p.stderr[len(p0.stderr):].count(b"\n") == 1
    got, plain = outputs(tmp_path / "with"), outputs(tmp_path / "without")
    assert got == plain and len(got) > 0
    for f in got:
        assert got[f] == open(os.path.join(gu.GOLDEN, name, "ref", f), "rb").read(), f
    if name == "fx_pe_k23":
        two = str(tmp_path / "two.tsv")
        run(name, tmp_path / "two", args, ["-gpus", "2", "-batch", "64", "-inflight", "2", "-overlap", two], {"RC_SHARED_GPU": "1"})
        assert open(two, "rb").read() == text
        small = str(tmp_path / "small.tsv")
        run(name, tmp_path / "small", args, ["-packed", "-batch", "60", "-overlap", small, "-overlap-min", "20", "-overlap-mm", "5"])
        assert open(small, "rb").read().startswith(b"min_overlap\t20\nmax_mismatch_pct\t5\npairs\t%d\n" % c["pairs"])


def test_overlap_with_single_end_input_or_verbose_is_refused(tmp_path):
    out = str(tmp_path / "o.tsv")
    p = run("fx_pe_k23", tmp_path / "v", fixture_args("fx_pe_k23"), ["-overlap", out, "-verbose"], ok=False)
    assert p.returncode != 0 and b"-overlap cannot be combined with -verbose" in p.stderr
    p = run("fx_se_k23", tmp_path / "r", fixture_args("fx_se_k23"), ["-overlap", out], ok=False)
    assert p.returncode != 0 and b"-overlap compares the two mates of a pair" in p.stderr
    p = run("fx_pe_k23", tmp_path / "m", fixture_args("fx_pe_k23"), ["-overlap", out, "-overlap-min", "0"], ok=False)
    assert p.returncode != 0 and b"-overlap-min must be 1..1023" in p.stderr
    assert not os.path.exists(out)
    p = subprocess.run([os.path.join(gu.ROOT, "rcorrector_amd", "rcorrector"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.stderr.index(b"\t-trust-by-pos STRING:") < p.stderr.index(b"\t-overlap STRING:") < p.stderr.index(b"\t-verbose-iter INT:")
