"""The batch observers armed together: the correction report, the duplicate census, the trust profile and a recount session
that follows the corrected batches all hang on one hook per batch (rc_api_observe.hip).  The suites test_change_report,
test_duplicates, test_trust_profile_surface and test_recount hold every observer ALONE to its model on every transport; this one
checks only that arming them together on one context changes none of them -- nor the corrected reads and ret / l / m / h.

Input: the first 64 pairs of tests/golden/fx_pe_k23 over the fixture's table, in three batches through slots 0, 1 and 2."""
import os

import numpy as np
import pytest

import golden_util as gu
import rcorrector_amd
from test_duplicates import TRANSPORTS
from test_recount import packed, unit_cuts
from test_weak_profile import fixture, fixture_ctx

pytestmark = pytest.mark.gpu

PAIRS, BATCHES, MAX_BIN, TRUST_MIN = 64, 3, 50, 2
OBSERVERS = ("report", "census", "trust", "recount")
RC_STATUS_ARG, RC_STATUS_NOSPACE = -1, -6


def dataset():
    f = fixture("fx_pe_k23")
    assert f["mode"] == 1 and f["k"] == 23 and len(f["seqs1"]) >= PAIRS
    d = dict(f)
    for name in ("seqs1", "quals1", "seqs2", "quals2"):
        d[name] = f[name][:PAIRS]
    return d


def fixture_dump(d):
    return os.path.join(gu.GOLDEN, d["name"], "dump.jf")


def new_ctx(d, resident):
    """the fixture's table and run parameters; resident: the data set's two arenas counted first and kept in HBM"""
    if not resident:
        return fixture_ctx(d), None
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    a1, off1 = rcorrector_amd.pack_reads(d["seqs1"])
    a2, off2 = rcorrector_amd.pack_reads(d["seqs2"])
    ctx.count_keep(True)
    ctx.count_begin()
    ctx.count_add(a1)
    ctx.count_add(a2)
    ctx.count_finish(2)
    ctx.load_jfdump(fixture_dump(d))
    ctx.set_run_params(ctx.estimate_error_rate(0.95), d["bad_q"])
    return ctx, (off1, off2)


def quality_bits(ctx, qa, bad_q):
    qb = ctx.host_array((qa.size + 7) // 8)
    ctx.pack_quality_bits(qa, bad_q, out=qb)
    return qb


def submit(transport, ctx, d, kept, slot, lo, hi, fix_cap=None):
    """one batch of `transport` into `slot`; returns what finish() needs"""
    a, qa, off, _, args = packed(rcorrector_amd, d, lo, hi)
    if transport in ("slots_lanes_on", "slots_lanes_off"):
        ctx.submit(slot, d["mode"], *args)
        return args, off
    if transport == "packed":
        arena = ctx.host_array(a.size)
        arena[:] = a
        bases, exc_pos, exc_chr = ctx.pack_bases(arena, bases=ctx.host_array((a.size + 15) // 16, np.uint32))
        qb = quality_bits(ctx, qa, d["bad_q"])
        ctx.submit_packed(slot, d["mode"], a.size, off, bases, qb, exc_pos, exc_chr, fix_cap=fix_cap)
        return arena, off, (bases, exc_pos, exc_chr, qb)
    assert transport == "resident"
    off1, off2 = kept
    qb = quality_bits(ctx, qa, d["bad_q"])
    ctx.submit_resident(slot, d["mode"], off, qb, arena_a=0, begin_a=int(off1[lo]), bytes_a=int(off1[hi] - off1[lo]), arena_b=1, begin_b=int(off2[lo]),
                        bytes_b=int(off2[hi] - off2[lo]), fix_cap=fix_cap)
    return a.copy(), off, qb


def finish(transport, ctx, slot, state):
    """the wait of a submitted batch: (corrected arena, ret, l, m, h)"""
    if transport in ("slots_lanes_on", "slots_lanes_off"):
        res = ctx.wait(slot)
        return (np.concatenate(state[0][0::3]),) + tuple(res)
    r = ctx.wait_packed(slot) if transport == "packed" else ctx.wait_resident(slot)
    ctx.apply_fixes(state[0], r[4], r[5])
    return (np.array(state[0]),) + tuple(r[:4])


def run(transport, armed, nospace=False):
    """the three batches through `transport` on a fresh context with the observers in `armed` open; returns the corrected arenas
    and result arrays of the batches, and what every armed observer has seen"""
    import torch
    d = dataset()
    ctx, kept = new_ctx(d, transport == "resident")
    ctx.set_slot_lanes(TRANSPORTS[transport][1])
    if "report" in armed:
        ctx.change_report_begin()
    if "census" in armed:
        ctx.dup_census_begin()
    if "trust" in armed:
        ctx.trust_profile_begin(TRUST_MIN)
    if "recount" in armed:
        ctx.recount_begin(MAX_BIN)
        ctx.recount_follow(True)
    cuts = unit_cuts(d, BATCHES)
    assert len(cuts) == BATCHES and all(hi > lo for lo, hi in cuts)
    out = {"batches": []}
    if transport == "correct_batch":
        for lo, hi in cuts:
            args = packed(rcorrector_amd, d, lo, hi)[4]
            res = ctx.correct_batch(d["mode"], *args)
            out["batches"].append((np.concatenate(args[0::3]),) + tuple(res))
    elif transport == "device":
        for lo, hi in cuts:
            a, qa, off, _, _ = packed(rcorrector_amd, d, lo, hi)
            n = len(off) - 1
            t_seq, t_q = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(qa.copy()).cuda()
            t_off = torch.from_numpy(off.astype(np.int32)).cuda()
            res = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(4)]
            ctx.correct_device(d["mode"], n, a.size, int(np.diff(off.astype(np.int64)).max()) - 1, t_seq, t_q, t_off, *res)
            ctx.sync()
            if "recount" in armed:   # (rc_correct_device has no wait and takes nothing: the caller adds what it corrected)
                ctx.recount_add_device(t_seq, a.size)
            out["batches"].append((t_seq.cpu().numpy(),) + tuple(r.cpu().numpy() for r in res))
    else:
        states = {}
        for slot, (lo, hi) in enumerate(cuts):                      # slots 0, 1 and 2, all in flight at once
            if nospace and slot == 1:
                submit(transport, ctx, d, kept, slot, lo, hi, fix_cap=1)
                wait = rcorrector_amd.load_library().rc_wait_packed if transport == "packed" else rcorrector_amd.load_library().rc_wait_resident
                assert wait(ctx._h, slot) == RC_STATUS_NOSPACE
                (ctx._inflight_packed if transport == "packed" else ctx._inflight_resident).pop(slot)
            states[slot] = submit(transport, ctx, d, kept, slot, lo, hi)
        for slot in sorted(states):
            out["batches"].append(finish(transport, ctx, slot, states[slot]))
    out.update(observed(ctx, armed))
    if "report" in armed:
        ctx.change_report_end()
    if "census" in armed:
        ctx.dup_census_end()
    if "trust" in armed:
        ctx.trust_profile_end()
    ctx.sync()
    ctx.close()
    return out


def observed(ctx, armed):
    """what the armed observers hold now (the recount session is finished by reading it)"""
    out = {}
    if "report" in armed:
        out["report"] = ctx.change_report()
    if "census" in armed:
        out["census"] = ctx.dup_census(MAX_BIN)
    if "trust" in armed:
        out["trust"] = ctx.trust_profile()
    if "recount" in armed:
        out["recount"] = ctx.recount_finish()
    return out


def flat(x, prefix=""):
    """a result as {path: array or scalar}"""
    if isinstance(x, dict):
        return {k2: v2 for k, v in x.items() for k2, v2 in flat(v, "%s.%s" % (prefix, k)).items()}
    if isinstance(x, (tuple, list)):
        return {k2: v2 for i, v in enumerate(x) for k2, v2 in flat(v, "%s[%d]" % (prefix, i)).items()}
    return {prefix: x}


def assert_same(got, want, what):
    got, want = flat(got), flat(want)
    assert sorted(got) == sorted(want), what
    for name in want:
        assert np.array_equal(np.asarray(got[name]), np.asarray(want[name])), "%s: %s differs" % (what, name)


_alone = {}


def alone(transport, observer):
    """the same batches with one observer armed (None: with nothing armed), each run once"""
    if (transport, observer) not in _alone:
        _alone[transport, observer] = run(transport, () if observer is None else (observer,))
    return _alone[transport, observer]


def assert_together_equals_alone(transport, got, what):
    assert_same(got["batches"], alone(transport, None)["batches"], "%s: corrected reads and ret / l / m / h" % what)
    for o in OBSERVERS:
        assert_same(got[o], alone(transport, o)[o], "%s: %s" % (what, o))
    # the alone runs saw something: the batches changed bases, and every unit and read was counted
    assert int(got["report"]["changes"].sum()) > 0 and int(got["report"]["reads"].sum()) == 2 * PAIRS
    assert got["census"]["units"] == PAIRS and int(got["trust"]["reads"].sum()) == 2 * PAIRS
    assert got["recount"][1]["total"] > 0


@pytest.mark.parametrize("transport", sorted(TRANSPORTS))
def test_all_observers_armed_together_see_what_each_sees_alone(transport):
    assert_together_equals_alone(transport, run(transport, OBSERVERS), transport)


@pytest.mark.parametrize("transport", ["packed", "resident"])
def test_a_batch_resubmitted_after_nospace_counts_once_in_every_observer(transport):
    """the middle batch's first submission has room for one substitution: RC_ERR_NOSPACE, nothing counted; submitted again with
    room, it is in every observer once -- the results are those of the run where it fitted at once"""
    middle = alone(transport, None)["batches"][1]
    assert int((middle[1] > 0).sum()) > 1, "the middle batch needs more than one substitution"
    assert_together_equals_alone(transport, run(transport, OBSERVERS, nospace=True), "%s, resubmitted" % transport)


def test_a_refused_batch_reaches_no_observer():
    """rc_correct_device on a paired batch with an odd read count: the error it always gave, and all four results as they were"""
    import torch
    d = dataset()
    ctx, _ = new_ctx(d, False)
    ctx.change_report_begin()
    ctx.dup_census_begin()
    ctx.trust_profile_begin(TRUST_MIN)
    ctx.recount_begin(MAX_BIN)
    ctx.recount_follow(True)
    lo, hi = unit_cuts(d, BATCHES)[0]
    args = packed(rcorrector_amd, d, lo, hi)[4]
    ctx.correct_batch(d["mode"], *args)
    before = observed(ctx, OBSERVERS[:3])
    a, qa, off, _, _ = packed(rcorrector_amd, d, lo, hi)
    n = len(off) - 2                                                  # an odd number of reads: the last one has no mate
    assert n % 2 == 1
    t_seq, t_q = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(qa.copy()).cuda()
    t_off = torch.from_numpy(off.astype(np.int32)).cuda()
    res = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(4)]
    with pytest.raises(rcorrector_amd.RcorrectorError,
                       match=r"^rc=%d: correct: paired mode needs an even number of reads \(got %d\)$" % (RC_STATUS_ARG, n)):
        ctx.correct_device(1, n, int(off[n]), int(np.diff(off.astype(np.int64)).max()) - 1, t_seq, t_q, t_off, *res)
    ctx.sync()
    assert np.array_equal(t_seq.cpu().numpy(), a)                     # nothing ran on it
    assert_same(observed(ctx, OBSERVERS[:3]), before, "after the refused batch")
    # the recount session holds the one accepted batch and nothing else: the same as a session that saw only that batch
    got = ctx.recount_finish()
    ctx.recount_begin(MAX_BIN)
    ctx.recount_add(np.concatenate(args[0::3]))
    assert_same(got, ctx.recount_finish(), "recount after the refused batch")
    ctx.change_report_end()
    ctx.dup_census_end()
    ctx.trust_profile_end()
    ctx.close()
