"""GPU: the trust profile's begin / get / end through every transport -- rc_correct_batch, rc_submit / rc_wait (lanes on, four
slots in flight), the packed and the resident transport and rc_correct_device: `before` must equal the restatement
(tests/test_trust_profile.py) of the fixture's reads, `after` that of the REFERENCE's corrected reads (ref/*.cor.*), however the
reads are cut into batches.  A packed batch that came back RC_STATUS_NOSPACE counts once; get repeats and accumulation goes on
across it; open or closed, nothing else a batch returns changes, and end gives the device memory back.  Every comparison is
exact integer equality, and every test ends with a sync."""
import os

import numpy as np
import pytest

import golden_util as gu
import rcorrector_amd
from test_duplicates import reads_of, via_correct_batch, via_device, via_packed, via_resident, via_slots
from test_recount import packed, unit_cuts
from test_trust_profile import FIELDS, assert_counts, fixture_restated
from test_weak_profile import fixture, packed_inputs

pytestmark = pytest.mark.gpu
RC_STATUS_NOSPACE = -6
NAME = "fx_pe_k23"
TRANSPORTS = {"correct_batch": (via_correct_batch, True, 3), "slots_lanes_on": (via_slots, True, 7), "slots_lanes_off": (via_slots, False, 5),
              "packed": (via_packed, True, 3), "resident": (via_resident, True, 3), "device": (via_device, True, 2)}
_ctx = {}


def shared_ctx():
    """the paired fixture and ONE context for all transports: the counter keeps the fixture's arenas (what the resident
    transport corrects), the table is the fixture's dump"""
    if not _ctx:
        f = dict(fixture(NAME))
        ctx = rcorrector_amd.Context(k=f["k"], max_fix_per_k=f["mfk"], device=0)
        f["a1"], f["off1"] = rcorrector_amd.pack_reads(f["seqs1"])
        f["a2"], f["off2"] = rcorrector_amd.pack_reads(f["seqs2"])
        ctx.count_keep(True)
        ctx.count_begin()
        ctx.count_add(f["a1"])
        ctx.count_add(f["a2"])
        ctx.count_finish(2)
        ctx.load_jfdump(os.path.join(gu.GOLDEN, NAME, "dump.jf"))
        ctx.set_run_params(ctx.estimate_error_rate(0.95), f["bad_q"])
        _ctx["v"] = (f, ctx)
    return _ctx["v"]


@pytest.fixture(scope="module", autouse=True)
def _close_shared():
    yield
    for _, ctx in _ctx.values():
        ctx.sync()
        ctx.close()
    _ctx.clear()


def assert_profile(got, f, want, min_count, batches=1, what=""):
    n = len(f["seqs1"])
    assert got["k"] == f["k"] and got["min_count"] == min_count, what
    assert got["reads"].tolist() == ([batches * n, batches * len(f["seqs2"])] if f["mode"] == 1 else [batches * n // 2] * 2 if f["mode"] == 2 else [batches * n, 0]), what
    for tag, w in zip(("before", "after"), want):
        assert_counts(got[tag], {x: batches * w[x] for x in FIELDS}, "%s %s" % (what, tag))


@pytest.mark.parametrize("transport", sorted(TRANSPORTS))
def test_before_and_after_through_every_transport(transport):
    f, ctx = shared_ctx()
    via, lanes, nb = TRANSPORTS[transport]
    ctx.set_slot_lanes(lanes)
    min_count = 3 if transport == "packed" else 1
    ctx.trust_profile_begin(min_count)
    c1, c2 = via(ctx, f, nb)
    got = ctx.trust_profile()
    ctx.trust_profile_end()
    ctx.set_slot_lanes(True)
    assert c1 == f["cor1"] and c2 == f["cor2"] and c1 != f["seqs1"]          # (what came back is what the reference wrote)
    assert_profile(got, f, fixture_restated(NAME, min_count), min_count, 1, transport)
    ctx.sync()


def test_interleaved_batches_and_single_end_batches():
    """mode 2 (fx_il_k23, even reads mate 0) through rc_correct_batch and the slots; mode 0: every read is mate 0"""
    f = fixture("fx_il_k23")
    from test_weak_profile import fixture_ctx
    ctx = fixture_ctx(f)
    want = fixture_restated("fx_il_k23")
    for via, nb in ((via_correct_batch, 2), (via_slots, 5)):
        ctx.trust_profile_begin()
        c1, _ = via(ctx, f, nb)
        got = ctx.trust_profile()
        ctx.trust_profile_end()
        assert c1 == f["cor1"]
        assert_profile(got, f, want, 1, 1, "fx_il_k23")
        assert int(got["before"]["windows"][1].sum()) > 0
    ctx.sync()
    ctx.close()


def test_a_batch_resubmitted_after_nospace_counts_once():
    f, ctx = shared_ctx()
    n = len(f["seqs1"])
    a, qa, off, _, _ = packed(rcorrector_amd, f, 0, n)
    arena, bases, exc_pos, exc_chr, qb = packed_inputs(ctx, a, qa, f["bad_q"])
    L, h = rcorrector_amd.load_library(), ctx._h
    ctx.trust_profile_begin()
    ctx.submit_packed(1, f["mode"], a.size, off, bases, qb, exc_pos, exc_chr, fix_pos=np.zeros(0, np.uint32), fix_chr=np.zeros(0, np.uint8))   # fix_cap = 0
    assert L.rc_wait_packed(h, 1) == RC_STATUS_NOSPACE
    ctx._inflight_packed.pop(1)
    got = ctx.trust_profile()
    assert got["reads"].tolist() == [0, 0] and int(got["before"]["windows"].sum()) == 0      # the batch that did not fit is in no profile yet
    ctx.submit_packed(1, f["mode"], a.size, off, bases, qb, exc_pos, exc_chr)
    r = ctx.wait_packed(1)
    assert len(r[4]) > 0
    ctx.apply_fixes(arena, r[4], r[5])
    cor = reads_of(arena, off)
    assert cor[:n] == f["cor1"] and cor[n:] == f["cor2"]
    assert_profile(ctx.trust_profile(), f, fixture_restated(NAME), 1, 1, "resubmitted")
    ctx.trust_profile_end()
    ctx.sync()


def test_get_repeats_and_accumulation_continues_across_it():
    f, ctx = shared_ctx()
    want = fixture_restated(NAME)
    ctx.trust_profile_begin()
    via_correct_batch(ctx, f, 2)
    first = ctx.trust_profile()
    again = ctx.trust_profile()
    assert_profile(first, f, want, 1, 1, "first get")
    for tag in ("before", "after"):
        assert all(np.array_equal(first[tag][x], again[tag][x]) for x in FIELDS)
    assert first["reads"].tolist() == again["reads"].tolist()
    via_slots(ctx, f, 4)                                                          # the same reads once more: every count doubles
    assert_profile(ctx.trust_profile(), f, want, 1, 2, "second round")
    ctx.trust_profile_end()
    ctx.trust_profile_begin(2)                                                    # a new profile starts empty
    got = ctx.trust_profile()
    assert got["reads"].tolist() == [0, 0] and int(got["after"]["windows"].sum()) == 0 and got["min_count"] == 2
    ctx.trust_profile_end()
    ctx.sync()


def test_open_or_closed_nothing_else_changes_and_end_frees():
    f, ctx = shared_ctx()
    n = len(f["seqs1"])

    def run():
        out = []
        for slot in (0, 2):
            a, qa, off, _, args = packed(rcorrector_amd, f, 0, n)
            ctx.submit(slot, f["mode"], *args)
            res = ctx.wait(slot)
            out.append(([r.copy() for r in res], args[0].copy(), args[3].copy()))
        a, qa, off, _, args = packed(rcorrector_amd, f, 0, n // 2)
        res = ctx.correct_batch(f["mode"], *args)
        out.append(([np.asarray(r).copy() for r in res], args[0].copy(), args[3].copy()))
        return out

    digest = ctx.table_digest()
    ctx.trust_profile_begin()                                                     # (one whole cycle first: the context's own buffers are
    run()                                                                         # grown, the lanes exist, every kernel's code is loaded)
    ctx.trust_profile_end()
    ctx.sync()
    free0 = ctx.device_memory()[0]
    s0 = ctx.summary()
    closed = run()
    s1 = ctx.summary()
    ctx.sync()
    assert ctx.device_memory()[0] == free0                                        # closed: nothing is allocated for it
    ctx.trust_profile_begin()
    opened = run()
    s2 = ctx.summary()
    got = ctx.trust_profile()
    assert got["reads"].tolist() == [2 * n + n // 2, 2 * n + n // 2] and ctx.device_memory()[0] < free0
    ctx.trust_profile_end()
    assert ctx.device_memory()[0] == free0                                        # end leaves nothing allocated
    for (res, s1a, s2a), (res0, s1b, s2b) in zip(opened, closed):
        assert all(np.array_equal(x, y) for x, y in zip(res, res0)) and np.array_equal(s1a, s1b) and np.array_equal(s2a, s2b)
    delta = lambda a, b: {key: b[key] - a[key] for key in a} if isinstance(a, dict) else tuple(y - x for x, y in zip(a, b))   # noqa: E731
    assert delta(s0, s1) == delta(s1, s2)                                         # the summary counts the same for either round
    assert ctx.table_digest() == digest
    ctx.sync()
