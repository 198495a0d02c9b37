"""GPU: the three per-read payloads -- weak-k-mer profile, k-mer depth, hit profile against a second table -- as one table of
kinds by slots: four batches in flight in slots 0 .. 3, each with another subset of the three registered, some arrays pageable and
some page-locked within one submit.  What a mix-up of a kind or a slot index would show: a value in the wrong array, an array
that was not registered written, a registration that outlives its submit.

The data set is test_read_depth's synthetic one (every window count, the longest read, letters outside ACGT, an empty read), a few
of its reads with a substitution for the corrector to find.  The yardstick of a registered array is the payload's own *_device
entry point on the batch's corrected arena -- the entry points test_weak_profile, test_read_depth and test_read_screen hold to
their restatements -- computed once per batch and shared by every case.  Every comparison is exact equality.
"""
import numpy as np
import pytest

import rcorrector_amd
from test_read_depth import device_depth, synthetic, table_of
from test_read_screen import device_screen
from test_weak_profile import device_profile, packed_inputs

pytestmark = pytest.mark.gpu
KINDS = ("weak", "depth", "screen")
BATCH_READS = (3, 64, 65, 130)
WEAK_MIN, SCREEN_MIN = 3, 2        # (different, so that one kind's threshold in the other's place shows)
SENTINEL = -9
_data, _want = {}, {}


def data():
    """k, the table's {code: count}, the screen table's, and the four batches as lists of reads"""
    if not _data:
        k, reads, counts = synthetic()
        pool = (reads * 2)[:sum(BATCH_READS)]
        assert len(pool) == sum(BATCH_READS)
        for i in range(0, len(pool), 5):                   # a substitution in the middle of every fifth read that is long enough
            r = pool[i]
            if len(r) >= 150 and r[75:76] in b"ACGT":
                pool[i] = r[:75] + b"ACGT"[(b"ACGT".index(r[75:76]) + 1) % 4:][:1] + r[76:]
        cuts = np.concatenate([[0], np.cumsum(BATCH_READS)])
        _data.update(k=k, counts=counts, screen={c: n for c, n in counts.items() if c % 3}, batches=[pool[cuts[i]:cuts[i + 1]] for i in range(4)])
    return _data


def contexts(lanes):
    d = data()
    ctx = rcorrector_amd.Context(k=d["k"], device=0)
    table_of(ctx, d["counts"])
    ctx.set_run_params(0.01, b"H")
    ctx.set_slot_lanes(lanes)
    screen = rcorrector_amd.Context(k=d["k"], device=0)
    table_of(screen, d["screen"])
    return ctx, screen


def want_of(ctx, screen, b, cor, off):
    """{kind: the kind's *_device entry point on batch b's corrected arena}: computed once, the arena the same in every case"""
    if b not in _want:
        _want[b] = (cor.copy(), {"weak": device_profile(ctx, cor, off, WEAK_MIN), "depth": device_depth(ctx, cor, off),
                                 "screen": device_screen(ctx, screen, cor, off, SCREEN_MIN)})
    assert np.array_equal(cor, _want[b][0]), "batch %d: corrected differently than in the first case" % b
    return _want[b][1]


def register(ctx, screen, kind, slot, total, pinned):
    out = None if pinned else np.zeros((total, 4), dtype=np.int32)
    if kind == "weak":
        return ctx.weak_profile_into(slot, total, WEAK_MIN, out=out)
    if kind == "depth":
        return ctx.read_depth_into(slot, total, out=out)
    return ctx.read_screen_into(slot, total, screen, SCREEN_MIN, out=out)


class Flight:
    """the four batches through one transport: submit(slot) starts batch `slot` there, wait(slot) returns its corrected arena"""

    def __init__(self, ctx, transport):
        self.ctx, self.transport, self.held = ctx, transport, {}
        self.off = [rcorrector_amd.pack_reads(reads)[1] for reads in data()["batches"]]

    def submit(self, slot):
        reads = data()["batches"][slot]
        a, off = rcorrector_amd.pack_reads(reads)
        qa, _ = rcorrector_amd.pack_reads([b"I" * len(r) for r in reads])
        if self.transport == "submit":
            self.ctx.submit(slot, 0, a, qa, off)
            self.held[slot] = a
        else:
            arena, bases, exc_pos, exc_chr, qb = packed_inputs(self.ctx, a, qa, b"H")
            self.ctx.submit_packed(slot, 0, a.size, off, bases, qb, exc_pos, exc_chr)
            self.held[slot] = arena

    def wait(self, slot):
        arena = self.held.pop(slot)
        if self.transport == "submit":
            self.ctx.wait(slot)
        else:
            r = self.ctx.wait_packed(slot)
            self.ctx.apply_fixes(arena, r[4], r[5])
        return np.array(arena)


@pytest.mark.parametrize("transport", ["submit", "packed"])
@pytest.mark.parametrize("lanes", [True, False], ids=["lanes_on", "lanes_off"])
def test_every_kind_in_every_slot_with_and_without_a_registration(lanes, transport):
    ctx, screen = contexts(lanes)
    fl = Flight(ctx, transport)
    totals = [len(o) - 1 for o in fl.off]
    # arrays[kind, slot]: the array the library was last given for that place, or one it never saw
    arrays = {(kind, s): ctx.host_array(totals[s] * 4, dtype=np.int32).reshape(totals[s], 4) for kind in KINDS for s in range(4)}
    changed = 0
    for rnd in (0, 1):
        registered = {}
        for a in arrays.values():                          # (nothing is in flight: last round's arrays stand for the places without one now)
            a[:] = SENTINEL
        for s in range(4):      # slot s: the kinds whose bits are s + 1, then the complement; all four in flight before the first wait
            bits = (s + 1) if rnd == 0 else (~(s + 1) & 7)
            pinned = (s + rnd) % 2 == 0
            for i, kind in enumerate(KINDS):
                if bits >> i & 1:
                    arrays[kind, s] = register(ctx, screen, kind, s, totals[s], pinned)
                    arrays[kind, s][:] = SENTINEL
                    registered[kind, s] = pinned
                    pinned = not pinned                    # (the kinds of one submit alternate: pageable beside page-locked)
            fl.submit(s)
        assert len(registered) == (5, 7)[rnd] and len(set(registered.values())) == 2
        assert all(len({(kind, s) in registered for s in range(4)}) == 2 for kind in KINDS)
        cors = {s: fl.wait(s) for s in (2, 0, 3, 1)}
        for s in range(4):
            want = want_of(ctx, screen, s, cors[s], fl.off[s])
            changed += int((cors[s] != rcorrector_amd.pack_reads(data()["batches"][s])[0]).sum())
            for kind in KINDS:
                got, what = arrays[kind, s], "round %d, slot %d, %s" % (rnd, s, kind)
                if (kind, s) in registered:
                    assert got.shape == want[kind].shape and np.array_equal(got, want[kind]), what
                else:
                    assert (got == SENTINEL).all(), what + ": written without a registration"
    # (the three yardsticks differ on every batch: an array filled by another kind's kernel cannot pass)
    assert all(not np.array_equal(w[1][a], w[1][b]) for w in _want.values() for a, b in (("weak", "depth"), ("weak", "screen"), ("depth", "screen")))
    assert changed > 0
    # registrations are one-shot: a plain submit into each slot writes none of the arrays
    before = {key: a.copy() for key, a in arrays.items()}
    for s in range(4):
        fl.submit(s)
    for s in range(4):
        fl.wait(s)
    for key, a in arrays.items():
        assert np.array_equal(a, before[key]), "%s of slot %d written by a submit without a registration" % key
    ctx.sync()
    ctx.close()
    screen.close()
