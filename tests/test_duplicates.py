"""GPU: the duplicate census -- rc_dup_census_begin / get / end, rc_read_keys_device and the binding's dup_census* methods: how
many reads (pairs, in modes 1 and 2) are exact copies of one another, in the bases as uploaded and in the bases as corrected.

The yardstick is pure Python over the strings: a collections.Counter of seq, or of (seq1, seq2) -- never the library.  `before`
is held to the Counter of the strings that went in, `after` to the Counter of the strings the same calls returned (the golden
fixtures: of the REFERENCE's ref/*.cor.* reads).  The keys themselves are held, word for word, to the host program
tests/hostmath/dup_key.cpp, which computes them from rc_dups.h byte by byte.  Every comparison is exact integer equality.
"""
import collections
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import rcorrector_amd
from test_recount import packed, unit_cuts
from test_weak_profile import fixture, fixture_ctx, packed_inputs

pytestmark = pytest.mark.gpu
RC_STATUS_ARG, RC_STATUS_STATE, RC_STATUS_NOSPACE = -1, -4, -6
MAX_BIN = 50
_LETTERS = np.frombuffer(b"ACGT", np.uint8)


# ---- the yardstick -------------------------------------------------------------------------------------------------------------
def units_of(mode, seqs1, seqs2=None):
    if mode == 0:
        return list(seqs1)
    if mode == 1:
        return list(zip(seqs1, seqs2))
    return list(zip(seqs1[0::2], seqs1[1::2]))


def census_of(units, max_bin=MAX_BIN):
    """(units, distinct, copies[max_bin + 1]) of a list of strings or of pairs of strings"""
    c = collections.Counter(units)
    copies = np.zeros(max_bin + 1, dtype=np.uint64)
    for v in c.values():
        copies[min(v, max_bin)] += 1
    return len(units), len(c), copies


def assert_census(got, before, after, what="", max_bin=MAX_BIN):
    for tag, units in (("before", before), ("after", after)):
        n, distinct, copies = census_of(units, max_bin)
        assert got["units"] == n, "%s: units" % what
        assert got["distinct_" + tag] == distinct, "%s: distinct %s: got %d, want %d" % (what, tag, got["distinct_" + tag], distinct)
        g = got["copies_" + tag]
        assert g.dtype == np.uint64 and np.array_equal(g, copies), "%s: copies_%s differ at %s" % (what, tag, np.nonzero(g != copies)[0][:10])
        assert int(g.sum()) == distinct


def reads_of(arena, off):
    a = np.asarray(arena).tobytes()
    return [a[int(off[i]):int(off[i + 1]) - 1] for i in range(len(off) - 1)]


# ---- 1. the kernel's keys against the host program's ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dup_key(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dup_key") / "dup_key")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-I", os.path.join(gu.ROOT, "rcorrector_amd", "csrc"),
                    os.path.join(gu.ROOT, "tests", "hostmath", "dup_key.cpp"), "-o", exe], check=True)
    return exe


def host_keys(exe, reads, mode):
    p = subprocess.run([exe, "keys", str(mode)], input=b"".join(r + b"\n" for r in reads), stdout=subprocess.PIPE, check=True)
    k = np.array([[int(w, 16) for w in ln.split()] for ln in p.stdout.decode().splitlines()], dtype=np.uint64)
    return k.reshape(-1, 2)


def device_keys(ctx, reads, mode, lead=0):
    """rc_read_keys_device on an arena that starts `lead` bytes behind a 16-byte boundary of device memory, with letters, not
    NULs, in front of it and behind it: what the kernel may read there must not reach a key"""
    import torch
    arena, off = rcorrector_amd.pack_reads(reads)
    n = len(reads)
    units = n if mode == 0 else n // 2
    buf = torch.full((lead + arena.size + 64,), ord("C"), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if arena.size:
        buf[lead:lead + arena.size] = torch.from_numpy(arena).cuda()
    t_off = torch.from_numpy(off.astype(np.int32)).cuda()
    out = torch.full((max(units, 1), 2), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.read_keys_device(buf.data_ptr() + lead, t_off, n, arena.size, mode, out)
    ctx.sync()
    return out.cpu().numpy().view(np.uint64)[:units]


def length_set_reads():
    """reads of every length 0..70 and 255, 256, 257, 1023 (an empty read among them), a few with N and lower case; 76 of them"""
    rng = np.random.default_rng(20260101)
    reads = [rng.choice(_LETTERS, size=n).tobytes() for n in list(range(71)) + [255, 256, 257, 1023]]
    reads.append(b"ACGTNNacgtN" * 9)
    assert len(reads) % 2 == 0 and b"" in reads
    return reads


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_read_keys_device_equals_the_host_programs_keys(dup_key, mode):
    ctx = rcorrector_amd.Context(k=23, device=0)   # (needs neither a table nor an open census)
    reads = length_set_reads()
    want = host_keys(dup_key, reads, mode)
    assert want.shape == ((76 if mode == 0 else 38), 2) and len({tuple(k) for k in want.tolist()}) == len(want)
    for lead in range(16):
        got = device_keys(ctx, reads, mode, lead)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert got.shape == want.shape and len(bad) == 0, "mode %d lead %d: unit %d: got %s, want %s" % (mode, lead, bad[0], got[bad[0]], want[bad[0]])
    # the order of the reads is the order of the keys: reversed reads, reversed single-end keys
    if mode == 0:
        assert np.array_equal(device_keys(ctx, reads[::-1], 0, 3), want[::-1])
    # n = 1 unit, an arena of one empty read, and n = 0
    one = reads[5:6] if mode == 0 else reads[5:7]
    assert np.array_equal(device_keys(ctx, one, mode, 9), host_keys(dup_key, one, mode))
    empty = [b""] if mode == 0 else [b"", b""]
    assert np.array_equal(device_keys(ctx, empty, mode, 15), host_keys(dup_key, empty, mode))
    assert device_keys(ctx, [], mode).shape == (0, 2)
    ctx.sync()
    ctx.close()


# ---- 2. a census through every transport -----------------------------------------------------------------------------------------
def synthetic(mode):
    """4 000 units of 600 distinct fragments, seeded multiplicities 1..300 (Zipf-like: the last bin of MAX_BIN = 50 is used),
    shuffled so that copies lie in different batches; a single seeded substitution in every eighth unit, so that what comes back
    differs from what went in.  mode 0: reads; 1 and 2: the fragment's two halves as mates."""
    rng = np.random.default_rng(77 + mode)
    frags = [rng.choice(_LETTERS, size=int(rng.integers(90, 151))).tobytes() for _ in range(600)]
    assert len(set(frags)) == 600
    mult = np.ones(600, dtype=np.int64)
    w = 1.0 / np.arange(1, 601)
    while mult.sum() < 4000:
        i = int(rng.choice(600, p=w / w.sum()))
        if mult[i] < 300:
            mult[i] += 1
    assert mult.max() == 300 and (mult > MAX_BIN).sum() >= 2 and (mult == 1).any()
    order = rng.permutation(np.repeat(np.arange(600), mult))
    s1, s2 = [], []
    for j, f in enumerate(order.tolist()):
        s = bytearray(frags[f])
        if j % 8 == 0 and mult[f] >= 8:
            p = int(rng.integers(30, len(s) - 30))
            s[p] = b"ACGT"[(b"ACGT".index(s[p]) + 1 + int(rng.integers(0, 3))) % 4]
        s, cut = bytes(s), len(s) // 2
        if mode == 0:
            s1.append(s)
        elif mode == 1:
            s1.append(s[:cut])
            s2.append(s[cut:])
        else:
            s1 += [s[:cut], s[cut:]]
    q = lambda seqs: [b"I" * len(x) for x in seqs]   # noqa: E731
    return dict(k=23, mfk=4, mode=mode, seqs1=s1, quals1=q(s1), seqs2=s2, quals2=q(s2), bad_q=b"H")


_synth = {}


def synth_ctx(mode):
    """the synthetic set of a mode and ONE context for all its transports: the table is counted from the set itself, and the
    counter keeps the arenas (what the resident transport corrects)"""
    if mode not in _synth:
        d = synthetic(mode)
        ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
        ctx.count_keep(True)
        ctx.count_begin()
        d["a1"], d["off1"] = rcorrector_amd.pack_reads(d["seqs1"])
        ctx.count_add(d["a1"])
        if mode == 1:
            d["a2"], d["off2"] = rcorrector_amd.pack_reads(d["seqs2"])
            ctx.count_add(d["a2"])
        ctx.count_finish(2)
        ctx.set_run_params(0.01, d["bad_q"])
        _synth[mode] = (d, ctx)
    return _synth[mode]


@pytest.fixture(scope="module", autouse=True)
def _close_synth():
    yield
    for _, ctx in _synth.values():
        ctx.sync()
        ctx.close()
    _synth.clear()


def split_mates(d, seqs, lo, hi):
    """the reads a batch [lo, hi) returned, as (mates 1, mates 2) lists"""
    n = hi - lo
    return (seqs[:n], seqs[n:]) if d["mode"] == 1 else (seqs, [])


def via_correct_batch(ctx, d, nb):
    out1, out2 = [], []
    for lo, hi in unit_cuts(d, nb):
        a, _, off, _, args = packed(rcorrector_amd, d, lo, hi)
        ctx.correct_batch(d["mode"], *args)
        m1, m2 = split_mates(d, reads_of(np.concatenate(args[0::3]), off), lo, hi)
        out1 += m1
        out2 += m2
    return out1, out2


def via_slots(ctx, d, nb):
    """rc_submit / rc_wait, up to four slots in flight (slots above 0 run in lanes of their own while lanes are on)"""
    res, busy = {}, {}

    def finish(s):
        i, lo, hi, off, args = busy.pop(s)
        ctx.wait(s)
        res[i] = split_mates(d, reads_of(np.concatenate(args[0::3]), off), lo, hi)

    for i, (lo, hi) in enumerate(unit_cuts(d, nb)):
        s = i % 4
        if s in busy:
            finish(s)
        a, _, off, _, args = packed(rcorrector_amd, d, lo, hi)
        busy[s] = (i, lo, hi, off, args)
        ctx.submit(s, d["mode"], *args)
    for s in sorted(busy, reverse=True):
        finish(s)
    return sum((res[i][0] for i in sorted(res)), []), sum((res[i][1] for i in sorted(res)), [])


def via_packed(ctx, d, nb):
    out1, out2 = [], []
    for i, (lo, hi) in enumerate(unit_cuts(d, nb)):
        a, qa, off, _, _ = packed(rcorrector_amd, d, lo, hi)
        arena, bases, exc_pos, exc_chr, qb = packed_inputs(ctx, a, qa, d["bad_q"])
        ctx.submit_packed(i % 3, d["mode"], a.size, off, bases, qb, exc_pos, exc_chr)
        r = ctx.wait_packed(i % 3)
        ctx.apply_fixes(arena, r[4], r[5])
        m1, m2 = split_mates(d, reads_of(arena, off), lo, hi)
        out1 += m1
        out2 += m2
    return out1, out2


def via_resident(ctx, d, nb):
    out1, out2 = [], []
    off1 = d["off1"]
    q1 = rcorrector_amd.pack_reads(d["quals1"])[0]
    if d["mode"] == 1:
        off2 = d["off2"]
        q2 = rcorrector_amd.pack_reads(d["quals2"])[0]
    for i, (lo, hi) in enumerate(unit_cuts(d, nb)):
        b1 = int(off1[hi] - off1[lo])
        off = [off1[lo:hi + 1].astype(np.int64) - int(off1[lo])]
        qs, host = [q1[off1[lo]:off1[hi]]], [d["a1"][off1[lo]:off1[hi]]]
        args = dict(arena_a=0, begin_a=int(off1[lo]), bytes_a=b1)
        if d["mode"] == 1:
            off.append(off2[lo + 1:hi + 1].astype(np.int64) - int(off2[lo]) + b1)
            qs.append(q2[off2[lo]:off2[hi]])
            host.append(d["a2"][off2[lo]:off2[hi]])
            args.update(arena_b=1, begin_b=int(off2[lo]), bytes_b=int(off2[hi] - off2[lo]))
        off = np.concatenate(off).astype(np.uint32)
        qb = ctx.host_array((int(off[-1]) + 7) // 8)
        ctx.pack_quality_bits(np.concatenate(qs), d["bad_q"], out=qb)
        ctx.submit_resident(i % 2, d["mode"], off, qb, **args)
        r = ctx.wait_resident(i % 2)
        host = np.concatenate(host).copy()
        ctx.apply_fixes(host, r[4], r[5])
        m1, m2 = split_mates(d, reads_of(host, off), lo, hi)
        out1 += m1
        out2 += m2
    return out1, out2


def via_device(ctx, d, nb):
    """rc_correct_device corrects the caller's memory in place and has no wait: the batch is in the census when the call returns"""
    import torch
    out1, out2 = [], []
    for lo, hi in unit_cuts(d, nb):
        a, qa, off, _, _ = packed(rcorrector_amd, d, lo, hi)
        n = len(off) - 1
        t_seq, t_q = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(qa.copy()).cuda()
        t_off = torch.from_numpy(off.astype(np.int32)).cuda()
        res = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(4)]
        ctx.correct_device(d["mode"], n, a.size, int(np.diff(off.astype(np.int64)).max()) - 1, t_seq, t_q, t_off, *res)
        ctx.sync()
        m1, m2 = split_mates(d, reads_of(t_seq.cpu().numpy(), off), lo, hi)
        out1 += m1
        out2 += m2
    return out1, out2


TRANSPORTS = {"correct_batch": (via_correct_batch, True), "slots_lanes_on": (via_slots, True), "slots_lanes_off": (via_slots, False),
              "packed": (via_packed, True), "resident": (via_resident, True), "device": (via_device, True)}


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("transport", sorted(TRANSPORTS))
def test_census_through_every_transport_in_1_3_and_7_batches(transport, mode):
    d, ctx = synth_ctx(mode)
    via, lanes = TRANSPORTS[transport]
    ctx.set_slot_lanes(lanes)
    before = units_of(mode, d["seqs1"], d["seqs2"])
    assert len(before) == 4000
    changed = 0
    for nb in (1, 3, 7):
        ctx.dup_census_begin()
        c1, c2 = via(ctx, d, nb)
        got = ctx.dup_census(MAX_BIN)
        ctx.dup_census_end()
        after = units_of(mode, c1, c2)
        assert_census(got, before, after, "%s mode %d, %d batches" % (transport, mode, nb))
        assert got["copies_before"][MAX_BIN] >= 2 and got["copies_before"][1] > 0          # (the last bin is used)
        changed += after != before
    assert changed == 3                              # (the planted substitutions were corrected: after is not before)
    ctx.set_slot_lanes(True)


# ---- 3. the golden fixtures: census `after` is the Counter of the reference's corrected reads ------------------------------------
@pytest.mark.parametrize("name", ["fx_pe_k23", "fx_il_k23", "fa_se_k23", "fx_k15"])
def test_census_after_equals_the_references_corrected_reads(name):
    f = fixture(name)
    if f["quals1"] is None:                          # FASTA: no qualities, the marker qual[0] == 0 (Reads.h:241)
        f = dict(f, quals1=[b"\0" * len(s) for s in f["seqs1"]])
    ctx = fixture_ctx(f)
    ctx.dup_census_begin()
    for lo, hi in unit_cuts(f, 2):
        ctx.correct_batch(f["mode"], *packed(rcorrector_amd, f, lo, hi)[4])
    got = ctx.dup_census(MAX_BIN)
    before, after = units_of(f["mode"], f["seqs1"], f["seqs2"]), units_of(f["mode"], f["cor1"], f["cor2"])
    assert before != after
    assert_census(got, before, after, name)
    ctx.dup_census_end()
    ctx.sync()
    ctx.close()


# ---- 4. distinct reads that become equal once corrected --------------------------------------------------------------------------
def test_reads_with_errors_become_copies_once_corrected():
    """every read of a fixture that the reference left unchanged (so the table trusts its k-mers), five times over, four of the
    five copies with one seeded substitution each: distinct before, and as many of them equal afterwards as the correction
    restores -- the assertion is the two Counters, of what went in and of what came back"""
    f = fixture("fx_pe_k23")
    rng = np.random.default_rng(5)
    clean = [(s, q) for s, q, c in zip(f["seqs1"], f["quals1"], f["cor1"]) if s == c and len(s) >= 100][:150]
    assert len(clean) == 150
    seqs, quals = [], []
    for s, q in clean:
        for copy in range(5):
            b = bytearray(s)
            if copy:
                p = int(rng.integers(25, len(b) - 25))
                b[p] = b"ACGT"[(b"ACGT".index(b[p]) + 1 + int(rng.integers(0, 3))) % 4]
            seqs.append(bytes(b))
            quals.append(q)
    d = dict(f, mode=0, seqs1=seqs, quals1=quals, seqs2=[], quals2=[])
    ctx = fixture_ctx(f)
    ctx.dup_census_begin()
    out = []
    for lo, hi in unit_cuts(d, 3):
        a, _, off, _, args = packed(rcorrector_amd, d, lo, hi)
        ctx.correct_batch(0, *args)
        out += reads_of(args[0], off)
    got = ctx.dup_census(MAX_BIN)
    assert_census(got, seqs, out, "planted errors")
    assert got["distinct_after"] < got["distinct_before"]           # (errors were removed, and with them distinct reads)
    ctx.dup_census_end()
    ctx.sync()
    ctx.close()


# ---- 5. a sort that crosses block boundaries -------------------------------------------------------------------------------------
def test_census_of_200000_units_through_read_keys_device():
    """200 000 reads of 40 bases with Zipf-like multiplicities: rc_read_keys_device's keys are equal exactly where the strings
    are, and the census's sort and run lengths over the same arena (one rc_correct_device batch with a census open, the table
    counted from the reads themselves) are the Counters of what went in and of what came back"""
    import torch
    rng = np.random.default_rng(11)
    n = 200000
    pool = rng.choice(_LETTERS, size=(30000, 40))
    rows = pool[np.minimum(rng.zipf(1.3, size=n) - 1, len(pool) - 1)]
    seqs = [r.tobytes() for r in rows]
    arena = np.zeros((n, 41), dtype=np.uint8)
    arena[:, :40] = rows
    arena = arena.reshape(-1)
    off = (np.arange(n + 1, dtype=np.int64) * 41).astype(np.int32)
    c = collections.Counter(seqs)
    assert max(c.values()) > MAX_BIN and len(c) > 5000      # (the set itself: a last bin in use, thousands of runs to sort)
    ctx = rcorrector_amd.Context(k=23, device=0)
    ctx.count_begin()
    ctx.count_add(arena)
    ctx.count_finish(2)
    ctx.set_run_params(0.01, b"H")
    t_seq, t_off = torch.from_numpy(arena).cuda(), torch.from_numpy(off).cuda()
    t_q = torch.full((arena.size,), ord("I"), dtype=torch.uint8, device="cuda")
    keys = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.read_keys_device(t_seq, t_off, n, arena.size, 0, keys)
    ctx.sync()
    k = keys.cpu().numpy()
    by_key = collections.Counter(zip(k[:, 0].tolist(), k[:, 1].tolist()))
    assert sorted(by_key.values()) == sorted(c.values())               # equal keys exactly where the strings are equal
    ctx.dup_census_begin()
    res = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(4)]
    ctx.correct_device(0, n, arena.size, 40, t_seq, t_q, t_off, *res)
    ctx.sync()
    got = ctx.dup_census(MAX_BIN)
    assert_census(got, seqs, reads_of(t_seq.cpu().numpy(), off), "200 000 units")
    full = ctx.dup_census(400000)                                        # nothing reaches the last bin: the multiplicities add up
    assert int((full["copies_before"] * np.arange(400001, dtype=np.uint64)).sum()) == n
    ctx.dup_census_end()
    ctx.sync()
    ctx.close()


# ---- 6. state ---------------------------------------------------------------------------------------------------------------------
def test_state_errors_and_what_end_leaves_behind():
    f = fixture("fx_pe_k23")
    ctx = fixture_ctx(f)
    L, h = rcorrector_amd.load_library(), ctx._h
    with pytest.raises(rcorrector_amd.RcorrectorError, match="rc_dup_census_begin"):
        ctx.dup_census(MAX_BIN)                                         # get without begin
    assert L.rc_dup_census_end(h) == RC_STATUS_STATE
    n = len(f["seqs1"])
    run = lambda: ctx.correct_batch(f["mode"], *packed(rcorrector_amd, f, 0, n)[4])   # noqa: E731
    ctx.dup_census_begin()                                               # (one whole cycle first: the context's own buffers are
    run()                                                                # grown and every kernel's code is loaded)
    assert ctx.dup_census(MAX_BIN)["units"] == n
    ctx.dup_census_end()
    ctx.sync()
    free0 = ctx.device_memory()[0]
    ctx.dup_census_begin()
    assert ctx.device_memory()[0] == free0                               # begin allocates nothing
    assert L.rc_dup_census_begin(h) == RC_STATUS_STATE                   # begin twice
    assert b"open already" in L.rc_last_error(h)
    run()
    got = ctx.dup_census(MAX_BIN)
    assert got["units"] == n and ctx.device_memory()[0] < free0          # the keys are in HBM
    assert L.rc_dup_census_get(h, 0, None) == RC_STATUS_ARG
    ctx.dup_census_end()
    assert ctx.device_memory()[0] == free0                               # end leaves nothing allocated
    run()                                                                # closed: nothing is launched or allocated for it
    ctx.sync()
    assert ctx.device_memory()[0] == free0
    ctx.dup_census_begin()                                               # a new census starts empty
    assert ctx.dup_census(MAX_BIN)["units"] == 0
    ctx.dup_census_end()
    ctx.close()


def test_a_batch_resubmitted_after_nospace_counts_once():
    f = fixture("fx_pe_k23")
    ctx = fixture_ctx(f)
    n = len(f["seqs1"])
    a, qa, off, _, _ = packed(rcorrector_amd, f, 0, n)
    arena, bases, exc_pos, exc_chr, qb = packed_inputs(ctx, a, qa, f["bad_q"])
    L, h = rcorrector_amd.load_library(), ctx._h
    ctx.dup_census_begin()
    ctx.submit_packed(1, f["mode"], a.size, off, bases, qb, exc_pos, exc_chr, fix_pos=np.zeros(0, np.uint32), fix_chr=np.zeros(0, np.uint8))   # fix_cap = 0
    assert L.rc_wait_packed(h, 1) == RC_STATUS_NOSPACE
    ctx._inflight_packed.pop(1)
    assert ctx.dup_census(MAX_BIN)["units"] == 0                         # the batch that did not fit is in no census yet
    ctx.submit_packed(1, f["mode"], a.size, off, bases, qb, exc_pos, exc_chr)
    r = ctx.wait_packed(1)
    assert len(r[4]) > 0
    ctx.apply_fixes(arena, r[4], r[5])
    cor = reads_of(arena, off)
    got = ctx.dup_census(MAX_BIN)
    assert_census(got, units_of(1, f["seqs1"], f["seqs2"]), units_of(1, cor[:n], cor[n:]), "resubmitted")
    ctx.dup_census_end()
    ctx.sync()
    ctx.close()
