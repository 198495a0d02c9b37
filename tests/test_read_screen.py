"""GPU: the per-read screen against a second k-mer set -- rc_read_screen_device / rc_read_screen_into and the binding's
read_screen_* methods: for every read its valid k-windows, those the screen table holds at least min_count times, the bases they
cover and their longest run (include/rcorrector_amd.h: rc_read_screen).

The yardstick is `restate` below, pure Python over a dict {canonical k-mer code: count} of the SCREEN set (missing = 0) that is
built from the text or the arrays the screen table was made from -- never from the library.  Every comparison is exact equality
on all four fields of every read, and every test ends with a sync of the context.
"""
import os

import numpy as np
import pytest

import datasets
import golden_util as gu
import rcorrector_amd
from seam_arena import canonical
from test_recount import packed, unit_cuts
from test_table_compare import WIDE, assert_layout, make_ctx
from test_read_depth import out_array as depth_out_array
from test_read_depth import restate_all as depth_restate_all
from test_weak_profile import RC_STATUS_ARG, RC_STATUS_NOSPACE, RC_STATUS_STATE, device_profile, fixture, fixture_ctx, packed_inputs, single_end
from test_weak_profile import out_array as weak_out_array

pytestmark = pytest.mark.gpu
_ACGT = frozenset(b"ACGT")
LETTERS = np.frombuffer(b"ACGT", np.uint8)


def restate(seq, k, counts, min_count=1):
    """the feature's contract for one read: (valid, hits, covered, longest)"""
    L = len(seq)
    valid = hits = longest = run = 0
    base = [0] * L
    for i in range(L - k + 1):
        w = seq[i:i + k]
        ok = _ACGT.issuperset(w)
        valid += ok
        if ok and counts.get(canonical(w), 0) >= min_count:
            hits += 1
            run += 1
            longest = max(longest, run)
            base[i:i + k] = [1] * k
        else:
            run = 0
    return (valid, hits, sum(base), longest)


def restate_all(seqs, k, counts, min_count=1):
    return np.array([restate(s, k, counts, min_count) for s in seqs], dtype=np.int32).reshape(len(seqs), 4)


def counts_of_reads(seqs, k):
    """{canonical code: occurrences} of the valid windows of `seqs`: what a counter kept from 1 on holds"""
    d = {}
    for s in seqs:
        for i in range(len(s) - k + 1):
            if _ACGT.issuperset(s[i:i + k]):
                c = canonical(s[i:i + k])
                d[c] = d.get(c, 0) + 1
    return d


def device_screen(ctx, screen, arena, off, min_count=1, lead=0, max_len=None):
    """rc_read_screen_device on a copy of `arena` that starts `lead` bytes behind a 16-byte boundary of device memory; the bytes
    in front of it and behind it are letters, not NULs: what the kernel may read there must not count"""
    import torch
    n = len(off) - 1
    buf = torch.full((lead + arena.size + 64,), ord("A"), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if arena.size:
        buf[lead:lead + arena.size] = torch.from_numpy(np.ascontiguousarray(arena)).cuda()
    t_off = torch.from_numpy(np.asarray(off).astype(np.int32)).cuda()
    out = torch.full((max(n, 1), 4), -7, dtype=torch.int32, device="cuda")
    if max_len is None:
        max_len = int(np.diff(np.asarray(off).astype(np.int64)).max()) - 1 if n else 0
    torch.cuda.synchronize()
    ctx.read_screen_device(screen, buf.data_ptr() + lead, t_off, n, arena.size, max_len, out, min_count=min_count)
    ctx.sync()
    return out.cpu().numpy()[:n]


def assert_screen(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.int32, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "%s: read %d: got %s, want %s (%d reads differ)" % (what, bad[0], got[bad[0]], want[bad[0]], len(bad))


def table_of(ctx, counts):
    codes = np.array(sorted(counts), dtype=np.uint64)
    ctx.table_build(codes, np.array([counts[int(c)] for c in codes], dtype=np.int32))


_screen_cache = {}


def fixture_screen(f):
    """(reads the screen set is made of, its dict): every third read of the fixture, every k-mer from one occurrence on"""
    if f["name"] not in _screen_cache:
        picked = (f["seqs1"] + f["seqs2"])[::3]
        _screen_cache[f["name"]] = (picked, counts_of_reads(picked, f["k"]))
    return _screen_cache[f["name"]]


def counted_screen_ctx(f):
    picked, _ = fixture_screen(f)
    screen = rcorrector_amd.Context(k=f["k"], device=0)
    screen.count_begin()
    screen.count_add(rcorrector_amd.pack_reads(picked)[0])
    screen.count_finish(1)
    return screen


# ---- 1. the device entry point against the restatement on golden fixtures ------------------------------------------------------
FIXTURES = {"fx_pe_k23": False, "fx_edge": True, "fx_varlen_n": True, "fx_k15": False, "fx_k32": False}   # name: holds a read without a valid window


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_device_screen_equals_the_restatement_on_golden_fixtures(name):
    f = fixture(name)
    _, counts = fixture_screen(f)
    screen = counted_screen_ctx(f)
    assert screen.table_stats()["entries"] == len(counts)
    ctx = rcorrector_amd.Context(k=f["k"], device=0)          # no table of its own
    seen, lens, changed = [], [], 0
    for which, seqs in (("uncorrected", f["seqs1"] + f["seqs2"]), ("corrected", f["cor1"] + f["cor2"])):
        changed += which == "corrected" and seqs != f["seqs1"] + f["seqs2"]
        arena, off = rcorrector_amd.pack_reads(seqs)
        want = restate_all(seqs, f["k"], counts)
        print("%s %s: %d reads, %d without a valid window, %d with a hit, %d all hits" %
              (name, which, len(seqs), int((want[:, 0] == 0).sum()), int((want[:, 1] > 0).sum()), int(((want[:, 1] == want[:, 0]) & (want[:, 0] > 0)).sum())))
        assert_screen(device_screen(ctx, screen, arena, off), want, "%s %s" % (name, which))
        seen.append(want)
        lens += [len(s) for s in seqs]
    assert changed == 1
    want, lens = np.concatenate(seen), np.array(lens)
    # (a regenerated fixture cannot empty the test)
    assert ((0 < want[:, 1]) & (want[:, 1] < want[:, 0])).any()
    assert ((want[:, 1] == want[:, 0]) & (want[:, 0] > 0)).any()
    assert ((want[:, 2] < lens) & (want[:, 1] > 0)).any()
    assert (want[:, 0] == 0).any() == FIXTURES[name]
    ctx.sync()
    ctx.close()
    screen.close()


# ---- 2. synthetic arenas over table_build screens ------------------------------------------------------------------------------
_synthetic_cache = {}


def synthetic(k):
    """reads assembled from segments of a sequence G whose windows are the screen set (counts 1, 2, 3, 5) and from junk that is
    not in it, and the set's dict"""
    if k in _synthetic_cache:
        return _synthetic_cache[k]
    rng = np.random.default_rng(20250911 + k)
    G = rng.choice(LETTERS, size=2400).tobytes()
    junk = lambda n: rng.choice(LETTERS, size=n).tobytes()   # noqa: E731
    counts = {}
    for i in range(len(G) - k + 1):
        counts.setdefault(canonical(G[i:i + k]), (1, 2, 3, 5)[int(rng.integers(0, 4))])

    def build(*parts):
        """a read of segments of G -- (start, bases) -- and junk -- bases: the junk's first letter is not the one that follows the
        segment in front of it in G, its last not the one ahead of the segment behind it, so that no hit run grows by chance"""
        out = bytearray()
        for n, p in enumerate(parts):
            if isinstance(p, tuple):
                out += G[p[0]:p[0] + p[1]]
                continue
            j = bytearray(junk(p))
            shun = set()
            if p and n > 0:
                shun.add(G[parts[n - 1][0] + parts[n - 1][1]])
                j[0] = next(c for c in b"ACGT" if c not in shun)
            if p and n + 1 < len(parts):
                shun = (shun if p == 1 else set()) | {G[parts[n + 1][0] - 1]}
                j[-1] = next(c for c in b"ACGT" if c not in shun)
            out += j
        return bytes(out)

    reads = [G[40:40 + n] for n in (k - 1, k, k + 1, k + 62, k + 63, k + 64, k + 127, k + 128, k + 255, k + 256)]
    reads += [G[j:j + 1023] for j in (0, 300, 600, 900, 1200)]            # five 1 023-base reads in a row: the run overflows the tile
    reads.append(junk(150))                                                 # no hit
    reads.append(build((100, k), 60))                                       # one hit, at the first window
    reads.append(build(60, (200, k)))                                       # ... at the last
    alt = junk(200)                                                         # alternating hits: every other window of `alt` is in the set
    for i in range(0, len(alt) - k + 1, 2):
        counts[canonical(alt[i:i + k])] = 2
    reads.append(alt)
    first = len(reads)
    a = 300                                                                 # two hits d windows apart: the union's boundary
    j = next(j for j in range(400, 2000) if G[j] == G[a + k - 1] and G[j + 1] != G[a + k] and G[j - 1] != G[a + k - 2])
    reads.append(build(5, (a, k - 1), (j, k), 5))                           # d = k - 1: the two windows share a base
    j = next(j for j in range(400, 2000) if G[j] != G[a + k] and G[j - 1] != G[a + k - 1])
    reads.append(build(5, (a, k), (j, k), 5))                               # d = k: they touch
    reads.append(build(5, (a, k), 1, (500, k), 5))                          # d = k + 1: a base between them
    reads.append(build(50, (700, 14 + k - 1), 30))                          # a run of hits at windows 50 .. 63
    reads.append(build(64, (800, 20 + k - 1), 30))                          # ... 64 .. 83
    reads.append(build((900, 30 + k - 1), 10 + k, (1000, 100 + k - 1), 7))  # a short run, then one across two words
    s = bytearray(G[1100:1100 + 160])                                        # an N and a lower-case letter inside a run of hits
    s[50], s[110] = ord("N"), ord("g")
    reads.append(bytes(s))
    reads.append(b"NNNN" + G[0:k - 1])                                       # bases, but no valid window
    reads.append(b"")
    patterns = (first, len(reads))
    reads += [G[j:j + 150] if j % 3 else G[j:j + 70] + junk(80) for j in range(0, 1300, 20)]   # 65 ordinary reads: a second workgroup
    _synthetic_cache[k] = (reads, counts, patterns)
    return _synthetic_cache[k]


@pytest.mark.parametrize("lead,min_count", [(0, 1), (1, 2), (15, 6)])
@pytest.mark.parametrize("k", [15, 23, 32])
def test_device_screen_on_synthetic_arenas(k, lead, min_count):
    reads, counts, (first, _) = synthetic(k)
    screen = rcorrector_amd.Context(k=k, device=0)
    table_of(screen, counts)
    ctx = rcorrector_amd.Context(k=k, device=0)
    want = restate_all(reads, k, counts, min_count)
    if min_count == 1:      # the patterns are what their construction says
        assert want[:10, 0].tolist() == [0, 1, 2, 63, 64, 65, 128, 129, 256, 257] and (want[:10, 1] == want[:10, 0]).all()
        assert (want[10:15] == [1024 - k, 1024 - k, 1023, 1024 - k]).all()
        assert tuple(want[15]) == (151 - k, 0, 0, 0) and tuple(want[16]) == (61, 1, k, 1) and tuple(want[17]) == (61, 1, k, 1)
        assert tuple(want[18]) == (201 - k, (202 - k) // 2, (200 - k) // 2 * 2 + k, 1)
        assert [tuple(w[1:]) for w in want[first:first + 3]] == [(2, 2 * k - 1, 1), (2, 2 * k, 1), (2, 2 * k, 1)]
        assert tuple(want[first + 3][1:]) == (14, 14 + k - 1, 14) and tuple(want[first + 4][1:]) == (20, 20 + k - 1, 20)
        assert tuple(want[first + 5][1:]) == (130, 130 + 2 * (k - 1), 100)
        assert want[first + 6][0] == 161 - k - 2 * k == want[first + 6][1] and want[first + 6][3] == 110 - k + 1 - 51
        assert tuple(want[first + 7]) == (0, 0, 0, 0) and tuple(want[first + 8]) == (0, 0, 0, 0)
    elif min_count == 6:    # above every count
        assert (want[:, 1:] == 0).all() and (want[:, 0] > 0).any()
    else:
        assert ((0 < want[:, 1]) & (want[:, 1] < want[:, 0])).sum() > 20
    assert len(reads) > 64 + 1
    arena, off = rcorrector_amd.pack_reads(reads)
    assert_screen(device_screen(ctx, screen, arena, off, min_count, lead), want, "k %d lead %d min_count %d" % (k, lead, min_count))
    if lead == 0:           # 65 reads in one call, one read, none; offsets that leave the arena; a read beyond the limit
        for seqs in (reads[-65:], reads[-1:], []):
            arena, off = rcorrector_amd.pack_reads(seqs)
            assert_screen(device_screen(ctx, screen, arena, off, min_count, 3), restate_all(seqs, k, counts, min_count), "%d reads" % len(seqs))
        seqs = reads[-10:]
        arena, off = rcorrector_amd.pack_reads(seqs)
        want = restate_all(seqs, k, counts, min_count)
        bad = off.astype(np.int64).copy()
        bad[4] = arena.size + 1000
        want[3] = want[4] = 0
        assert_screen(device_screen(ctx, screen, arena, bad.astype(np.uint32), min_count, 0, max_len=150), want, "offsets outside")
        seqs = [reads[-1], reads[10] + reads[11][:100], reads[-2]]
        arena, off = rcorrector_amd.pack_reads(seqs)
        want = restate_all(seqs, k, counts, min_count)
        want[1] = 0
        assert_screen(device_screen(ctx, screen, arena, off, min_count, 0, max_len=150), want, "a read beyond the limit")
    ctx.sync()
    ctx.close()
    screen.close()


# ---- 3. layouts: the screen table's, not the context's -------------------------------------------------------------------------
def genome_set(seed, k, n, count=lambda i: 1 + i % 7):
    """a random sequence of n + k - 1 bases and the (codes, counts) of its windows' canonical k-mers"""
    G = np.random.default_rng(seed).choice(LETTERS, size=n + k - 1).tobytes()
    d = {}
    for i in range(n):
        d.setdefault(canonical(G[i:i + k]), count(i))
    return G, d


def dict_arrays(d):
    codes = np.array(sorted(d), dtype=np.uint64)
    return codes, np.array([d[int(c)] for c in codes], dtype=np.int32)


@pytest.mark.parametrize("screen_is_small", [True, False], ids=["ext_screen_under_plain_ctx", "plain_screen_under_ext_ctx"])
def test_the_screen_tables_layout_decides_not_the_contexts(screen_is_small, monkeypatch):
    k = 23
    Gs, small = genome_set(71, k, 3000)          # PACKED, 4 extension bits
    Gb, big = genome_set(72, k, 30000)           # PACKED, none
    a = make_ctx(rcorrector_amd, k, *dict_arrays(small), monkeypatch)
    b = make_ctx(rcorrector_amd, k, *dict_arrays(big), monkeypatch)
    assert_layout(a, k, len(small), 1, 4)
    assert_layout(b, k, len(big), 1, 0)
    reads = [Gs[j:j + 100] + Gb[5 * j:5 * j + 100] for j in range(0, 2800, 35)] + [Gb[j:j + 151] for j in range(0, 6000, 75)] + [Gs[j:j + 151] for j in range(0, 2800, 75)]
    arena, off = rcorrector_amd.pack_reads(reads)
    ctx, screen, counts = (b, a, small) if screen_is_small else (a, b, big)
    for mc in (1, 4):
        want = restate_all(reads, k, counts, mc)
        assert ((0 < want[:, 1]) & (want[:, 1] < want[:, 0])).any() and (want[:, 1] == 0).any() and (want[:, 1] == want[:, 0]).any() == (mc == 1)
        assert_screen(device_screen(ctx, screen, arena, off, mc), want, "min_count %d" % mc)
    w = make_ctx(rcorrector_amd, k, *dict_arrays(small), monkeypatch, WIDE)     # and a WIDE screen under either
    assert w.table_layout() == 0
    assert_screen(device_screen(ctx, w, arena, off, 2), restate_all(reads, k, small, 2), "wide screen")
    ctx.sync()
    a.close()
    b.close()
    w.close()


def test_counts_beyond_a_packed_slots_field_compare_like_any_other(monkeypatch):
    k, limit = 23, 1 << 27                       # ext 0: the slot's count field holds up to 2^27 - 2, 2^27 - 1 is its mark
    G, d = genome_set(73, k, 30000)
    pins = {limit - 2: 100, limit - 1: 200, limit: 300, limit + 1: 400, datasets.INT_MAX: 500}
    for c, at in pins.items():
        for i in range(at, at + 40):             # 40 consecutive windows of G at each pinned count
            d[canonical(G[i:i + k])] = c
    screen = make_ctx(rcorrector_amd, k, *dict_arrays(d), monkeypatch)
    assert_layout(screen, k, len(d), 1, 0)
    assert datasets.huge_overflowing(list(d.values()), 0) >= 4 * 40
    ctx = rcorrector_amd.Context(k=k, device=0)
    reads = [G[j:j + 150] for j in range(50, 600, 10)]
    arena, off = rcorrector_amd.pack_reads(reads)
    for mc in (limit - 1, limit, limit + 1, datasets.INT_MAX):
        want = restate_all(reads, k, d, mc)
        assert (want[:, 1] > 0).any() and (want[:, 1] < want[:, 0]).all()
        assert_screen(device_screen(ctx, screen, arena, off, mc), want, "min_count %d" % mc)
    ctx.sync()
    ctx.close()
    screen.close()


# ---- 4. a context screened against itself: the weak profile's kernels as cross-check ------------------------------------------
@pytest.mark.parametrize("min_count", [1, 3])
def test_screen_is_ctx_gives_valid_minus_weak(min_count):
    f = fixture("fx_pe_k23")
    ctx = fixture_ctx(f)
    seqs = f["seqs1"] + f["seqs2"]
    arena, off = rcorrector_amd.pack_reads(seqs)
    got = device_screen(ctx, ctx, arena, off, min_count)
    weak = device_profile(ctx, arena, off, min_count)
    assert np.array_equal(got[:, 1], got[:, 0] - weak[:, 0]) and (weak[:, 0] > 0).any() and (got[:, 1] > 0).any()
    assert_screen(got, restate_all(seqs, f["k"], f["counts_of"], min_count), "against its own table")
    ctx.sync()
    ctx.close()


# ---- 5. transports -------------------------------------------------------------------------------------------------------------
# The expected values are the restatement on the corrected reads the same call returned.
def reads_of(arena, off):
    raw = np.ascontiguousarray(arena).tobytes()
    return [raw[int(off[i]):int(off[i + 1]) - 1] for i in range(len(off) - 1)]


def out_array(ctx, slot, total, screen, min_count, pinned):
    if pinned:
        out = ctx.read_screen_into(slot, total, screen, min_count)
    else:
        out = ctx.read_screen_into(slot, total, screen, min_count, out=np.zeros((total, 4), dtype=np.int32))
    out[:] = -9
    return out


@pytest.mark.parametrize("lanes", [True, False], ids=["lanes_on", "lanes_off"])
def test_screen_into_through_correct_batch_submit_and_packed_with_the_other_two_beside_it(lanes):
    f = fixture("fx_pe_k23")
    _, counts = fixture_screen(f)
    screen = counted_screen_ctx(f)
    ctx = fixture_ctx(f)
    ctx.set_slot_lanes(lanes)
    k, corrected_bases = f["k"], 0
    for d, mc in ((f, 1), (single_end(f), 2)):
        (lo0, hi0), (lo1, hi1) = unit_cuts(d, 2)
        # rc_correct_batch (slot 0), pinned
        a, qa, off, _, args = packed(rcorrector_amd, d, lo0, hi0)
        out = out_array(ctx, 0, len(off) - 1, screen, mc, True)
        before = a.copy()
        ctx.correct_batch(d["mode"], *args)
        cor = np.concatenate(args[0::3])
        corrected_bases += int((cor != before).sum())
        want0 = restate_all(reads_of(cor, off), k, counts, mc)
        assert (want0[:, 1] > 0).any() and (want0[:, 1] == 0).any()
        assert_screen(out, want0, "mode %d correct_batch" % d["mode"])
        # rc_submit / rc_wait, two slots in flight, all three registrations on the second
        a0, _, off0, _, args0 = packed(rcorrector_amd, d, lo0, hi0)
        a1, _, off1, _, args1 = packed(rcorrector_amd, d, lo1, hi1)
        t1 = len(off1) - 1
        out0 = out_array(ctx, 1, len(off0) - 1, screen, mc, False)
        out1, weak1, depth1 = out_array(ctx, 2, t1, screen, mc, True), weak_out_array(ctx, 2, t1, 2, True), depth_out_array(ctx, 2, t1, False)
        ctx.submit(1, d["mode"], *args0)
        ctx.submit(2, d["mode"], *args1)
        ctx.wait(2)
        ctx.wait(1)
        cor1 = np.concatenate(args1[0::3])
        assert np.array_equal(np.concatenate(args0[0::3]), cor)
        assert_screen(out0, want0, "mode %d submit, slot 1" % d["mode"])
        want1 = restate_all(reads_of(cor1, off1), k, counts, mc)
        assert_screen(out1, want1, "mode %d submit, slot 2" % d["mode"])
        assert np.array_equal(weak1, device_profile(ctx, cor1, off1, 2))
        assert np.array_equal(depth1, depth_restate_all(reads_of(cor1, off1), k, f["counts_of"]))
        # one shot: the following submit leaves a sentinel-filled array untouched; so does one whose registration was withdrawn
        out1[:] = -9
        a1, _, off1, _, args1 = packed(rcorrector_amd, d, lo1, hi1)
        ctx.submit(2, d["mode"], *args1)
        ctx.wait(2)
        assert (out1 == -9).all()
        withdrawn = out_array(ctx, 2, t1, screen, mc, True)
        ctx.read_screen_withdraw(2)
        a1, _, off1, _, args1 = packed(rcorrector_amd, d, lo1, hi1)
        ctx.submit(2, d["mode"], *args1)
        ctx.wait(2)
        assert (withdrawn == -9).all() and (out1 == -9).all()
        # rc_submit_packed / rc_wait_packed
        a, qa, off, _, _ = packed(rcorrector_amd, d, lo0, hi0)
        arena, bases, exc_pos, exc_chr, qb = packed_inputs(ctx, a, qa, f["bad_q"])
        out = out_array(ctx, 3, len(off) - 1, screen, mc, False)
        ctx.submit_packed(3, d["mode"], a.size, off, bases, qb, exc_pos, exc_chr)
        r = ctx.wait_packed(3)
        ctx.apply_fixes(arena, r[4], r[5])
        assert np.array_equal(arena, cor)
        assert_screen(out, want0, "mode %d packed" % d["mode"])
    assert corrected_bases > 0
    ctx.sync()
    ctx.close()
    screen.close()


@pytest.mark.parametrize("lanes", [True, False], ids=["lanes_on", "lanes_off"])
def test_screen_into_through_the_resident_transport(lanes):
    d = fixture("fx_pe_k23")
    _, counts = fixture_screen(d)
    screen = counted_screen_ctx(d)
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    ctx.set_slot_lanes(lanes)
    a1, off1 = rcorrector_amd.pack_reads(d["seqs1"])
    a2, off2 = rcorrector_amd.pack_reads(d["seqs2"])
    q = [rcorrector_amd.pack_reads(d["quals1"])[0], rcorrector_amd.pack_reads(d["quals2"])[0]]
    ctx.count_keep(True)
    ctx.count_begin()
    ctx.count_add(a1)
    ctx.count_add(a2)
    off = np.concatenate([off1, (off2[1:].astype(np.int64) + a1.size).astype(np.uint32)])
    ctx.count_finish(2)
    ctx.load_jfdump(os.path.join(gu.GOLDEN, d["name"], "dump.jf"))
    ctx.set_run_params(ctx.estimate_error_rate(0.95), d["bad_q"])
    qb = ctx.host_array((int(off[-1]) + 7) // 8)
    ctx.pack_quality_bits(np.concatenate(q), d["bad_q"], out=qb)
    for slot, pinned in ((0, True), (3, False)):
        out = out_array(ctx, slot, len(off) - 1, screen, 1, pinned)
        ctx.submit_resident(slot, 1, off, qb, arena_a=0, begin_a=0, bytes_a=a1.size, arena_b=1, begin_b=0, bytes_b=a2.size)
        r = ctx.wait_resident(slot)
        host = np.concatenate([a1, a2])
        assert len(r[4]) > 0
        ctx.apply_fixes(host, r[4], r[5])
        assert_screen(out, restate_all(reads_of(host, off), d["k"], counts), "resident slot %d" % slot)
    ctx.sync()
    ctx.close()
    screen.close()


def test_a_batch_resubmitted_after_nospace_must_register_again():
    f = fixture("fx_pe_k23")
    _, counts = fixture_screen(f)
    screen = counted_screen_ctx(f)
    ctx = fixture_ctx(f)
    n = len(f["seqs1"])
    a, qa, off, _, _ = packed(rcorrector_amd, f, 0, n)
    arena, bases, exc_pos, exc_chr, qb = packed_inputs(ctx, a, qa, f["bad_q"])
    L, h = rcorrector_amd.load_library(), ctx._h
    out = out_array(ctx, 1, 2 * n, screen, 1, False)
    ctx.profile(True)
    ctx.profile_reset()
    ctx.submit_packed(1, f["mode"], a.size, off, bases, qb, exc_pos, exc_chr, fix_pos=np.zeros(0, np.uint32), fix_chr=np.zeros(0, np.uint8))   # fix_cap = 0
    assert L.rc_wait_packed(h, 1) == RC_STATUS_NOSPACE
    ctx._inflight_packed.pop(1)
    assert (out == -9).all()                      # (a pageable array is written by the wait that succeeds, and only by it)
    refused = ctx.profile_get(8)[1]
    ctx.submit_packed(1, f["mode"], a.size, off, bases, qb, exc_pos, exc_chr)     # the registration went with the refused submit
    ctx.wait_packed(1)
    assert (out == -9).all() and ctx.profile_get(8)[1] == refused == 1
    out = out_array(ctx, 1, 2 * n, screen, 1, False)
    ctx.submit_packed(1, f["mode"], a.size, off, bases, qb, exc_pos, exc_chr)
    res = ctx.wait_packed(1)
    assert ctx.profile_get(8)[1] == refused + 1
    host = a.copy()
    ctx.apply_fixes(host, res[4], res[5])
    ctx.profile(False)
    assert_screen(out, restate_all(reads_of(host, off), f["k"], counts), "resubmitted")
    ctx.sync()
    ctx.close()
    screen.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_their_texts():
    import torch
    f = fixture("fx_k15")
    L = rcorrector_amd.load_library()
    seqs = f["seqs1"][:8]
    arena, off = rcorrector_amd.pack_reads(seqs)
    t_seq, t_off = torch.from_numpy(arena).cuda(), torch.from_numpy(off.astype(np.int32)).cuda()
    t_out = torch.zeros((8, 4), dtype=torch.int32, device="cuda")
    host = np.zeros((8, 4), dtype=np.int32)
    torch.cuda.synchronize()
    screen = fixture_ctx(f)
    ctx = rcorrector_amd.Context(k=f["k"], device=0)
    err = lambda: L.rc_last_error(ctx._h)   # noqa: E731

    def dev(s=screen, seq=t_seq.data_ptr(), off_p=t_off.data_ptr(), out=t_out.data_ptr(), nbytes=arena.size, max_len=100, mc=1):
        return L.rc_read_screen_device(ctx._h, s._h if s else None, seq, off_p, 8, nbytes, max_len, mc, out)

    for kw in (dict(s=None), dict(seq=None), dict(off_p=None), dict(out=None)):
        assert dev(**kw) == RC_STATUS_ARG and b"null pointer" in err(), kw
    assert dev(nbytes=1 << 32) == RC_STATUS_ARG and b"4 GiB" in err()
    assert dev(max_len=1024) == RC_STATUS_ARG and b"1023-base limit" in err() and dev(max_len=1023) == 0
    assert dev(mc=0) == RC_STATUS_ARG and b"min_count" in err()
    other_k = rcorrector_amd.Context(k=f["k"] + 2, device=0)
    table_of(other_k, {5: 2, 9: 3})
    assert dev(s=other_k) == RC_STATUS_ARG and b"of k = 17" in err()
    bare = rcorrector_amd.Context(k=f["k"], device=0)
    assert dev(s=bare) == RC_STATUS_STATE and b"no k-mer table in the screen context" in err()
    assert dev(s=ctx) == RC_STATUS_STATE                                         # itself, and it has none
    if torch.cuda.device_count() > 1:
        far = rcorrector_amd.Context(k=f["k"], device=1)
        table_of(far, {5: 2, 9: 3})
        assert dev(s=far) == RC_STATUS_ARG and b"on device 1" in err()
        far.close()
    into = lambda slot, s, mc, out: L.rc_read_screen_into(ctx._h, slot, s._h if s else None, mc, out)   # noqa: E731
    assert into(4, screen, 1, host.ctypes.data) == RC_STATUS_ARG and into(-1, screen, 1, host.ctypes.data) == RC_STATUS_ARG and b"no slot" in err()
    assert into(0, None, 1, host.ctypes.data) == RC_STATUS_ARG and into(0, screen, 0, host.ctypes.data) == RC_STATUS_ARG and b"min_count" in err()
    assert into(0, other_k, 1, host.ctypes.data) == RC_STATUS_ARG and b"of k = 17" in err()
    assert into(0, bare, 1, host.ctypes.data) == RC_STATUS_STATE and b"table" in err()
    assert into(0, None, 0, None) == 0                                           # withdrawing looks at neither
    assert L.rc_read_screen_device(ctx._h, screen._h, None, None, 0, 0, 0, 1, None) == 0
    assert dev() == 0
    ctx.sync()
    assert_screen(t_out.cpu().numpy(), restate_all(seqs, f["k"], f["counts_of"]))
    # the contexts still correct a batch afterwards
    a, qa, off2, _, args = packed(rcorrector_amd, f, 0, 50)
    before = a.copy()
    res = screen.correct_batch(f["mode"], *args)
    assert len(res[0]) == 50 and (np.concatenate(args[0::3]) != before).any()
    screen.sync()
    for c in (ctx, other_k, bare, screen):
        c.close()
