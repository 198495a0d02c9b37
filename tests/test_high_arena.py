"""GPU: the device entry points on arenas above 2 GiB, up to the last byte the library accepts (nbytes = 2^32 - 1).

Every test places a small batch (tests/high_arena.py) where the uint32 offsets are large -- the `mid` windows across byte 2^31,
at lead 0, 5 and 15; the `top` window up to byte 2^32 - 2, at every lead 0..15 -- and compares every output row, key and tally
word with the CPU reference the entry point's own test file compares with, run on the reads as byte strings: the reference never
sees an offset.  The arenas are two uninitialised 4 GiB allocations shared by the module; only the window is written.
tests/test_high_arena_cases.py shows on the CPU that the expected results are not empty ones.

read_merge_device, the one entry point that writes an arena and an offset array, has its high-offset coverage here too (section 7):
both modes at every placement with qualities and two more 4 GiB arenas for its output, and one filled arena whose merged output
passes 2^31, handed on to read_trim_device as it lies in HBM.  tests/test_read_merge.py keeps the contract at small offsets."""
import functools

import numpy as np
import pytest

import datasets
import high_arena as ha
import merge_model as mm
import recur_model as rm
import rcorrector_amd
import test_mate_overlap_host as mho
import test_trust_profile as ttp
import trim_model as tm
from rcorrector_amd import binding as B
from test_duplicates import dup_key, host_keys  # noqa: F401  (dup_key: the fixture that builds the host program)
from test_read_depth import restate_all as depth_rows
from test_read_depth import table_of
from test_read_merge import POISON
from test_read_merge import assert_equal as assert_merge_equal
from test_read_merge import params_of as merge_params_of
from test_read_screen import restate_all as screen_rows
from test_read_trim import params_of
from test_weak_profile import restate_all as weak_rows

pytestmark = pytest.mark.gpu
NEED_FREE = 16 << 30
B_TALLY = B.TRIM_TALLY_WORDS


@pytest.fixture(scope="module")
def arenas():
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip("%.1f GiB of device memory are free, the arenas above 2 GiB need %d" % (free / 2.0 ** 30, NEED_FREE >> 30))
    bufs = [ha.allocate(), ha.allocate()]
    yield bufs
    del bufs[:]
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def tables():
    """a context per k with the table of high_arena.table_case"""
    made = {}
    for k, counts in ha.table_case()[1].items():
        made[k] = rcorrector_amd.Context(k=k, device=0)
        table_of(made[k], counts)
    yield made
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def bare():
    c = rcorrector_amd.Context(k=23, max_fix_per_k=4, device=0)      # (no table: trimming, the overlap report and the keys need none)
    yield c
    c.close()


def placements(reads, mids):
    """(number, window, lead) of every run of a batch"""
    return [(i, w, lead) for i, (w, leads) in enumerate(ha.windows(reads, mids)) for lead in leads]


def where(w, lead):
    return "%s lead %d" % (w["name"] + ("" if w["name"] == "top" else " (first read at %d)" % w["off"][0]), lead)


def differing_rows(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return "" if len(bad) == 0 else "%d rows differ, first read %d of %d: got %s, want %s" % (len(bad), bad[0], len(want), got[bad[0]], want[bad[0]])


def report(failures):
    assert not failures, "%d placements differ:\n%s" % (len(failures), "\n".join(failures))


# ---- 1. the per-read profiles over a table, k = 23 and k = 5 --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table_want(what, k, mode=0):
    reads, counts = ha.table_case()
    mc = ha.TABLE_MIN_COUNT[k]
    if what == "depth":
        return depth_rows(reads, k, counts[k])
    if what == "screen":
        return screen_rows(reads, k, counts[k], mc)
    if what == "weak":
        return weak_rows(reads, k, counts[k], mc)
    return ttp.restate_reads(reads, mode, k, counts[k], mc)


def run_rows(arenas, tables, k, what, launch):
    """launch(ctx, address, t_off, n, nbytes, max_len, out) at every placement; out: n x 4 int32"""
    import torch
    reads = ha.table_case()[0]
    want, ctx, failures = table_want(what, k), tables[k], []
    for _, w, lead in placements(reads, ha.TABLE_MID):
        p, t_off = ha.put(arenas[0], lead, w), ha.off_tensor(w)
        out = torch.full((len(reads), 4), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        try:
            launch(ctx, p, t_off, len(reads), w["nbytes"], w["max_len"], out)
            ctx.sync()
            d = differing_rows(out.cpu().numpy(), want)
        except rcorrector_amd.RcorrectorError as e:      # (a refusal is one placement's failure: the others still run)
            d = "refused: %s" % e
        if d:
            failures.append("%s: %s" % (where(w, lead), d))
    report(failures)


@pytest.mark.parametrize("k", [23, 5])
def test_read_depth_device(arenas, tables, k):
    run_rows(arenas, tables, k, "depth", lambda ctx, p, off, n, nbytes, ml, out: ctx.read_depth_device(p, off, n, nbytes, ml, out))


@pytest.mark.parametrize("k", [23, 5])
def test_read_screen_device(arenas, tables, k):
    run_rows(arenas, tables, k, "screen",
             lambda ctx, p, off, n, nbytes, ml, out: ctx.read_screen_device(ctx, p, off, n, nbytes, ml, out, min_count=ha.TABLE_MIN_COUNT[k]))


@pytest.mark.parametrize("k", [23, 5])
def test_weak_profile_device(arenas, tables, k):
    run_rows(arenas, tables, k, "weak",
             lambda ctx, p, off, n, nbytes, ml, out: ctx.weak_profile_device(p, off, n, nbytes, ml, out, ha.TABLE_MIN_COUNT[k]))


@pytest.mark.parametrize("k", [23, 5])
def test_trust_profile_device(arenas, tables, k):
    """every mode at every placement"""
    import torch
    reads = ha.table_case()[0]
    ctx, failures = tables[k], []
    for _, w, lead in placements(reads, ha.TABLE_MID):
        p, t_off = ha.put(arenas[0], lead, w), ha.off_tensor(w)
        for mode in (0, 1, 2):
            out = torch.zeros((5, 2, ttp.MAX_LEN), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ctx.trust_profile_device(p, t_off, len(reads), w["nbytes"], w["max_len"], mode, out, ha.TABLE_MIN_COUNT[k])
            ctx.sync()
            got, want = ttp.as_counts(out), table_want("trust", k, mode)
            for f in ttp.FIELDS:
                if not np.array_equal(got[f], want[f]):
                    failures.append("%s mode %d: %s differs in %d entries" % (where(w, lead), mode, f, int((got[f] != want[f]).sum())))
                    break
    report(failures)


# ---- 2. trimming, with the qualities in a second arena of the same size -----------------------------------------------------------
def trim_lists(mode):
    reads, quals, p = ha.trim_case()
    return (ha.halves(reads), ha.halves(quals), ha.TRIM_MID_HALVES, p) if mode == 1 else (reads, quals, ha.TRIM_MID, p)


@functools.lru_cache(maxsize=None)
def trim_want(mode):
    reads, quals, _, p = trim_lists(mode)
    return tm.trim_batch(reads, quals, mode, p)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_read_trim_device(arenas, bare, mode):
    import torch
    reads, quals, mids, p = trim_lists(mode)
    rows, keep, tally = trim_want(mode)
    n, failures = len(reads), []
    units = n if mode == 0 else n // 2
    for _, w, lead in placements(reads, mids):
        ps, pq, t_off = ha.put(arenas[0], lead, w), ha.put(arenas[1], lead, w, quals), ha.off_tensor(w)
        d_out = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
        d_keep = torch.full((units,), 9, dtype=torch.uint8, device="cuda")
        d_tally = torch.zeros(B.TRIM_TALLY_WORDS, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        bare.read_trim_device(ps, pq, t_off, n, w["nbytes"], 1023, mode, params_of(p), d_out, d_keep, d_tally)
        bare.sync()
        d = differing_rows(d_out.cpu().numpy(), rows)
        if not d and not np.array_equal(d_keep.cpu().numpy(), keep):
            d = "keep differs"
        if not d and not tm.tally_equal(B.trim_tally_dict(d_tally.cpu().numpy()), tally):
            d = "the tally differs"
        if d:
            failures.append("%s: %s" % (where(w, lead), d))
    report(failures)


# ---- 3. the mate-overlap report, the bases as read and as corrected in two arenas ----------------------------------------------
@functools.lru_cache(maxsize=None)
def overlap_lists(mode):
    before, after = ha.overlap_case()
    if mode == 1:
        before, after = ha.halves(before), ha.halves(after)
    return before, after, mho.brute(ha.pairs4(before, after, mode), ha.OVERLAP_MIN, 10)


@pytest.mark.parametrize("mode", [1, 2])
def test_mate_overlap_device(arenas, bare, mode):
    import torch
    before, after, want = overlap_lists(mode)
    failures = []
    for _, w, lead in placements(before, ha.TRIM_MID_HALVES if mode == 1 else ha.TRIM_MID):
        lead2 = (lead + 5) % 16                                      # (the two arenas need not share an alignment)
        pb, pa, t_off = ha.put(arenas[0], lead, w), ha.put(arenas[1], lead2, w, after), ha.off_tensor(w)
        counts = torch.zeros(B.OVERLAP_WORDS, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        bare.mate_overlap_device(pb, pa, t_off, len(before), w["nbytes"], 1023, mode, counts, ha.OVERLAP_MIN, 10)
        bare.sync()
        got = B.mate_overlap_dict(counts.cpu().numpy())
        try:
            mho.assert_equal_counts(got, want)
        except AssertionError as e:
            failures.append("%s: %s" % (where(w, lead), str(e).splitlines()[0]))
    report(failures)


# ---- 4. the duplicate census's keys ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_read_keys_device(arenas, bare, dup_key, mode):  # noqa: F811
    import torch
    reads, _, mids, _ = trim_lists(mode)
    want = host_keys(dup_key, reads, mode)
    n, failures = len(reads), []
    units = n if mode == 0 else n // 2
    assert want.shape == (units, 2)
    for _, w, lead in placements(reads, mids):
        p, t_off = ha.put(arenas[0], lead, w), ha.off_tensor(w)
        out = torch.full((units, 2), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        bare.read_keys_device(p, t_off, n, w["nbytes"], mode, out)
        bare.sync()
        d = differing_rows(out.cpu().numpy().view(np.uint64), want)
        if d:
            failures.append("%s: %s" % (where(w, lead), d))
    report(failures)


def test_change_keys_device(arenas, bare):
    """the site keys of the changes between the overlap batch's two versions, the arenas at the same alignment"""
    import torch
    before, after = ha.overlap_case()
    want = rm.Census().add(before, after)
    failures = []
    for _, w, lead in placements(before, ha.TRIM_MID):
        pb, pa, t_off = ha.put(arenas[0], lead, w), ha.put(arenas[1], lead, w, after), ha.off_tensor(w)
        room = want.contexted + 8
        keys = torch.full((room + 4,), -7, dtype=torch.int64, device="cuda")
        counts = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        bare.change_keys_device(pb, pa, t_off, len(before), w["nbytes"], keys, room, counts)
        bare.sync()
        c, k = [int(x) for x in counts.cpu().numpy()], keys.cpu().numpy()
        if c != [want.changes, want.contexted, want.contexted]:
            failures.append("%s: counts %s, want %s" % (where(w, lead), c, [want.changes, want.contexted, want.contexted]))
        elif sorted(int(x) for x in k[:want.contexted].view(np.uint64)) != want.key_list() or k[room:].tolist() != [-7] * 4:
            failures.append("%s: the keys differ" % where(w, lead))
    report(failures)


# ---- 5. the strong threshold and the correction itself, up to the arena's last byte ---------------------------------------------
@functools.lru_cache(maxsize=None)
def correct_want(name):
    from oracle import pyoracle as po
    po.build()
    d = ha.correct_case()[name]
    T = po.Table(d["k"], len(d["keys"]))
    T.put_many(d["keys"], d["counts"])
    P = po.make_params(d["k"], d["mfk"], d["rate"], b"H")
    strong = np.array([po.strong_threshold(P, T, s) for s in d["seqs1"]], dtype=np.int32)
    return strong, datasets.run_oracle(po, d)


@pytest.mark.parametrize("locality", ["default", "force"])
@pytest.mark.parametrize("name", ["plain", "tail"])
def test_strong_threshold_and_correct_device(arenas, name, locality, monkeypatch):
    """`top` with the tail reads behind the data set's, and the data set's reads alone, so that the read that ends at byte
    2^32 - 2 is one of 150 bases; every lead; interleaved pairs.  force: probed in locality order, as a large batch over a large
    table is -- the list-driven probe kernels, which copy read by read (rc_tile_copy_reads)"""
    import torch
    if locality == "force":
        monkeypatch.setenv("RC_LOCALITY", "force")       # (read when the context is made)
    d = ha.correct_case()[name]
    strong, (ret, l, m, h, bases) = correct_want(name)
    reads, n = d["seqs1"], len(d["seqs1"])
    w = ha.top(reads) if name == "tail" else ha.top_plain(reads)
    first, end = int(w["off"][0]), int(w["off"][-1])
    assert np.array_equal(ha.arena_bytes(reads) != 0, bases != 0) and bases.size == end - first
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    ctx.table_build(d["keys"], d["counts"])
    ctx.set_run_params(d["rate"], b"H")
    failures = []
    for lead in ha.TOP_LEADS:
        ps, pq, t_off = ha.put(arenas[0], lead, w), ha.put(arenas[1], lead, w, d["quals1"]), ha.off_tensor(w)
        d_strong = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        res = [torch.full((n,), -77, dtype=torch.int32, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        ctx.strong_threshold_device(ps, t_off, n, w["nbytes"], w["max_len"], d_strong)
        ctx.sync()
        ctx.correct_device(d["mode"], n, w["nbytes"], w["max_len"], ps, pq, t_off, *res)
        ctx.sync()
        got = [d_strong.cpu().numpy()] + [r.cpu().numpy() for r in res] + [arenas[0][lead + first:lead + end].cpu().numpy()]
        for g, want, what in zip(got, (strong, ret, l, m, h, bases), ("strong", "ret", "l", "m", "h", "bases")):
            bad = np.nonzero(g != want)[0]
            if len(bad):
                failures.append("%s: %s differs at %s of %d: got %s, want %s" % (where(w, lead), what, bad[:3], len(want), g[bad[:3]], want[bad[:3]]))
                break
    ctx.close()
    report(failures)


# ---- 6. one filled arena: offsets and read indices large together, and the entry points without offsets ------------------------
def probe_want(reads, k, counts):
    """what rc_probe_device leaves in an arena of int32 preset to -7: the count at the first byte of every k-window of a read"""
    from seam_arena import canonical
    out = []
    for r in reads:
        row = [-7] * (len(r) + 1)
        for i in range(len(r) - k + 1):
            w = r[i:i + k]
            row[i] = counts.get(canonical(w), 0) if set(w) <= set(b"ACGT") else 0
        out += row
    return np.array(out, dtype=np.int32)


def fill(buf, lead, c, strings, tail):
    """the arena at buf + lead: c["tiles"] copies of the base batch made on the device from one copy of the distinct list, then the tail"""
    import torch
    one = torch.from_numpy(ha.arena_bytes(strings).copy()).cuda()
    B, T = c["base_bytes"], c["tiles"]
    assert one.numel() * c["reps"] == B
    buf[lead:lead + T * B].view(T * c["reps"], one.numel()).copy_(one.expand(T * c["reps"], one.numel()))
    t = torch.from_numpy(ha.arena_bytes(tail).copy()).cuda()
    buf[lead + T * B:lead + T * B + t.numel()] = t
    assert T * B + t.numel() == ha.TOP_NBYTES
    buf[lead + ha.TOP_NBYTES:] = ord("A")
    return buf.data_ptr() + lead


def filled_offsets(c):
    """(n, d_off) of a filled arena (ha.filled_case, ha.merge_filled_case): the offsets of every copy of the distinct list and of
    the tail pair, made on the device, as the uint32 bit patterns in an int32 tensor of n + 1"""
    import torch
    T, BB, copies = c["tiles"], c["base_bytes"], c["tiles"] * c["reps"]
    n = copies * len(c["reads"]) + 2
    lens1 = np.array([len(r) + 1 for r in c["reads"]], dtype=np.int64)
    one_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens1)[:-1]])).cuda()
    off = (torch.arange(copies, dtype=torch.int64, device="cuda")[:, None] * int(lens1.sum()) + one_off[None, :]).reshape(-1)
    off = torch.cat([off, torch.tensor([T * BB, T * BB + len(c["tail"][0]) + 1, ha.TOP_NBYTES], dtype=torch.int64, device="cuda")])
    assert off.numel() == n + 1 and int(off[-3]) == T * BB > 0xFFFFF000 and bool((off[1:] > off[:-1]).all())
    t_off = uint32_bits(off)
    assert bool((t_off.to(torch.int64) & 0xFFFFFFFF == off).all())
    return n, t_off


def uint32_bits(x):
    """an int64 tensor of values below 2^32 as their uint32 bit patterns in an int32 tensor"""
    import torch
    return torch.where(x >= 1 << 31, x - (1 << 32), x).to(torch.int32)


def assert_tiled(copies, got, want, tail_want, what):
    """the device tensor `got` is `copies` times the model's `want` of the distinct list, then `tail_want`"""
    import torch
    w = torch.from_numpy(np.ascontiguousarray(want)).cuda()
    body = got[:copies * len(want)].view((copies,) + tuple(w.shape))
    assert torch.equal(body, w.expand_as(body)), "%s: a tile differs from the base batch" % what
    assert np.array_equal(got[copies * len(want):].cpu().numpy(), tail_want), "%s: the tail" % what


def test_one_filled_arena(arenas):
    """nbytes = 2^32 - 1, 27.6 million reads: read_trim_device in mode 2 and read_depth_device at lead 5, every tile's rows equal to
    the base batch's, the tally tiles x the base batch's + the tail's; then, at lead 0, rc_probe_device byte for byte, the counter
    (count_add_device -> table_export) and the recount session (recount_add_device) against tiles x the exact counts"""
    import torch
    from test_read_screen import counts_of_reads
    c = ha.filled_case()
    reads, quals, copies = c["reads"], c["quals"], c["tiles"] * c["reps"]
    n, t_off = filled_offsets(c)
    p = tm.params()
    rows, keep, tally = tm.trim_batch(reads, quals, 2, p)
    t_rows, t_keep, t_tally = tm.trim_batch(c["tail"], c["tail_quals"], 2, p)
    assert tally["pairs_overlapping"] > 20 and (tally["cut_reads"] > 5).all() and 0 < tally["units_kept"] < tally["units"]
    counts = counts_of_reads(reads, 23)
    depth = depth_rows(reads, 23, counts)
    assert (depth[:, 0] > 0).sum() > 80 and depth[-1].tolist() == [0, 0, 0, 0]
    ctx = rcorrector_amd.Context(k=23, device=0)
    table_of(ctx, counts)

    def tiled(got, want, tail_want, what):
        assert_tiled(copies, got, want, tail_want, what)

    # trim and depth, the arena 5 bytes behind a 16-byte boundary
    ps, pq = fill(arenas[0], 5, c, reads, c["tail"]), fill(arenas[1], 5, c, quals, c["tail_quals"])
    d_out = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
    d_keep = torch.full((n // 2,), 9, dtype=torch.uint8, device="cuda")
    d_tally = torch.zeros(B_TALLY, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.read_trim_device(ps, pq, t_off, n, ha.TOP_NBYTES, 1023, 2, params_of(p), d_out, d_keep, d_tally)
    ctx.sync()
    tiled(d_out, rows, t_rows, "trim rows")
    tiled(d_keep, keep, t_keep, "trim keep")
    got = B.trim_tally_dict(d_tally.cpu().numpy())
    for f in tm.empty_tally():
        want = np.asarray(tally[f], np.uint64) * np.uint64(copies) + np.asarray(t_tally[f], np.uint64)
        assert np.array_equal(np.asarray(got[f], np.uint64), want), "trim tally %s" % f
    d_out.fill_(-7)
    torch.cuda.synchronize()
    ctx.read_depth_device(ps, t_off, n, ha.TOP_NBYTES, 1023, d_out)
    ctx.sync()
    tiled(d_out, depth, np.zeros((2, 4), np.int32), "depth rows")
    del d_out, d_keep

    # the entry points without offsets, the arena on a 16-byte boundary
    ps = fill(arenas[0], 0, c, reads, c["tail"])
    d_cnt = torch.full((ha.TOP_NBYTES,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.probe_device(ps, ha.TOP_NBYTES, d_cnt)
    ctx.sync()
    tiled(d_cnt, probe_want(reads, 23, counts), probe_want(c["tail"], 23, counts), "probe counts")
    del d_cnt
    total, top_count = sum(counts.values()), max(counts.values())
    ctx.recount_begin(10000)
    ctx.recount_add_device(ps, ha.TOP_NBYTES)
    freq, st = ctx.recount_finish()
    assert (st["distinct"], st["total"], st["max_count"], st["absent_distinct"], st["absent_total"]) == (len(counts), total * copies, top_count * copies, 0, 0)
    assert int(freq[-1]) == len(counts) and int(freq.sum()) == len(counts)
    ctx.close()
    counter = rcorrector_amd.Context(k=23, device=0)
    counter.count_begin()
    counter.count_add_device(ps, ha.TOP_NBYTES)
    assert counter.count_finish(1) == len(counts)
    codes, cnt = counter.table_export()
    order = np.argsort(codes)
    want_codes = np.array(sorted(counts), dtype=np.uint64)
    assert np.array_equal(codes[order], want_codes)
    assert np.array_equal(cnt[order].astype(np.int64), np.array([counts[int(x)] for x in want_codes], dtype=np.int64) * copies)
    counter.close()


# ---- 7. merging: the one entry point that writes an arena and an offset array, so the offsets are large on the way out too -------
ARENA_ALLOC = (ha.TOP_NBYTES + 16 + 15) // 16 * 16          # what ha.allocate() takes
MERGE_GUARD = 4096                                          # bytes behind d_moff[units] that must stay poison


def merge_need_free():
    """device bytes test_one_filled_arena_merged takes at its peak: the four arenas; per read the offsets (int32, and the int64
    ones with two temporaries while they are made); per unit the merge's rows, d_moff and the library's scratch lengths, the
    hand-off's rows and keep flags, and the expected d_moff (int64, with a temporary); and one byte for every output byte looked
    at in one comparison, which is at most an arena"""
    c = ha.merge_filled_case()
    n = c["tiles"] * c["reps"] * len(c["reads"]) + 2
    return 4 * ARENA_ALLOC + n * (4 + 3 * 8) + (n // 2) * (16 + 4 + 4 + 16 + 1 + 2 * 8) + ARENA_ALLOC


@pytest.fixture(scope="module")
def merged_arenas(arenas):
    """two more 4 GiB allocations: the merged sequences and the merged qualities (out_cap is at least nbytes)"""
    import torch
    torch.cuda.empty_cache()
    free, need = torch.cuda.mem_get_info()[0], merge_need_free() - sum(a.numel() for a in arenas)       # (the input arenas are there already)
    if free < need:
        pytest.skip("%.1f GiB of device memory are free, the merged arenas above 2 GiB need %.1f more" % (free / 2.0 ** 30, need / 2.0 ** 30))
    bufs = [ha.allocate(), ha.allocate()]
    yield bufs
    del bufs[:]
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def merge_runs(mode):
    """[(reads, quals, the windows with their leads, merge_model's results)]: mode 2 as trimming runs; mode 1 through halves()
    as trimming runs, and through split() -- every pair a pair again, so the expected results are mode 2's -- up to the arena's last byte"""
    reads, quals, p = ha.merge_case()
    if mode == 2:
        return [(reads, quals, ha.windows(reads, ha.TRIM_MID), mm.merge_batch(reads, quals, 2, p))]
    h, hq, s, sq = ha.halves(reads), ha.halves(quals), ha.split(reads), ha.split(quals)
    return [(h, hq, ha.windows(h, ha.TRIM_MID_HALVES), mm.merge_batch(h, hq, 1, p)),
            (s, sq, [(ha.top_plain(s), ha.TOP_LEADS)], mm.merge_batch(s, sq, 1, p))]


@pytest.mark.parametrize("mode", [1, 2])
def test_read_merge_device(arenas, merged_arenas, bare, mode):
    """sequences and qualities at the same lead, d_mqual asked for, out_cap = nbytes; the rows, d_moff, both merged arenas and the
    tally equal the model, and the 4096 bytes behind d_moff[units] are still poison"""
    import torch
    p = ha.merge_case()[2]
    failures = []
    for reads, quals, wins, want in merge_runs(mode):
        n, units = len(reads), len(reads) // 2
        total = int(want[1][units])
        for w, leads in wins:
            for lead in leads:
                ps, pq, t_off = ha.put(arenas[0], lead, w), ha.put(arenas[1], lead, w, quals), ha.off_tensor(w)
                for o in merged_arenas:
                    o[:total + MERGE_GUARD] = POISON
                rows = torch.full((units, 4), -7, dtype=torch.int32, device="cuda")
                moff = torch.full((units + 2,), -7, dtype=torch.int32, device="cuda")
                tal = torch.zeros(B.MERGE_TALLY_WORDS, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                try:
                    bare.read_merge_device(ps, pq, t_off, n, w["nbytes"], 1023, mode, merge_params_of(p), rows, merged_arenas[0], merged_arenas[1], moff,
                                           w["nbytes"], tal)
                    bare.sync()
                    m = moff.cpu().numpy()
                    got = {"rows": rows.cpu().numpy(), "moff": m.view(np.uint32)[:units + 1], "tally": B.merge_tally_dict(tal.cpu().numpy()),
                           "mseq": merged_arenas[0][:total].cpu().numpy().tobytes(), "mqual": merged_arenas[1][:total].cpu().numpy().tobytes()}
                    assert m[units + 1] == -7, "d_moff has units + 1 entries"
                    assert_merge_equal(got, want)
                    for o, what in zip(merged_arenas, ("mseq", "mqual")):
                        assert bool((o[total:total + MERGE_GUARD] == POISON).all()), "%s: a byte behind d_moff[units] = %d was written" % (what, total)
                except (AssertionError, rcorrector_amd.RcorrectorError) as e:      # (a refusal is one placement's failure: the others still run)
                    failures.append("%s: %s" % (where(w, lead), (str(e) or repr(e)).splitlines()[0]))
    report(failures)


def test_one_filled_arena_merged(arenas, merged_arenas, bare):
    """nbytes = 2^32 - 1, 21.8 million reads in interleaved pairs with qualities at lead 5, most of which merge: the merged arenas
    take 2.66 GiB, so d_moff passes 2^31 and every copy of the distinct list lands on another alignment modulo 16.  Every copy's
    rows, d_moff (as uint32 bit patterns) and merged bytes equal merge_model's of the distinct list, the tally is copies x the
    list's + the tail pair's, every byte at or behind d_moff[units] is still poison.  Then the merged arenas, as they lie in HBM,
    go to read_trim_device in mode 0: d_moff above 2^31 as an input offset array.
    Measured on an MI355X in one session: d_moff[units] = 2 859 060 727; 0.19 s for this test's call (and 1.3 s to set up its
    fixture: the model on the distinct list, two allocations) against 3.09 s for test_one_filled_arena's call, so nothing of it
    had to be dropped."""
    import torch
    c = ha.merge_filled_case()
    reads, quals = c["reads"], c["quals"]
    copies, ndu = c["tiles"] * c["reps"], len(reads) // 2
    rows, moff, mseq, mqual, tally = c["want"]
    t_rows, t_moff, t_mseq, t_mqual, t_tally = c["tail_want"]
    per = int(moff[ndu])
    assert per * c["reps"] == c["base_out"] and t_mseq == t_mqual == b"\0"
    total = copies * per + 1
    n, t_off = filled_offsets(c)
    units = n // 2
    assert units == copies * ndu + 1
    ps, pq = fill(arenas[0], 5, c, reads, c["tail"]), fill(arenas[1], 5, c, quals, c["tail_quals"])
    for o in merged_arenas:
        o.fill_(POISON)
    d_rows = torch.full((units, 4), -7, dtype=torch.int32, device="cuda")
    d_moff = torch.full((units + 1,), -7, dtype=torch.int32, device="cuda")
    d_tally = torch.zeros(B.MERGE_TALLY_WORDS, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bare.read_merge_device(ps, pq, t_off, n, ha.TOP_NBYTES, 1023, 2, merge_params_of(c["params"]), d_rows, merged_arenas[0], merged_arenas[1], d_moff,
                           ha.TOP_NBYTES, d_tally)
    bare.sync()
    del t_off
    got_total = int(d_moff[units].item()) & 0xFFFFFFFF
    print("d_moff[units] = %d" % got_total)
    assert got_total > (1 << 31) + (1 << 29), "the merged arena does not reach 2^31 + 2^29: d_moff[units] = %d" % got_total
    assert_tiled(copies, d_rows, rows, t_rows, "merge rows")
    want_moff = (torch.arange(copies, dtype=torch.int64, device="cuda")[:, None] * per + torch.from_numpy(moff[:ndu].astype(np.int64)).cuda()[None, :]).reshape(-1)
    want_moff = uint32_bits(torch.cat([want_moff, torch.tensor([copies * per, total], dtype=torch.int64, device="cuda")]))
    bad = torch.nonzero(d_moff != want_moff)
    assert bad.numel() == 0, "d_moff differs at %d units, first at unit %d" % (bad.numel(), int(bad[0]))
    del want_moff, bad
    assert got_total == total
    for o, base, what in zip(merged_arenas, (mseq, mqual), ("mseq", "mqual")):
        w = torch.from_numpy(np.frombuffer(base, dtype=np.uint8).copy()).cuda()
        body = o[:copies * per].view(copies, per)
        assert torch.equal(body, w.expand_as(body)), "%s: a copy's merged bytes differ from the distinct list's" % what
        assert int(o[total - 1]) == 0, "%s: the tail pair's NUL" % what
        assert bool((o[total:] == POISON).all()), "%s: a byte at or behind d_moff[units] = %d was written" % (what, total)
    got = B.merge_tally_dict(d_tally.cpu().numpy())
    for f in mm.TALLY_KEYS:
        want = np.asarray(tally[f], np.uint64) * np.uint64(copies) + np.asarray(t_tally[f], np.uint64)
        assert np.array_equal(np.asarray(got[f], np.uint64), want), "merge tally %s" % f
    del d_rows

    # the hand-off: the merged reads as single reads, where the merge left them
    p = tm.params()
    strings = [mseq[moff[u]:moff[u + 1] - 1] for u in range(ndu)]
    qstrings = [mqual[moff[u]:moff[u + 1] - 1] for u in range(ndu)]
    assert max(len(s) for s in strings) <= 1023 and all(len(s) == r[0] for s, r in zip(strings, rows))
    h_rows, h_keep, h_tally = tm.trim_batch(strings, qstrings, 0, p)
    ht_rows, ht_keep, ht_tally = tm.trim_batch([b""], [b""], 0, p)
    assert (h_rows[:, 0] < rows[:, 0]).sum() > 3 and 0 < h_tally["units_kept"] < h_tally["units"]       # (some merged reads are cut, some units are short)
    d_out = torch.full((units, 4), -7, dtype=torch.int32, device="cuda")
    d_keep = torch.full((units,), 9, dtype=torch.uint8, device="cuda")
    d_tally = torch.zeros(B_TALLY, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bare.read_trim_device(merged_arenas[0], merged_arenas[1], d_moff, units, total, 1023, 0, params_of(p), d_out, d_keep, d_tally)
    bare.sync()
    assert_tiled(copies, d_out, h_rows, ht_rows, "hand-off: trim rows")
    assert_tiled(copies, d_keep, h_keep, ht_keep, "hand-off: trim keep")
    got = B.trim_tally_dict(d_tally.cpu().numpy())
    for f in tm.empty_tally():
        want = np.asarray(h_tally[f], np.uint64) * np.uint64(copies) + np.asarray(ht_tally[f], np.uint64)
        assert np.array_equal(np.asarray(got[f], np.uint64), want), "hand-off: trim tally %s" % f
