"""CPU: the inputs of tests/test_high_arena.py hold what they are there for, by the references alone -- so the GPU tests cannot
pass on empty results, and the offsets reach where a 32-bit position wraps.

Two statements of the plan cannot hold as written and are asked for as far as they can: no read starts at 2^32 - 1 (the arena's
last byte is 2^32 - 2), so a read's *start* wraps for lead 2..15 only, while a read's end reaches 2^32 - 4 at every lead; and a
read whose every window is solid has the weak row of an empty read, (0, 0, 0, 0): the read of exactly k bases, whose one window must
be solid, is pinned by its depth and screen rows, and every other of the last four reads has a solid and a weak window.

A third, of the merge's plan: halves() makes pairs of the first twelve pairs only -- in mode 1 it gives the tail reads other mates,
so the pair of 1022 and 150 bases and the pair of 16 and 15 are pairs in mode 2 alone, and the two modes cannot give the same merged
arena through it.  They do through split() (all first mates, then all second mates), which the GPU test runs in mode 1 as well, up to
the arena's last byte; through halves() the modes agree on the twelve pairs, and at least 9 units merge in either."""
import numpy as np

import high_arena as ha
import merge_model as mm
import trim_model as tm
from test_mate_overlap_host import brute
from test_read_depth import restate_all as depth_rows
from test_read_screen import restate_all as screen_rows
from test_weak_profile import restate_all as weak_rows


def test_the_last_four_reads_of_k_bases_have_solid_and_valid_windows():
    reads, counts = ha.table_case()
    for k in (23, 5):
        last = [r for r in reads if len(r) >= k][-4:]
        assert last == [r for r in reads[-len(ha.TAIL_LENGTHS) - 1:] if len(r) >= k][-4:]      # (they are tail reads, or the read in front)
        mc = ha.TABLE_MIN_COUNT[k]
        depth, screen, weak = depth_rows(last, k, counts[k]), screen_rows(last, k, counts[k], mc), weak_rows(last, k, counts[k], mc)
        assert (depth[:, 0] >= 1).all() and (depth[:, 2] > 0).all(), (k, depth)
        assert (screen[:, 1] >= 1).all() and (screen_rows(last, k, counts[k], 1)[:, 1] >= 1).all(), (k, screen)
        several = np.array([len(r) > k for r in last])       # (a read of k bases has one window: solid, its weak row is the empty read's)
        assert weak[several].any(axis=1).all() and several.sum() >= 3, (k, weak)
        assert ((screen[several, 1] >= 1) & (screen[several, 1] < screen[several, 0])).all(), (k, screen)      # a solid and a weak window each
    # the reads of 5 to 14 bases that begin in the last 15 bytes have windows at k = 5 only
    w = ha.top(reads)
    late = [i for i in range(len(reads)) if w["off"][i] >= ha.TOP_NBYTES - 15]
    assert {len(reads[i]) for i in late} == {0, 1, 3, 5} and depth_rows([reads[i] for i in late], 5, counts[5])[:, 0].tolist() == [1, 0, 0, 0]


def test_every_cut_fires_near_the_end_and_the_straddling_pair_overlaps():
    reads, quals, p = ha.trim_case()
    rows, keep, tally = tm.trim_batch(reads, quals, 2, p)
    L = np.array([len(r) for r in reads[-8:]])
    assert L.tolist() == list(ha.TAIL_LENGTHS[-8:])
    for c in (1, 2, 3):
        assert (rows[-8:, c] < L).any(), "cut %d fires on none of the last eight reads" % c
    assert 0 < tally["units_kept"] < tally["units"]
    for kind, i in ha.TRIM_MID:
        a, b = reads[i & ~1], reads[i | 1]
        assert tm.pair_offset(a, b, p["pair_min_overlap"], p["pair_mm_pct"]) is not None
    assert {i & 1 for kind, i in ha.TRIM_MID if kind == "straddle"} == {0, 1}       # the straddling read is once mate 1, once mate 2
    before, after = ha.overlap_case()
    assert ha.pairs4(ha.halves(before), ha.halves(after), 1)[:12] == ha.pairs4(before, after, 2)[:12]
    assert [ha.halves(reads)[i] for kind, i in ha.TRIM_MID_HALVES] == [reads[i] for kind, i in ha.TRIM_MID] and ha.halves(reads)[-12:] == reads[-12:]
    for mode in (1, 2):
        c = brute(ha.pairs4(ha.halves(before), ha.halves(after), 1) if mode == 1 else ha.pairs4(before, after, 2), ha.OVERLAP_MIN, 10)
        assert c["overlapping"] >= 8 and c["disagree_after"] != c["disagree_before"]
    assert brute(ha.pairs4(before, after, 2)[3:4], ha.OVERLAP_MIN, 10)["overlapping"] == 1      # reads 6 and 7, the straddling pair
    assert brute(ha.pairs4(before, after, 2)[-4:-3], ha.OVERLAP_MIN, 10)["overlapping"] == 1    # the pair of 16 and 15 bases


def test_the_offsets_reach_where_a_32_bit_position_wraps():
    for reads in (ha.table_case()[0], ha.trim_case()[0]):
        w = ha.top(reads)
        off = w["off"]
        assert off[-1] == ha.TOP_NBYTES == (1 << 32) - 1 and len(reads[-1]) == 0 and off[-2] == (1 << 32) - 2
        for lead in range(1, 16):
            if lead >= 2:
                assert (off[:-1] + lead >= 1 << 32).any(), lead                  # a read's start, counted from the 16-byte boundary
            assert (off[1:] - 1 + lead >= (1 << 32) - 4).any(), lead             # a read's last byte
        assert (off[1:] - 1 >= (1 << 32) - 4).any()                                # ... and at lead 0, for the kernels that take the arena as it is
        assert sum(off[i] >= ha.TOP_NBYTES - 15 for i in range(len(reads))) >= 4 and off[-12] >= ha.TOP_NBYTES - 512     # (the full-length read ends there)


def test_offsets_above_2_31_are_negative_as_int32():
    for reads, mids in ((ha.table_case()[0], ha.TABLE_MID), (ha.trim_case()[0], ha.TRIM_MID), (ha.halves(ha.trim_case()[0]), ha.TRIM_MID_HALVES)):
        for w, leads in ha.windows(reads, mids):
            bits, off = ha.off_bits(w), w["off"]
            assert bits.dtype == np.int32 and np.array_equal(bits < 0, off >= ha.HALF) and (bits < 0).any()
            assert np.array_equal(bits.view(np.uint32).astype(np.int64), off)
            if w["name"] == "top":
                assert (bits < 0).all() and leads == tuple(range(16))
            else:
                assert (bits >= 0).any() and leads == (0, 5, 15) and w["nbytes"] == (1 << 31) + 65536
                assert (ha.HALF in off.tolist()) == (w["name"] == "mid seam")


def test_the_correction_batches_end_in_a_read_the_oracle_has_something_to_say_about():
    from oracle import pyoracle as po
    import datasets
    po.build()
    for name, d in ha.correct_case().items():
        ret, l, m, h = datasets.run_oracle(po, d)[:4]
        n = len(d["seqs1"])
        assert n % 2 == 0 and len(ret) == n and (ret > 0).sum() > n // 10
        if name == "plain":
            assert len(d["seqs1"][-1]) == 150 and h[-1] > 0 and ha.top_plain(d["seqs1"])["off"][-1] == ha.TOP_NBYTES
            assert (ret[-8:] > 0).any()                                   # a read among the last eight is corrected
        else:
            assert ha.top(d["seqs1"])["max_len"] == 1022


def test_the_change_keys_batch_has_contexted_and_clipped_changes():
    import recur_model as rm
    before, after = ha.overlap_case()
    c = rm.Census().add(before, after)
    assert c.contexted >= 5 and c.changes > c.contexted


def test_the_filled_arena_is_full_to_the_last_byte_and_its_tiles_shift_alignment():
    c = ha.filled_case()
    per_copy = sum(len(r) + 1 for r in c["reads"])
    assert per_copy * c["reps"] == c["base_bytes"] and c["base_bytes"] % 2 == 1 and abs(c["base_bytes"] - (1 << 20)) < 1 << 17
    assert c["tiles"] * c["base_bytes"] + sum(len(t) + 1 for t in c["tail"]) == (1 << 32) - 1
    assert len({(t * c["base_bytes"]) % 16 for t in range(16)}) == 16 and len(c["reads"]) % 2 == 0 and len(c["tail"]) == 2
    lens = [len(r) for r in c["reads"]]
    assert set(ha.TAIL_LENGTHS) <= set(lens) and min(lens[:80]) == 37 and max(lens[:80]) == 250 and max(len(t) for t in c["tail"]) <= 1023
    assert c["tiles"] * c["reps"] * len(c["reads"]) > 1 << 24                  # read indices and offsets are large together
    assert len(c["quals"]) == len(c["reads"]) and all(len(q) == len(r) for q, r in zip(c["quals"], c["reads"]))


def test_the_merge_batch_merges_in_both_modes_and_its_last_pairs_hit_the_edges():
    reads, quals, p = ha.merge_case()
    assert (reads, quals) == ha.trim_case()[:2] and p == mm.params(min_overlap=12)
    two = mm.merge_batch(reads, quals, 2, p)
    rows, moff, mseq, mqual, t = two
    print("merge_case, mode 2: %d of %d units merge, %d read-through, %d merged bytes" % (t["merged"], t["pairs"], t["readthrough"], moff[-1]))
    assert t["merged"] >= 9 and len(mqual) == len(mseq) == moff[-1]
    assert [len(r) for r in reads[-12:-10]] == [1022, 150] and rows[-6, 0] == 1100 > 1023                      # the wide instance
    assert [len(r) for r in reads[-8:-6]] == [16, 15] and rows[-4].tolist()[:2] == [13, -2] and rows[-4, 0] < 16      # a read-through: F < La, d < 0
    assert [len(r) for r in reads[-2:]] == [1, 0] and rows[-1].tolist() == [0, 0, 0, 0] and moff[-1] - moff[-2] == 1
    # mode 1, every pair a pair again (split): the same merged arena, d_moff, rows and tally
    one = mm.merge_batch(ha.split(reads), ha.split(quals), 1, p)
    assert one[2] == two[2] and one[3] == two[3] and np.array_equal(one[1], two[1]) and np.array_equal(one[0], two[0]) and mm.tally_equal(one[4], two[4])
    assert ha.split(reads)[-1] == b"" and [len(r) for r in ha.split(reads)[-6:]] == list(ha.TAIL_LENGTHS[1::2])
    # mode 1 through halves(): the twelve pairs of "pair offsets" are pairs again, with the same rows and merged bytes
    h = mm.merge_batch(ha.halves(reads), ha.halves(quals), 1, p)
    print("merge_case, mode 1 through halves(): %d of %d units merge, %d read-through" % (h[4]["merged"], h[4]["pairs"], h[4]["readthrough"]))
    assert np.array_equal(h[0][:12], rows[:12]) and np.array_equal(h[1][:13], moff[:13]) and h[2][:moff[12]] == mseq[:moff[12]] and h[3][:moff[12]] == mqual[:moff[12]]
    assert h[4]["merged"] >= 9 and h[0][-1].tolist() == [0, 0, 0, 0]


def test_the_merged_filled_arena_crosses_2_31_and_its_copies_shift_alignment():
    c = ha.merge_filled_case()
    rows, moff, mseq, mqual, t = c["want"]
    copies, units = c["tiles"] * c["reps"], len(c["reads"]) // 2
    total = copies * int(moff[-1]) + int(c["tail_want"][1][-1])            # the tiled d_moff[units]
    print("merge_filled_case: %d of %d units merge, %d read-through, %d unmerged; %d output bytes of %d; mismatches %d, mate 1 %d, mate 2 %d; d_moff[units] = %d"
          % (t["merged"], units, t["readthrough"], t["unmerged"], moff[-1], c["base_bytes"] // c["reps"], t["mismatches"], t["took_mate1"], t["took_mate2"], total))
    assert (1 << 31) + (1 << 29) <= total <= (1 << 32) - 1
    assert t["merged"] >= 30 and t["readthrough"] >= 4 and t["unmerged"] >= 3 and t["pairs"] == units == len(rows)
    assert t["mismatches"] > 0 and t["took_mate1"] > 0 and t["took_mate2"] > 0
    assert set((moff % 16).tolist()) == set(range(16))
    assert c["base_bytes"] % 2 == 1 and c["base_out"] % 2 == 1 and c["base_out"] == c["reps"] * int(moff[-1])
    assert len({(i * c["base_out"]) % 16 for i in range(16)}) == 16 == len({(i * int(moff[-1])) % 16 for i in range(16)})
    # shaped as filled_case is
    assert sum(len(r) + 1 for r in c["reads"]) * c["reps"] == c["base_bytes"] and abs(c["base_bytes"] - (1 << 20)) < 1 << 17
    assert c["tiles"] * c["base_bytes"] + sum(len(x) + 1 for x in c["tail"]) == (1 << 32) - 1 and len(c["tail"]) == 2
    lens = [len(r) for r in c["reads"]]
    assert min(lens[:80]) >= 150 and max(lens[:80]) <= 250 and tuple(lens[80:92]) == ha.TAIL_LENGTHS and len(lens) == 94
    assert all(len(q) == len(r) for q, r in zip(c["quals"], c["reads"])) and c["reads"] != ha.filled_case()["reads"]
    assert c["tail_want"][0].tolist() == [[0, 0, 0, 0]] and c["tail_want"][2] == b"\0"
