"""CPU: tests/merge_model.py, the model every merging test compares with, on pairs small enough to merge by hand -- the merged
strings are spelled out here -- and its offset against tests/trim_model.py: the pair cut of mate 1 is min(La, F)."""
import numpy as np

import merge_model as mm
import trim_cases as tc
import trim_model as tm

# a fragment of 10 bases read 7 deep from both ends: a = ACGTTGC, r = TTGCAAG (b = CTTGCAA), d* = 3, positions 3 .. 6 faced
A, B = b"ACGTTGC", b"CTTGCAA"
P4 = mm.params(min_overlap=4, max_mismatch_pct=25)


def q(*phred):
    return bytes(33 + x for x in phred)


def test_agreement_adds_the_phred_values_up_to_the_cap():
    qa = q(40, 40, 40, 40, 10, 20, 40)
    qr = q(2, 10, 20, 40, 40, 40, 40)          # of r: position p of the merged read faces qr[p - 3]
    row, s, ql, took = mm.merge_pair(A, B, qa, qr[::-1], P4)
    assert row == (10, 3, 4, 0) and s == b"ACGTTGCAAG" and took == (0, 0, 0)
    #              a alone          40+2 -> 41   10+10   20+20   40+40 -> 41   r alone
    assert ql == q(40, 40, 40) + q(41, 20, 40, 41) + q(40, 40, 40)
    assert mm.merge_pair(A, B, qa, qr[::-1], mm.params(min_overlap=4, qual_cap=93))[2][3:7] == q(42, 20, 40, 80)
    assert mm.merge_pair(A, B, qa, qr[::-1], mm.params(min_overlap=5))[0] == (0, 0, 0, 0)          # four faced bases are too few


def test_disagreement_goes_to_the_better_quality_and_a_tie_to_mate_1():
    a = b"ACGTTTC"                              # position 5: T against r's G
    for pa, pr, base, qual, took in ((20, 10, b"T", 10, (1, 0, 0)), (10, 20, b"G", 10, (0, 1, 0)), (20, 20, b"T", 2, (0, 0, 1)), (20, 21, b"G", 2, (0, 1, 0)),
                                     (0, 60, b"G", 41, (0, 1, 0)), (23, 20, b"T", 3, (1, 0, 0))):
        qa = q(40, 40, 40, 40, 40, pa, 40)
        qr = q(40, 40, pr, 40, 40, 40, 40)
        row, s, ql, tk = mm.merge_pair(a, B, qa, qr[::-1], P4)
        assert row == (10, 3, 4, 1) and s == b"ACGTT" + base + b"CAAG" and ql[5] == 33 + qual and tk == took, (pa, pr)
    # a quality byte below qual_base is phred 0: '!' (33) against base 40 is 0, as is 40 itself -- a tie
    row, s, ql, tk = mm.merge_pair(a, B, b"IIIII!I", b"IIII(II", mm.params(min_overlap=4, max_mismatch_pct=25, qual_base=40))
    assert s[5:6] == b"T" and ql[5] == 42 and tk == (0, 0, 1)
    # without qualities mate 1's base stays and nothing is made for the qualities
    row, s, ql, tk = mm.merge_pair(a, B, None, None, P4)
    assert row == (10, 3, 4, 1) and s == b"ACGTTTCAAG" and ql is None and tk == (0, 0, 1)
    # one disagreement of four is 25 %: not accepted at 24
    assert mm.merge_pair(a, B, None, None, mm.params(min_overlap=4, max_mismatch_pct=24))[0] == (0, 0, 0, 0)


def test_bytes_that_are_no_base_are_never_compared_and_go_through_verbatim():
    p3 = mm.params(min_overlap=3, max_mismatch_pct=0)
    # N against a base: the base and ITS quality; a base against n: the base of mate 1; N against N: mate 1's two bytes
    row, s, ql, tk = mm.merge_pair(b"ACGNTGC", B, b"ABCDEFG", b"7654321", p3)
    assert row == (10, 3, 3, 0) and s == b"ACGTTGCAAG" and ql == b"ABC1" + q(41, 41, 41) + b"567" and 36 + 17 > 41
    row, s, ql, tk = mm.merge_pair(A, b"CTTGCAn", b"ABCDEFG", b"7654321", p3)       # r = nTGCAAG: the lower-case n stays n where r is alone
    assert row == (10, 3, 3, 0) and s == b"ACGTTGCAAG" and ql[3:4] == b"D"
    row, s, ql, tk = mm.merge_pair(b"ACGNTGC", b"CTTGCAN", b"ABCDEFG", b"7654321", p3)
    assert s == b"ACGNTGCAAG" and ql[3:4] == b"D"
    # lower case is no base, and mate 2's lower case is complemented in case
    row, s, ql, tk = mm.merge_pair(b"ACGTTGCA", b"cTTGCAAC", None, None, p3)         # r = GTTGCAAg
    assert row == (10, 2, 6, 0) and s == b"ACGTTGCAAg"
    assert [mm.comp(x) for x in b"ACGTacgtNn-"] == list(b"TGCAtgcaNn-")


def test_read_through_is_dropped_on_both_sides():
    # a fragment of 6 bases, CCGGTA, read 9 deep: mate 1 runs 3 bases into the adapter (TTT), mate 2 likewise
    frag = b"CCGGTA"
    a, b = frag + b"TTT", tc.revcomp(frag) + b"GGG"
    row, s, ql, tk = mm.merge_pair(a, b, b"I" * 9, b"5" * 9, mm.params(min_overlap=6, max_mismatch_pct=0, qual_cap=93))
    assert row == (6, -3, 6, 0) and s == frag and ql == q(*([60] * 6))
    rows, moff, mseq, mqual, t = mm.merge_batch([a, b, b"ACGT", b"ACGT"], [b"I" * 9, b"5" * 9, b"IIII", b"IIII"], 2, mm.params(min_overlap=6, qual_cap=93))
    assert rows.tolist() == [[6, -3, 6, 0], [0, 0, 0, 0]] and moff.tolist() == [0, 7, 8] and mseq == frag + b"\0\0" and mqual == q(*([60] * 6)) + b"\0\0"
    assert (t["pairs"], t["merged"], t["unmerged"], t["readthrough"], t["compared"]) == (2, 1, 1, 1, 6) and t["len_hist"][6] == 1 == t["len_hist"][0]


def test_the_offset_is_the_pair_cut_of_the_trimming_model():
    rng = np.random.default_rng(11)
    p = mm.params()
    tp = tm.params(qual_min=0, adapter1=b"", min_len=0)
    seen = set()
    for n in range(150):
        La, Lb = (int(x) for x in rng.integers(30, 90, 2))
        F = int(rng.integers(20, 150))
        a, b = tc.pair_of(rng, F, La, Lb, tail=b"")
        a, b = a + tc.rand_seq(rng, La - len(a)), b + tc.rand_seq(rng, Lb - len(b))
        row, s, _, _ = mm.merge_pair(a, b, None, None, p)
        trows, _, ovl = tm.trim_unit([a, b], None, tp)
        assert ovl == (row[0] > 0)
        if ovl:
            assert trows[0][3] == min(La, row[0]) and trows[1][3] == min(Lb, Lb + row[1]) and row[0] == F and len(s) == F
            seen.add((row[1] < 0, F < La))
            assert s[:min(La, F)] == a[:min(La, F)] and tc.revcomp(s)[:min(Lb, F)] == b[:min(Lb, F)]       # (no disagreements: both mates read it)
        else:
            seen.add("unmerged")
    assert seen == {(True, True), (True, False), (False, True), (False, False), "unmerged"}
