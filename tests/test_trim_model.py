"""CPU: tests/trim_model.py -- the trimming contract of include/rcorrector_amd.h restated in plain Python, what the kernel, the
host program and the tool are compared with -- on hand-written cases whose answers are written out here."""
import numpy as np

import trim_model as tm

AD = b"AGATCGGAAGAGC"


def q(*vals):
    return bytes(33 + v for v in vals)


def test_quality_cut_by_hand():
    # threshold 20: t = 20 - Q.  Q = 30 30 30 10 10: t = -10 -10 -10 10 10, S = -10 0 10 20 10 (0); i0 = 0, the maximum 20 at i = 3
    assert tm.cut_quality(q(30, 30, 30, 10, 10), 5, 20) == 3
    assert tm.cut_quality(q(30, 30, 30, 30), 4, 20) == 4                      # all high: S < 0 everywhere, S(L) = 0 is the maximum
    assert tm.cut_quality(q(2, 2, 2), 3, 20) == 0                             # all low: S grows to the front
    # bad head, good middle, bad tail: S = (18 - 40 + 18, -22, -40 + 18 ..): the stop at the middle keeps the head
    assert tm.cut_quality(q(2, 40, 40, 2), 4, 20) == 3
    assert tm.cut_quality(q(2, 2, 40, 2, 2, 2), 6, 20) == 0                   # the tail outweighs the middle: S never negative, the head goes too
    assert tm.cut_quality(q(40, 20, 20), 3, 20) == 3                          # ties in S (0 at 1, 2 and 3): the larger i
    assert tm.cut_quality(q(40, 19, 21, 19, 21), 5, 20) == 5                  # S = -20 0 -1 0 -1 (0): i0 = 4, so only L is behind it
    assert tm.cut_quality(q(40, 19, 21, 19), 4, 20) == 3                      # S = -19 1 0 1 (0): the maximum 1 at i = 1 and 3
    assert tm.cut_quality(q(2, 2), 2, 0) == 2 and tm.cut_quality(None, 7, 20) == 7 and tm.cut_quality(b"", 0, 20) == 0
    assert tm.cut_quality(bytes([64 + 2, 64 + 40, 64 + 2]), 3, 20, 64) == 2   # phred 64


def test_adapter_cut_by_hand():
    assert tm.cut_adapter(AD + b"TTTT", AD, 5, 10) == 0
    assert tm.cut_adapter(b"TTTTTTTT" + AD[:5], AD, 5, 10) == 8               # v = 5 = adapter_min
    assert tm.cut_adapter(b"TTTTTTTT" + AD[:4], AD, 5, 10) == 12              # v = 4: not accepted anywhere
    assert tm.cut_adapter(b"TTTT" + AD + b"TT" + AD, AD, 5, 10) == 4          # two accepted offsets: the smaller
    assert tm.cut_adapter(b"TTTT" + b"AGATNGGAAGAGC", AD, 13, 0) == 17        # the N is not compared: v = 12 < 13
    assert tm.cut_adapter(b"TTTT" + b"AGATNGGAAGAGC", AD, 12, 0) == 4
    assert tm.cut_adapter(b"TTTT" + b"AGATcGGAAGAGC", AD, 12, 0) == 4         # nor is a lower-case base
    ad20 = b"ACGTTGCAAGGCTTAGCCAT"
    two, three = b"AGGTTGCAAGCCTTAGCCAT", b"AGGTTGCAAGCCTTAGCGAT"
    assert tm.cut_adapter(b"GGGG" + two, ad20, 20, 10) == 4                   # 100 * 2 <= 10 * 20
    assert tm.cut_adapter(b"GGGG" + three, ad20, 20, 10) == 24                # 100 * 3 > 10 * 20
    assert tm.cut_adapter(b"ACGT", b"", 1, 0) == 4 and tm.cut_adapter(b"", AD, 5, 10) == 0
    assert tm.cut_adapter(b"CCAC", b"A", 1, 0) == 2


def test_pair_cut_by_hand():
    frag = b"ACGGTCATTGCAAGCTTGGACCATGAGTCCAATGCGTACCTGAAGTCTAG"                # 50 bases
    rc = bytes({65: 84, 67: 71, 71: 67, 84: 65}[x] for x in reversed(frag))
    p = tm.params(qual_min=0, adapter1=b"", min_len=0, pair_min_overlap=30, pair_mm_pct=10)
    # both mates read 60 bases of a fragment of 50: F = 50, d* = -10
    a, b = frag + b"T" * 10, rc + b"T" * 10
    assert tm.pair_offset(a, b, 30, 10) == -10
    rows, kept, ovl = tm.trim_unit([a, b], None, p)
    assert rows == [(50, 60, 60, 50), (50, 60, 60, 50)] and kept and ovl
    # mates of 40 and 35 bases of it: d* = F - Lb = 15, F > La: nothing to cut
    assert tm.pair_offset(frag[:40], rc[:35], 30, 10) is None                 # only 25 bases face each other
    assert tm.pair_offset(frag[:40], rc[:45], 30, 10) == 5
    rows, kept, ovl = tm.trim_unit([frag[:40], rc[:45]], None, p)
    assert rows == [(40, 40, 40, 40), (45, 45, 45, 45)] and ovl
    # mate 2 alone runs through: La = 50 = F, Lb = 58, d* = -8
    rows, _, ovl = tm.trim_unit([frag, rc + b"G" * 8], None, p)
    assert rows == [(50, 50, 50, 50), (50, 58, 58, 50)] and ovl
    # the option off, and single reads
    assert tm.trim_unit([a, b], None, dict(p, pair_overlap=False)) == ([(60, 60, 60, 60)] * 2, True, False)
    assert tm.trim_unit([a], None, p) == ([(60, 60, 60, 60)], True, False)
    # a short mate drops its partner
    rows, kept, _ = tm.trim_unit([a, b], [q(*[40] * 60), q(*[2] * 60)], dict(p, qual_min=20, min_len=20))
    assert rows == [(50, 60, 60, 50), (0, 0, 60, 50)] and not kept


def test_batch_units_and_tally_by_hand():
    p = tm.params(qual_min=0, min_len=5, pair_overlap=False)
    seqs = [b"TTTTTTTT" + AD, b"TTTT" + AD, b"TTTTTTTTTT", b"TTT"]
    rows, keep, t = tm.trim_batch(seqs, None, 0, p)
    assert rows.tolist() == [[8, 21, 8, 21], [4, 17, 4, 17], [10, 10, 10, 10], [3, 3, 3, 3]] and keep.tolist() == [1, 0, 1, 0]
    assert t["reads"].tolist() == [4, 0] and t["cut_reads"].tolist() == [[0, 2, 0], [0, 0, 0]] and t["bases_removed"].tolist() == [26, 0]
    assert t["short_reads"].tolist() == [2, 0] and (t["units"], t["units_kept"], t["pairs_overlapping"]) == (4, 2, 0)
    assert t["keep_hist"][0, [3, 4, 8, 10]].tolist() == [1, 1, 1, 1] and int(t["keep_hist"].sum()) == 4
    rows1, keep1, t1 = tm.trim_batch(seqs, None, 1, p)                         # units (0, 2) and (1, 3)
    rows2, keep2, t2 = tm.trim_batch(seqs, None, 2, p)                         # units (0, 1) and (2, 3)
    assert np.array_equal(rows1, rows) and np.array_equal(rows2, rows) and keep1.tolist() == [1, 0] and keep2.tolist() == [0, 0]
    assert t1["reads"].tolist() == [2, 2] and t1["short_reads"].tolist() == [1, 1] and t2["short_reads"].tolist() == [0, 2]
    assert t2["cut_reads"].tolist() == [[0, 1, 0], [0, 1, 0]] and t2["bases_removed"].tolist() == [13, 13]
    # a mate longer than the instance holds is cut to that first
    rows, _, t = tm.trim_batch([b"T" * 300], None, 0, p, lmax=256)
    assert rows.tolist() == [[256, 256, 256, 256]] and t["bases_removed"].tolist() == [0, 0]
    # adding onto a tally
    _, _, t3 = tm.trim_batch(seqs, None, 0, p, tally=tm.trim_batch(seqs, None, 0, p)[2])
    assert t3["units"] == 8 and t3["reads"].tolist() == [8, 0] and tm.tally_equal(t3, t3) and not tm.tally_equal(t3, t2)
