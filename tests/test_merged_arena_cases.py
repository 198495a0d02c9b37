"""CPU: the fixtures of tests/merged_arena.py are what they claim, by the model (tests/merge_model.py) and the oracle
(oracle/pyoracle.py) alone.  A fixture that would make a comparison of tests/test_merged_arena.py vacuous -- no run of 64 empty
reads, no read the oracle changes in some length tier, no weak window left, a table nothing is solid in -- fails here, without a GPU."""
import numpy as np
import pytest

import merge_model as mm
import merged_arena as ma
from test_weak_profile import restate_all as weak_rows

K = ma.K


@pytest.mark.parametrize("name", ["mixed", "mixed_fasta", "long"])
def test_lengths_runs_and_offsets(name):
    a = ma.arena(name)
    lens = [len(s) for s in a["strings"]]
    rows, moff, mseq, mqual, tally = a["want"]
    for L in ma.EDGE_LENGTHS:
        assert L in lens, "no merged read of %d bases" % L
    assert len({L for L in lens if 40 <= L <= 300}) >= 40, "the spread of lengths between 40 and 300"
    runs = ma.runs_of_empty(a["strings"])
    for n in ma.RUNS:
        assert n in runs[1:-1], "no run of %d unmerged units between merged reads" % n
    last = ma.LONG_LAST_RUN if name == "long" else ma.LAST_RUN
    assert lens[:ma.FIRST_RUN] == [0] * ma.FIRST_RUN and lens[ma.FIRST_RUN] > 0 and lens[-last:] == [0] * last and lens[-last - 1] > 0
    starts = moff[:-1][np.array(lens) > 0]
    assert set((starts % 16).tolist()) == set(range(16)), "a merged read starts at every residue of 16"
    assert set((moff[ma.FIRST_RUN:ma.FIRST_RUN + 17] % 16).tolist()) == set(range(16)), "the leading units walk the residues"
    assert set((moff % 16).tolist()) == set(range(16)) and int(moff[-1]) == len(mseq) == sum(lens) + len(lens) < 1 << 20
    assert len(lens) <= 4000 and a["max_read_len"] <= 1023
    over = sorted(L for L in lens if L > 1023)
    assert over == (list(ma.LONG_LENGTHS) if name == "long" else []), over
    assert a["max_len"] == (2045 if name == "long" else 1023)
    if name == "mixed_fasta":
        assert mqual is None and tally["took_mate1"] == tally["took_mate2"] == 0 and tally["ties"] > 10
        assert lens == [len(s) for s in ma.arena("mixed")["strings"]]
        return
    base, cap = a["p"]["qual_base"], a["p"]["qual_cap"]
    q = np.frombuffer(mqual, np.uint8)
    assert (q == base + 2).sum() >= 10, "a disagreement at the floor: quality qual_base + 2"
    assert (q == base + cap).sum() >= 100, "an agreement at Q40 + Q40: the cap"
    assert q[q != 0].max() == base + cap and tally["ties"] > 5 and tally["took_mate2"] > 5 and tally["mismatches"] > 20
    assert all(len(s) == len(t) for s, t in zip(a["strings"], a["qstrings"]))


def test_long_holds_mixeds_reads_in_front():
    m, g = ma.arena("mixed"), ma.arena("long")
    n = len(m["strings"])
    assert g["strings"][:n] == m["strings"] and g["qstrings"][:n] == m["qstrings"], "min_overlap 1 merges mixed's pairs as min_overlap 20 does"
    assert [len(s) for s in g["strings"][n:]] == list(ma.LONG_LENGTHS) + [0] * ma.LONG_LAST_RUN
    assert g["want"][0][n + 2].tolist()[2] == 1, "the read of 2045 bases: an overlap of one base"


def test_unmerged_is_nothing_but_nul_bytes():
    a = ma.arena("unmerged")
    rows, moff, mseq, mqual, tally = a["want"]
    n = ma.N_UNMERGED
    assert mseq == mqual == b"\0" * n and moff.tolist() == list(range(n + 1)) and not rows.any() and a["max_len"] == 0
    assert tally["unmerged"] == n == tally["len_hist"][0] and a["strings"] == [b""] * n
    assert sum(1 for s in a["seqs"] if len(s) >= 40) > 900, "mates long enough to overlap, which do not"


@pytest.mark.parametrize("name", ["mixed", "mixed_fasta"])
def test_the_oracle_corrects_reads_of_every_length_tier_and_leaves_weak_windows(name):
    a = ma.arena(name)
    strong, ret, l, m, h, fixed = ma.oracle_want(name)
    lens = np.array([len(s) for s in a["strings"]])
    changed = np.array([s != t for s, t in zip(a["strings"], fixed)])
    assert np.array_equal(changed, ret > 0)
    for lo, hi in ((K, 160), (161, 320), (321, 1023)):
        tier = (lens >= lo) & (lens <= hi)
        assert (changed & tier).sum() >= 2, "%s: the oracle changes %d reads of %d to %d bases" % (name, (changed & tier).sum(), lo, hi)
    assert changed.sum() >= 30 and (ret[lens == 0] == ret[0]).all() and not changed[lens == 0].any()
    assert len(set(strong[lens >= K].tolist())) > 3 and (strong[lens == 0] == strong[0]).all()
    weak = weak_rows(fixed, K, ma.table_counts(), 1)
    assert (weak[:, 0] > 0).sum() >= 2, "a corrected read with a weak window left"
    assert ((weak[:, 0] == 0) & (lens >= K)).sum() > 50, "and reads without one"
    assert 0 < ma.error_rate() < 0.1


def test_the_tables_are_not_empty():
    full, half = ma.table_counts(), ma.table_counts("half")
    assert len(full) > 10000 and 0.3 * len(full) < len(half) < 0.7 * len(full) and min(full.values()) >= 20
    for name in ("mixed", "long"):
        c = ma.strings_counts(ma.arena(name)["strings"])
        assert len(c) > 10000 and sum(1 for x in c if x in full) > 0.8 * len(c) and sum(1 for x in c if x not in full) > 100
    assert ma.strings_counts(ma.arena("unmerged")["strings"]) == {}
    hit = sum(1 for s in ma.arena("long")["strings"] if len(s) >= K and any(ma.canonical(s[i:i + K]) in half for i in range(len(s) - K + 1)))
    merged = sum(1 for s in ma.arena("long")["strings"] if len(s) >= K)
    assert 0.3 * merged < hit < 0.8 * merged, "the screen set holds about half of the reads"
