"""The duplicate census's public surface.  CPU: the five C ABI symbols in the binding's list and in the header with
`rc_dup_census`, the struct in the binding, the five `Context` methods, `-dups` / `-dups-max` in `rcorrector`'s help and in the
run_rcorrector.pl-style wrapper.  GPU: rc_dup_census_merge of two contexts on device 0 is the census of the union, and get twice
gives the same answer and leaves the keys intact.  (What they compute: tests/test_duplicates.py, tests/test_duplicates_cli.py,
tests/test_dup_keys.py.)"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rc_dup_census_begin", "rc_dup_census_get", "rc_dup_census_end", "rc_read_keys_device", "rc_dup_census_merge"]
FIELDS = ["units", "distinct_before", "distinct_after", "copies_before", "copies_after"]


def test_dup_entry_points_and_struct_are_declared():
    import rcorrector_amd
    assert set(SYMBOLS) <= set(rcorrector_amd.ABI_SYMBOLS)
    h = open(os.path.join(ROOT, "include", "rcorrector_amd.h")).read()
    m = re.search(r"typedef struct \{\s*uint64_t ([\w, ]+);\s*uint64_t ([\w, *]+);[^}]*\} rc_dup_census;", h)
    assert m and [x.strip(" *") for x in (m.group(1) + "," + m.group(2)).split(",")] == FIELDS
    for s in SYMBOLS:
        assert re.search(r"^int %s\(rc_ctx \*" % s, h, re.M), s
    assert "Equality is decided on the key\n * alone" in h or "decided on the key alone" in h.replace("\n * ", " ")
    lib = rcorrector_amd.load_library()
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_the_binding_mirrors_the_struct():
    from rcorrector_amd import binding
    assert [n for n, _ in binding._DupCensus._fields_] == FIELDS
    assert ctypes.sizeof(binding._DupCensus) == 40


def test_context_has_the_dup_census_methods():
    import rcorrector_amd
    for m in ("dup_census_begin", "dup_census", "dup_census_end", "read_keys_device", "dup_census_merge"):
        assert callable(getattr(rcorrector_amd.Context, m, None)), m


def test_cli_help_lists_dups():
    import rcorrector_amd
    rcorrector_amd.build_library()
    p = subprocess.run([os.path.join(ROOT, "rcorrector_amd", "rcorrector"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    e = p.stderr
    # the reference's part of the help comes first, unchanged; the new flags are in the build's own part, behind -weak-min
    assert e.index(b"MI355X build only:") < e.index(b"\t-weak-min INT:") < e.index(b"\t-dups STRING:") < e.index(b"\t-dups-max INT:")
    assert b"-verbose" in e[e.index(b"\t-dups STRING:"):e.index(b"\t-dups-max INT:")]


def test_wrapper_help_lists_dups():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_rcorrector_gpu")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    e = p.stderr
    assert e.index(b"\t-weak-min INT:") < e.index(b"\t-dups FILE:") < e.index(b"\t-dups-max INT:")


@pytest.mark.gpu
def test_merge_of_two_contexts_is_the_census_of_the_union_and_get_repeats():
    import rcorrector_amd
    from test_duplicates import MAX_BIN, assert_census, reads_of, units_of
    from test_recount import packed, unit_cuts
    from test_weak_profile import fixture, fixture_ctx
    f = fixture("fx_pe_k23")
    a, b = fixture_ctx(f), fixture_ctx(f)
    L = rcorrector_amd.load_library()
    assert L.rc_dup_census_merge(a._h, b._h) == -4                       # neither is open
    a.dup_census_begin()
    assert L.rc_dup_census_merge(a._h, b._h) == -4 and L.rc_dup_census_merge(a._h, a._h) == -1
    b.dup_census_begin()
    n = len(f["seqs1"])
    cuts = unit_cuts(f, 4)
    back = {}
    for i, (lo, hi) in enumerate(cuts):                                  # batches 0 and 2 on a, 1 and 3 on b; batch 0 on both
        for ctx in ([a, b] if i == 0 else [a if i % 2 == 0 else b]):
            _, _, off, _, args = packed(rcorrector_amd, f, lo, hi)
            ctx.correct_batch(f["mode"], *args)
            r = reads_of(np.concatenate(args[0::3]), off)
            back[i] = (r[:hi - lo], r[hi - lo:])
    before, after = [], []
    for i in [0, 2, 1, 3, 0]:                                            # a's units, then b's
        lo, hi = cuts[i]
        before += units_of(1, f["seqs1"][lo:hi], f["seqs2"][lo:hi])
        after += units_of(1, *back[i])
    only_b = b.dup_census(MAX_BIN)
    a.dup_census_merge(b)
    got = a.dup_census(MAX_BIN)
    assert got["units"] == n + (cuts[0][1] - cuts[0][0]) and got["copies_before"][2] > 0   # (batch 0's units, twice)
    assert_census(got, before, after, "merged")
    again = a.dup_census(MAX_BIN)                                        # get twice: the same answer, the keys intact
    assert all(np.array_equal(got[key], again[key]) for key in got)
    still_b = b.dup_census(MAX_BIN)                                      # the source keeps its own
    assert all(np.array_equal(only_b[key], still_b[key]) for key in only_b)
    small = a.dup_census(1)                                              # another bound over the same keys
    assert small["distinct_before"] == got["distinct_before"] and int(small["copies_before"][1]) == got["distinct_before"]
    for ctx in (a, b):
        ctx.dup_census_end()
        ctx.sync()
        ctx.close()
