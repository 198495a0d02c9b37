"""numpy model of rc_table_compare (include/rcorrector_amd.h): the joint count matrix and the statistics of two k-mer sets,
by a join on the canonical code.  A set is (codes, counts) as rc_table_build takes it: forward or canonical codes, a later
duplicate overrides an earlier one."""
import numpy as np

import datasets

STAT_FIELDS = ("distinct_a", "distinct_b", "shared", "mass_a", "mass_b", "shared_mass_a", "shared_mass_b", "max_count_a", "max_count_b")


def canonical_set(codes, counts, k):
    """(sorted distinct canonical codes, the count of each: the LAST one given for it)"""
    codes = np.asarray(codes, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.int64)
    canon = np.minimum(codes, datasets.revcomp_codes(codes, k))
    uniq, first_rev = np.unique(canon[::-1], return_index=True)   # the first in reversed order = the last Put
    return uniq, counts[::-1][first_rev]


def compare(set_a, set_b, k, max_bin):
    """{"cells": uint64 (max_bin + 1, max_bin + 1), and STAT_FIELDS as ints}"""
    ka, ca = canonical_set(*set_a, k)
    kb, cb = canonical_set(*set_b, k)
    both = np.union1d(ka, kb)
    in_a, in_b = np.zeros(len(both), np.int64), np.zeros(len(both), np.int64)
    in_a[np.searchsorted(both, ka)] = ca
    in_b[np.searchsorted(both, kb)] = cb
    n = max_bin + 1
    flat = np.minimum(in_a, max_bin) * n + np.minimum(in_b, max_bin)
    cells = np.bincount(flat, minlength=n * n).astype(np.uint64).reshape(n, n)
    shared = (in_a > 0) & (in_b > 0)
    py = lambda a: int(a.sum(dtype=np.int64))   # (counts are below 2^31 and there are far fewer than 2^32 of them: exact)
    out = {"distinct_a": len(ka), "distinct_b": len(kb), "shared": int(shared.sum()), "mass_a": py(ca), "mass_b": py(cb),
           "shared_mass_a": py(in_a[shared]), "shared_mass_b": py(in_b[shared]),
           "max_count_a": int(ca.max()) if len(ca) else 0, "max_count_b": int(cb.max()) if len(cb) else 0}
    out["cells"] = cells
    return out


def transposed(r):
    """what compare(b, a) must give where r = compare(a, b)"""
    swap = {"distinct_a": "distinct_b", "mass_a": "mass_b", "shared_mass_a": "shared_mass_b", "max_count_a": "max_count_b"}
    swap.update({v: k for k, v in swap.items()})
    out = {f: r[swap.get(f, f)] for f in STAT_FIELDS}
    out["cells"] = r["cells"].T
    return out
