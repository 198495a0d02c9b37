"""CPU: tests/transport_model.py -- the numpy statement of the packed and the resident boundary that
tests/test_transport_kernels.py holds the kernels to -- agrees with itself and with the library's host half, and the sub-ranges
that file submits through rc_submit_resident exist in the data sets and mean to the oracle what the test takes them to mean."""
import numpy as np
import pytest

import datasets
import transport_model as tm

SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 16383, 16384, 16385, 65541]


@pytest.mark.parametrize("nbytes", SIZES)
def test_pack_then_unpack_gives_the_arena_back(nbytes):
    """Random arenas with N, IUPAC and lower-case letters (none, about 1 %, all of the bases), reads of random lengths with a
    1-byte read among them: unpack(pack(arena)) is the arena; the codes sit where rc_transport.hip's header says (checked against a
    byte-by-byte loop on the small sizes); the exception list is what is neither a base nor a NUL."""
    rng = np.random.default_rng(1000 + nbytes)
    for density in (0.0, 0.01, 1.0):
        off = tm.read_offsets(rng, nbytes)
        assert off[0] == 0 and off[-1] == nbytes and (np.diff(off.astype(np.int64)) == 1).any()
        arena = tm.random_arena(rng, off, density)
        assert arena.size == nbytes and (arena[off[1:].astype(np.int64) - 1] == 0).all()
        words, exc_pos, exc_chr = tm.pack(arena)
        assert len(words) == (nbytes + 15) // 16
        if nbytes <= 4097:
            slow = [0] * len(words)
            for p, ch in enumerate(arena.tolist()):
                slow[p >> 4] |= {65: 0, 67: 1, 71: 2, 84: 3}.get(ch, 0) << (30 - 2 * (p & 15))
            assert words.tolist() == slow
        is_exc = (arena != 0) & ~np.isin(arena, tm.ACGT)
        assert np.array_equal(exc_pos, np.nonzero(is_exc)[0]) and np.array_equal(exc_chr, arena[is_exc])
        if density == 1.0:
            assert is_exc.sum() == (arena != 0).sum() and not words.any()
        if density == 0.0:
            assert not is_exc.any()
        assert np.array_equal(tm.unpack(words, nbytes, off, (exc_pos, exc_chr)), arena)
        # the letters of the padding are those of code 0
        assert (tm.letters(words)[nbytes:] == ord("A")).all()


def test_model_agrees_with_the_librarys_host_packer():
    """rc_pack_bases is host code: the model's words and exception list are the library's on a random arena (no GPU)."""
    import rcorrector_amd
    rcorrector_amd.build_library()
    L = rcorrector_amd.load_library()
    rng = np.random.default_rng(7)
    off = tm.read_offsets(rng, 65541)
    arena = tm.random_arena(rng, off, 0.01)
    words, exc_pos, exc_chr = tm.pack(arena)
    bases = np.full(len(words), 0xDEADBEEF, np.uint32)
    ep, ec = np.zeros(len(exc_pos) + 4, np.uint32), np.zeros(len(exc_pos) + 4, np.uint8)
    n = L.rc_pack_bases(arena.ctypes.data, 0, arena.size, bases.ctypes.data, ep.ctypes.data, ec.ctypes.data, len(ep))
    assert n == len(exc_pos) and np.array_equal(bases, words) and np.array_equal(ep[:n], exc_pos) and np.array_equal(ec[:n], exc_chr)


def test_fix_models_on_a_hand_made_arena():
    """"ACGN" + NUL + "nT" + NUL: which changes are fixes, by hand."""
    arena = np.frombuffer(b"ACGN\0nT\0", np.uint8)
    words, exc_pos, exc_chr = tm.pack(arena)
    assert words.tolist() == [(1 << 28) | (2 << 26) | (3 << 18)] and exc_pos.tolist() == [3, 5] and bytes(exc_chr) == b"Nn"
    #                  A->T  C kept  G->N: none  N->A: listed  NUL  n->G: listed  T->a: none  NUL
    after = np.frombuffer(b"TCNA\0Ga\0", np.uint8)
    pos, chr_ = tm.fixes_packed(words, exc_pos, after)
    assert pos.tolist() == [0, 3, 5] and bytes(chr_) == b"TAG"
    # untouched exceptions and NULs are no fixes, nor is a NUL's code (0 = 'A') against the NUL
    pos, chr_ = tm.fixes_packed(words, exc_pos, arena)
    assert pos.size == 0
    pos, chr_ = tm.fixes_bytes(arena, after)
    assert pos.tolist() == [0, 2, 3, 5, 6] and bytes(chr_) == b"TNAGa"


def _offsets(oracle, d):
    _a1, off1 = oracle.pack_reads(d["seqs1"])
    off2 = oracle.pack_reads(d["seqs2"])[1] if d["mode"] == 1 else None
    return off1, off2


def test_sub_ranges_at_every_alignment_exist(oracle):
    """varlen has a read that starts at every offset modulo 16 in its second half, and pe_var pairs (i, j) whose second-mate range
    starts at every offset modulo 16 while the first-mate range's length takes every value modulo 16: the cases
    test_transport_kernels.py submits as resident sub-batches."""
    off1, _ = _offsets(oracle, datasets.make("varlen"))
    n = len(off1) - 1
    starts = tm.start_at_every_shift(off1, n // 2)
    assert sorted(starts) == list(range(16))
    assert all(i >= n // 2 and int(off1[i]) % 16 == s for s, i in starts.items())
    off1, off2 = _offsets(oracle, datasets.make("pe_var"))
    n = len(off1) - 1
    cuts = tm.paired_cuts(off1, off2, n // 2)
    assert sorted(cuts) == list(range(16))
    assert sorted(int(off2[i]) % 16 for i, j in cuts.values()) == list(range(16))
    assert sorted(int(off1[j] - off1[i]) % 16 for i, j in cuts.values()) == list(range(16))
    assert all(n // 2 <= i < j <= n for i, j in cuts.values())


def test_the_oracles_rows_of_a_sub_range_are_its_results_on_the_sub_range(oracle):
    """The oracle corrects a read (a pair) from the read (the pair), the table and the run parameters alone: its rows i.. of a whole
    data set are what it gives on reads i.. as a data set of their own -- so one oracle run per data set, indexed, is the
    reference of every sub-batch."""
    d = datasets.make("varlen")
    want = datasets.run_oracle(oracle, d)
    off1, _ = _offsets(oracle, d)
    i = tm.start_at_every_shift(off1, len(off1) // 2)[7]
    sub = datasets.run_oracle(oracle, dict(d, seqs1=d["seqs1"][i:], quals1=d["quals1"][i:]))
    for w, g in zip(want[:4], sub[:4]):
        assert np.array_equal(w[i:], g)
    assert np.array_equal(want[4][off1[i]:], sub[4])
    d = datasets.make("pe_var")
    want = datasets.run_oracle(oracle, d)
    off1, off2 = _offsets(oracle, d)
    n = len(off1) - 1
    i, j = tm.paired_cuts(off1, off2, n // 2)[3]
    sub = datasets.run_oracle(oracle, dict(d, seqs1=d["seqs1"][i:j], quals1=d["quals1"][i:j], seqs2=d["seqs2"][i:j], quals2=d["quals2"][i:j]))
    idx = np.concatenate([np.arange(i, j), n + np.arange(i, j)])
    for w, g in zip(want[:4], sub[:4]):
        assert np.array_equal(w[idx], g)
    assert np.array_equal(want[4][off1[i]:off1[j]], sub[4]) and np.array_equal(want[5][off2[i]:off2[j]], sub[5])
