"""Correction parity at every k the library accepts (rc_create: 1..32), not only at the k of the named data sets.

The code branches on k in many places -- the PACKED remainder (2k > 32 from k = 17), the counter's radix width (k < 16
or not), the instances of k_correct compiled for k = 23, 25 and 31, the probe kernels below k = 4 -- and which branch a
run takes depends on the table's size as much as on k: rc_k3_special returns the k = 23 / 25 instance only for a PACKED
table without extension bits, i.e. one of at least 2^(2k-32) home buckets (2^14 / 2^18), the k = 31 instance only for
one WITH them.  A table made of a few hundred reads' k-mers is far smaller, so some cases pad the table with k-mers that
no read holds (datasets.k_sweep: pad_to): the padding changes no read's result by design of the comparison -- the oracle
gets the same table -- it only gives the table the size at which the path under test is the one that runs.

CPU (-m "not gpu"): the oracle CLI against the unmodified reference binary, and the lane-serial build of the kernels'
control flow (tests/hostsim) against the oracle, at k = 3..32; k = 1 and 2 are fenced (test_k1_k2_*).
GPU (-m gpu): correct_batch against the oracle at k = 3..32 with the layout each k gets asserted, the k = 25 and k = 23
instances, PACKED with extension bits at k = 26..30, and the counter at k = 3..32."""
import functools
import os
import subprocess

import numpy as np
import pytest

import datasets
import synth

K_LO = 3            # below: the reference reads memory outside the read (test_k1_k2_are_fenced_the_reference_reads_outside_the_read)
KS = list(range(K_LO, 33))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "rcorrector_amd", "rcorrector")
WHAT = ["ret", "l", "m", "h", "seq1", "seq2"]


@functools.lru_cache(maxsize=4)
def _case(k, mode, pad_to=0):
    """(data set, the oracle's results on it): computed once, shared by the tests that need it, left unchanged"""
    from oracle import pyoracle
    pyoracle.build()
    pyoracle.lib()
    d = datasets.k_sweep(k, mode, pad_to)
    want = datasets.run_oracle(pyoracle, d)
    for a in want:
        a.setflags(write=False)
    return d, want


def _enough_corrected(want, k):
    """A case in which nothing is corrected cannot pass as parity: on these seeds the reference changes 260 or more reads
    of 600 (single) and 636 or more of 1 200 (paired) at every k >= 9.  Below k = 9 almost nothing is correctable (no read
    at k = 3..5, 44 reads at k = 8: nearly every k-mer that a substitution makes is in the table too), so there parity
    alone is asserted."""
    if k >= 9:
        assert int((want[0] > 0).sum()) >= 100, "k = %d: only %d reads corrected" % (k, int((want[0] > 0).sum()))


def _write_single(d, ds):
    with open(os.path.join(ds, "a.fq"), "wb") as f:
        for i, (r, q) in enumerate(zip(d["seqs1"], d["quals1"])):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, q))
    synth.write_dump(os.path.join(ds, "dump.jf"), d["keys"], d["counts"], d["k"])


def _run_cli(binary, k, ds, name, more=()):
    od = os.path.join(ds, name)
    os.makedirs(od)
    p = subprocess.run([binary, "-r", "a.fq", "-k", str(k), "-c", "dump.jf", "-od", od] + list(more), cwd=ds,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stderr, {f: open(os.path.join(od, f), "rb").read() for f in sorted(os.listdir(od))}


# ---- CPU -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_oracle_cli_equals_reference_at_every_k(oracle, k, tmp_path):
    """Pins the oracle at the k values the GPU sweep leans on: every output file and stderr, byte for byte, against the
    unmodified reference binary (skipped where oracle/_ref is not built, as in test_oracle_vs_ref.py)."""
    if not os.path.exists(oracle.REF_BIN):
        pytest.skip("oracle/_ref not built here (no /root/reference)")
    ds = str(tmp_path)
    _write_single(datasets.k_sweep(k, 0), ds)
    ref = _run_cli(oracle.REF_BIN, k, ds, "ref", ["-t", "3"] if k % 2 else [])
    ora = _run_cli(oracle.CLI_BIN, k, ds, "ora", ["-t", "2"])
    assert ref[0] == 0, ref[1].decode()
    assert ref[2].keys() == ora[2].keys() and ref[2]
    for f in ref[2]:
        assert ref[2][f] == ora[2][f], "%s differs at k = %d" % (f, k)
    assert ref[1] == ora[1], "stderr differs at k = %d" % k
    if k >= 9:   # (_enough_corrected: the same cap, counted in the reference's own output)
        heads = ref[2]["a.cor.fq"].split(b"\n")[0::4]
        assert sum(h.endswith(b" cor") for h in heads) >= 100


@pytest.mark.parametrize("mode", [0, 1], ids=["single", "paired"])
@pytest.mark.parametrize("k", KS)
def test_core_control_flow_matches_oracle_at_every_k(oracle, hostsim, k, mode):
    d, want = _case(k, mode)
    got = datasets.run_oracle(oracle, d, fn=lambda p, t, b: hostsim.hostsim_correct_batch(p, t, b, None))
    for w, g, what in zip(want, got, WHAT):
        assert np.array_equal(w, g), "%s differs at k = %d" % (what, k)
    _enough_corrected(want, k)


@pytest.mark.parametrize("k", [1, 2])
def test_k1_k2_are_fenced_the_reference_reads_outside_the_read(oracle, hostsim, k, tmp_path):
    """The fence below K_LO, with its evidence.  At k <= 2 every window counts as poly-A: IsPolyA's
    thresholds k - 2 and k - max(7, k / 2) are <= 0 (ErrorCorrection.cpp:53-71, :779, :875).  So no read has a trusted
    k-mer, the 'longest trusted run' is the empty one behind the last k-mer (:912-917: tstart = kcnt, tend = kcnt - 1), the
    one island made of it (:1002-1007) is [kcnt, kcnt + k - 2], and the one segment [0, kcnt - 1] is searched from an anchor
    that does not exist: at k = 1 to the right, the anchor k-mer read from seq[-1] (:1139-1142); at k = 2 to the left, the
    anchor read from seq[99] and seq[100], the terminating NUL, which indexes nucToNum[-65] (:1151-1154, KmerCode.cpp:13).
    An ASan + UBSan build of the reference stops in the first read on exactly that access at both k; the plain build
    goes on with whatever byte lies there (it marks no read, the same under -t 1 and -t 3, but that is the link map's and
    the heap's doing).  The oracle has fenced both accesses since SURVEY section 9.9 (return -1: `unfixable_error`), the
    kernels share that answer, and this test holds all three to it: every read that passes the screens in front of
    the search (:713-755) gets -1 and keeps its bases.  What the reference computes before the access -- the parameter
    lines on stderr, the l / m / h of every header -- must still be the oracle's."""
    for mode in (0, 1):
        d = datasets.k_sweep(k, mode)
        want = datasets.run_oracle(oracle, d)
        got = datasets.run_oracle(oracle, d, fn=lambda p, t, b: hostsim.hostsim_correct_batch(p, t, b, None))
        for w, g, what in zip(want, got, WHAT):
            assert np.array_equal(w, g), "%s differs at k = %d" % (what, k)
        assert (want[0] == -1).all()
        a, _ = oracle.pack_reads(d["seqs1"])
        assert np.array_equal(want[4], a)
    if not os.path.exists(oracle.REF_BIN):
        return
    ds = str(tmp_path)
    _write_single(datasets.k_sweep(k, 0), ds)
    ref = _run_cli(oracle.REF_BIN, k, ds, "ref")
    ora = _run_cli(oracle.CLI_BIN, k, ds, "ora")
    assert ref[0] == 0 and ora[0] == 0
    cut = ref[1].index(b"Processed")
    assert ref[1][:cut] == ora[1][:cut] and b"Bad quality threshold" in ref[1][:cut]
    rl, ol = ref[2]["a.cor.fq"].split(b"\n"), ora[2]["a.cor.fq"].split(b"\n")
    assert len(rl) == len(ol) == 4 * 600 + 1
    assert [h.split()[:4] for h in rl[0::4]] == [h.split()[:4] for h in ol[0::4]]   # @name l: m: h:
    assert all(h.endswith(b" unfixable_error") for h in ol[0:-1:4])


# ---- GPU -----------------------------------------------------------------------------------------------------------

def _packed_home_buckets(n):
    """rc_table.hip: rc_build_table_from_device_pairs -- the home buckets of a PACKED table of n entries at the default
    load of a table below 2 GiB (0.4; four 8-byte slots in a 32-byte bucket), and at least 64"""
    return max(64, int(n / (4 * 0.4)) + 1)


def _expected_layout(k, n):
    """(layout, ext, home buckets) the build chooses for n entries: PACKED (1) while the remainder needs at most 8
    extension bits, ext = the smallest number with buckets << ext >= 2^(2k-32); WIDE (0) beyond"""
    b = _packed_home_buckets(n)
    ext = 0
    while 2 * k > 32 and (b << ext) < (1 << (2 * k - 32)):
        ext += 1
    return (1 if ext <= 8 else 0), ext, b


def _ctx(d, env=None, monkeypatch=None):
    import rcorrector_amd
    for kk, v in (env or {}).items():
        monkeypatch.setenv(kk, v)   # (read when the context is made)
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    for kk in (env or {}):
        monkeypatch.delenv(kk)
    ctx.table_build(d["keys"], d["counts"])
    ctx.set_run_params(d["rate"], b"H")
    return ctx


def _check_layout(ctx, d):
    """The table has the layout the build's rule gives its size; returns (layout, ext).  A PACKED table reports its home
    buckets plus the buckets its last chains run on into (a displacement has five bits)."""
    layout, ext, home = _expected_layout(d["k"], len(d["keys"]))
    st = ctx.table_stats()
    assert st["entries"] == len(d["keys"])
    assert ctx.table_layout() == layout, "k = %d, %d entries: expected layout %d (ext %d)" % (d["k"], len(d["keys"]), layout, ext)
    if layout == 1:
        assert home < st["buckets"] <= home + 33
    return layout, ext


def _correct_and_compare(oracle, ctx, d, want, note=""):
    a, off = oracle.pack_reads(d["seqs1"])
    qa, _ = oracle.pack_reads(d["quals1"])
    if d["mode"] == 1:
        a2, off2 = oracle.pack_reads(d["seqs2"])
        qa2, _ = oracle.pack_reads(d["quals2"])
        got = ctx.correct_batch(1, a, qa, off, a2, qa2, off2) + (a, a2)
    else:
        got = ctx.correct_batch(0, a, qa, off) + (a,)
    for w, g, what in zip(want, got, WHAT):
        bad = np.nonzero(w != g)[0]
        assert len(bad) == 0, "%s differs at k = %d%s at %s (want %s got %s)" % (what, d["k"], note, bad[:5], w[bad[:5]], g[bad[:5]])


def _packed_boundary_and_compare(oracle, ctx, d, want):
    from test_gpu_parity import _packed_inputs
    arena, off, bases, exc_pos, exc_chr, qb = _packed_inputs(ctx, oracle, d)
    before = arena.copy()
    ctx.submit_packed(0, d["mode"], arena.size, off, bases, qb, exc_pos, exc_chr)
    ret, l, m, h, fix_pos, fix_chr = ctx.wait_packed(0)
    for w, g, what in zip(want[:4], (ret, l, m, h), WHAT):
        assert np.array_equal(w, g), "%s differs at k = %d through the packed boundary" % (what, d["k"])
    ctx.apply_fixes(arena, fix_pos, fix_chr)
    want_arena = np.concatenate(want[4:])
    assert np.array_equal(arena, want_arena)
    assert len(fix_pos) == int((before != want_arena).sum()) == int(want[0][want[0] > 0].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["single", "paired"])
@pytest.mark.parametrize("k", KS)
def test_correct_batch_matches_oracle_at_every_k(oracle, k, mode):
    """Unpadded tables: PACKED without extension bits up to k = 21, PACKED with them at k = 22..25, WIDE from k = 26 --
    asserted from the build's own rule, so that the sweep cannot change paths unnoticed when the load defaults move."""
    d, want = _case(k, mode)
    ctx = _ctx(d)
    layout, ext = _check_layout(ctx, d)
    assert (layout, ext > 0) == ((1, False) if k <= 21 else (1, True) if k <= 25 else (0, True))
    _correct_and_compare(oracle, ctx, d, want)
    reads, cors = ctx.summary()
    assert reads == len(want[0]) and cors == int(want[0][want[0] > 0].sum())
    _enough_corrected(want, k)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["single", "paired"])
@pytest.mark.parametrize("k,pad_to,min_buckets", [(25, 450_000, 1 << 18), (23, 30_000, 1 << 14)])
def test_the_instances_compiled_for_k25_and_k23_are_reached_and_match_the_oracle(oracle, k, pad_to, min_buckets, mode, monkeypatch):
    """rc_k3_special's preconditions, asserted: a PACKED table with ext == 0, i.e. at least 2^(2k-32) home buckets (which
    is what the padding is for), 100-base reads (the 192 class), no trace, no phase profile.  Then the oracle's results
    from the compiled-for-k instance, from the any-k instance over the same table (RC_K3_GENERIC=1), and through the
    packed transport."""
    d, want = _case(k, mode, pad_to)
    for env in ({}, {"RC_K3_GENERIC": "1"}):
        ctx = _ctx(d, env, monkeypatch)
        layout, ext = _check_layout(ctx, d)
        assert layout == 1 and ext == 0
        assert ctx.table_stats()["buckets"] >= min_buckets and _packed_home_buckets(len(d["keys"])) >= min_buckets
        _correct_and_compare(oracle, ctx, d, want, " under %s" % env)
        if not env:
            _packed_boundary_and_compare(oracle, ctx, d, want)
        ctx.close()
    _enough_corrected(want, k)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["single", "paired"])
@pytest.mark.parametrize("k,pad_to", [(26, 120_000), (27, 120_000), (28, 120_000), (29, 450_000), (30, 1_800_000)])
def test_packed_tables_with_extension_bits_between_k25_and_k31(oracle, k, pad_to, mode):
    """k = 26..30 over PACKED tables whose remainder borrows count bits (ext = 4, 6, 8, 8, 8 at these sizes): at the size
    of the unpadded sweep these k fall to WIDE.  (k = 31: test_k31_maxcork8_on_a_packed_table_with_extension_bits.)"""
    d, want = _case(k, mode, pad_to)
    ctx = _ctx(d)
    layout, ext = _check_layout(ctx, d)
    assert ctx.table_layout() == 1 and ctx.table_stats()["buckets"] < 1 << (2 * k - 32) and ext > 0
    _correct_and_compare(oracle, ctx, d, want)
    _enough_corrected(want, k)
    ctx.close()


def _palindromes(keys, k):
    return keys[keys == datasets.revcomp_codes(keys, k)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_counter_equals_exact_counts_at_every_k(k):
    """The streaming counter (radix width min(k, 16), rc_count.hip) at every k, on the sweep's reads plus 40 reads of
    ACGTACGT...: for k divisible by 4 some of their k-mers are their own reverse complement, and each occurrence of such
    a k-mer counts once, as `jellyfish count -C` counts it."""
    import rcorrector_amd
    from test_gpu_count import arena_of, sorted_pairs
    s1, _, _, _, _ = synth.make_reads(7100 + k, 600, 100, n_tx=6, l_tx=400, e=0.01)
    extra = np.tile(np.frombuffer(b"ACGT" * 25, np.uint8), (40, 1))
    want_k, want_c = synth.count_kmers([s1, extra], k)
    if k % 4 == 0:
        pal = _palindromes(want_k, k)
        assert len(pal) > 0
        # ACGT... has 101 - k windows, every fourth one starting with A, every fourth with G: both their own reverse complement
        a_code = np.uint64(int("".join("%d%d" % (c >> 1, c & 1) for c in ([0, 1, 2, 3] * 8)[:k]), 2))
        assert a_code in pal and int(want_c[want_k == a_code][0]) >= 40 * len(range(0, 101 - k, 4))
    rows = [r for r in s1] + [r for r in extra]
    ctx = rcorrector_amd.Context(k=k)
    ctx.count_begin()
    for lo, hi in ((0, 1), (1, 333), (333, len(rows))):
        ctx.count_add(arena_of(rows[lo:hi]))
    n = ctx.count_finish(2)
    got_k, got_c = sorted_pairs(*ctx.table_export())
    assert n == len(want_k)
    assert np.array_equal(got_k, want_k) and np.array_equal(got_c, want_c)
    assert np.array_equal(ctx.lookup(want_k), want_c.astype(np.int32))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 17, 24, 25])
def test_cli_without_c_one_pass_equals_two_passes_around_the_radix_width(k, tmp_path):
    """`rcorrector` without -c counts the k-mers itself: either side of the counter's radix-width switch (k = 16, 17) and
    at a k divisible by 4 and its neighbour (24, 25), one pass over the file must write what two passes write."""
    from test_gpu_fuzz import _one_pass_equals_two
    ds = str(tmp_path)
    d = datasets.k_sweep(k, 0)
    _write_single(d, ds)
    _one_pass_equals_two(["-r", "a.fq", "-k", str(k), "-c", "dump.jf"], ds, k)
