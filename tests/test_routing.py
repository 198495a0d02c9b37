"""Which kernel finishes each read: the device's routing against the model of the early finish (tests/k2s_model.py).

A batch is corrected by three kernels and every read is finished by one of them: the threshold kernel (rc_quarter.h: clean on
the real counts), k_single (rc_single.h: isolated substitutions, conditions (1)-(6)) or k_correct (everything else).  The
parity suites only see the three together, and k_correct corrects whatever an earlier kernel declines -- so k_single could
decline every read, or the threshold kernel could flag none, and they would stay green.  tests/test_k2s_model.py proves on
the CPU that what the model accepts is finished right; here the device kernels are held to the model's acceptance set, read
by read and in both directions, through rc_debug_routes (cls / cand / runs of the last batch, copied out of HBM):

    cls == 0, cand == 0   T   finished by the threshold kernel
    cls == 0, cand  > 0   S   finished by k_single
    cls != 0, cand  > 0   D   offered to k_single, declined, finished by k_correct
    cls != 0, cand == 0   C   straight to k_correct

(a) model T <=> device T, model S <=> device S, with the model's ret, bases and l / m / h (k_single clears cls at
rc_single.h:368); (b) the candidate flag and the stretches in `runs` equal the model's condition (2) -- so a declined
candidate is one the model rejects in (3)-(6), or one with more stretches than MAX_FIX_PER_K allows k_single, which the
flag does not look at (rc_single.h:121-122) -- and the work class of what goes to
k_correct is that of rc_quarter.h:510; (c) planted reads whose route is known without the model; (d) the project's own data
sets; (e) the hook's refusals, and RC_NO_SINGLE=1, under which every S becomes D.

No read is excused: the threshold kernel finishes a read only as clean (rc_quarter.h:505, :525) -- reads shorter than k and
the screened ones (:310) keep class 1 (:461, :510) and are k_correct's, route C -- so the sets must be equal, and are.  The
limits rc_single.h states for the device and the model does not have are the predicates DEVICE_LIMITS below.

What the model gives on the CPU for the first 600 units of each set of (d), T / S / D / C:
    se_k23 78/9/56/457   pe_k23 323/98/139/640   il_k23 314/112/115/659   skew 239/166/25/170   k11 321/111/35/133
    k32 59/9/45/487   pe_151 290/116/94/700   pe_160_k15 358/259/85/498   polya_k23 360/65/17/158   k15 156/8/49/387
(every D of these sets is declined in (3)-(6)).
"""
import functools

import numpy as np
import pytest

import datasets
import k2s_model as M
import synth

pytestmark = pytest.mark.gpu

# The shape limits of the device kernels that the model does not have (a read outside them is not expected S):
DEVICE_LIMITS = {
    "read length <= 160": lambda Ln, k, mfk, nseg: Ln <= 160,                          # rc_single.h:56, :94 (MAX_LEN)
    "kcnt >= 5": lambda Ln, k, mfk, nseg: Ln - k + 1 >= 5,                              # rc_single.h:94, rc_quarter.h:568
    "mfk >= 2": lambda Ln, k, mfk, nseg: mfk >= 2,                                      # rc_single.h:76
    "stretches <= min(3, mfk - 1)": lambda Ln, k, mfk, nseg: nseg <= min(3, mfk - 1),   # rc_single.h:121-122 (MAX_SEG)
}


def _po():
    from oracle import pyoracle
    pyoracle.build()
    pyoracle.lib()
    return pyoracle


def _all_reads(d):
    """the batch's reads in the device's order, and the mate of each (None: single-end)"""
    if d["mode"] == 1:
        n1 = len(d["seqs1"])
        return d["seqs1"] + d["seqs2"], (lambda i: i + n1 if i < n1 else i - n1)
    return d["seqs1"], ((lambda i: i ^ 1) if d["mode"] == 2 else None)


def _work_class(po, P, T, seq, k, s, screened):
    """rc_quarter.h:510 -- 4 / 3 / 2 / 1 by the share of k-mers below s: >= 7/8, >= 3/4, >= 1/2, the rest; the count is taken
    over the array the threshold scan sorted, in which a window that is poly-A at max(7, k/2) stands as -1 (:314-331, :483);
    a screened read, and one with every k-mer below s, has class 1 (:461)"""
    kc = len(seq) - k + 1
    if screened or kc <= 0:
        return 1
    x = np.where(M.polya(seq, k, max(7, k // 2)), -1, po.kmer_counts(P, T, seq).astype(np.int64))
    nb = int((x < s).sum())
    if nb >= kc:
        return 1
    return 4 if nb >= kc - (kc >> 3) else (3 if nb >= kc - (kc >> 2) else (2 if nb >= kc - (kc >> 1) else 1))


def _expect(d):
    """The model's verdict per read, on the CPU: route 'T' / 'S' / 'other', the result (ret, bases, l, m, h) where it accepts,
    cand (the threshold kernel's flag: condition (2) with 1..3 stretches, rc_quarter.h:568-626), segs, why (where a candidate is
    not S) and cls (the work class, should the read go to k_correct).  Also the oracle's results on the batch."""
    po = _po()
    k, mfk = d["k"], d["mfk"]
    T = po.Table(k, len(d["keys"]))
    T.put_many(d["keys"], d["counts"])
    P = po.make_params(k, mfk, d["rate"], d.get("badq", b"H"))
    seqs, mate = _all_reads(d)
    strong, info = M.front_end(P, T, seqs, k)
    out = []
    for i, s in enumerate(seqs):
        pt = -1 if mate is None else int(min(strong[i], strong[mate(i)]))
        args = (P, T, s, k, mfk, int(strong[i]), int(info[i]), pt)
        sh = M.shape(*args)
        r = M.finished_early(*args, allow_double=False)
        e = dict(route="other", res=r, cand=False, segs=None, why=None)
        if sh is not None and not sh["clean"] and sh["segs"] is not None:
            e["segs"] = [(z0, z1) for z0, z1, _ in sh["segs"]]
            e["cand"] = 1 <= len(e["segs"]) <= 3 and sh["kc"] >= 5
        nseg = len(e["segs"]) if e["segs"] else 0
        failed = [name for name, f in DEVICE_LIMITS.items() if not f(len(s), k, mfk, nseg)]
        if r is not None and r[0] == 0:
            assert sh["clean"]
            e["route"] = "T"
        elif r is not None and not failed:
            e["route"] = "S"
        elif e["cand"]:   # a candidate the model does not finish: a device limit, or conditions (3)-(6) -- (1)-(2) hold, that is what cand says
            assert failed or sh["ok"]
            e["why"] = "; ".join(failed) if failed else "(3)-(6)"
        s1, t1 = M.first_thresholds(P, int(strong[i]), int(info[i]), pt)
        e["thresholds"], e["own_thresholds"] = (s1, t1), M.first_thresholds(P, int(strong[i]), int(info[i]), -1)
        e["cls"] = _work_class(po, P, T, s, k, s1, bool(info[i] & 4))
        out.append(e)
    want = datasets.run_oracle(po, d)
    for a in want:
        a.setflags(write=False)
    return out, want


def _run(d, monkeypatch, env=None):
    """the batch through Context.correct_batch; dict(ret, l, m, h, seqs, cls, cand, runs, launches of probe / threshold / k_single)"""
    import rcorrector_amd
    po = _po()
    for kk, v in (env or {}).items():
        monkeypatch.setenv(kk, v)   # (read when the context is made)
    ctx = rcorrector_amd.Context(k=d["k"], max_fix_per_k=d["mfk"], device=0)
    for kk in (env or {}):
        monkeypatch.delenv(kk)
    try:
        ctx.table_build(d["keys"], d["counts"])
        ctx.set_run_params(d["rate"], d.get("badq", b"H"))
        a, off = po.pack_reads(d["seqs1"])
        qa, _ = po.pack_reads(d["quals1"])
        arenas = [a]
        ctx.profile(True)
        ctx.profile_reset()
        if d["mode"] == 1:
            a2, off2 = po.pack_reads(d["seqs2"])
            qa2, _ = po.pack_reads(d["quals2"])
            arenas.append(a2)
            res = ctx.correct_batch(1, a, qa, off, a2, qa2, off2)
            seqs = po.unpack_reads(a, off) + po.unpack_reads(a2, off2)
        else:
            res = ctx.correct_batch(d["mode"], a, qa, off)
            seqs = po.unpack_reads(a, off)
        launches = tuple(int(ctx.profile_get(i)[1]) for i in (0, 1, 3))
        ctx.profile(False)
        cls, cand, runs = ctx.debug_routes(len(seqs))
        layout, buckets = ctx.table_layout(), ctx.table_stats()["buckets"]
    finally:
        ctx.close()
    return dict(ret=res[0], l=res[1], m=res[2], h=res[3], seqs=seqs, arenas=arenas, cls=cls, cand=cand, runs=runs, launches=launches,
                layout=layout, buckets=buckets)


def _route(cls, cand):
    return ("S" if cand else "T") if cls == 0 else ("D" if cand else "C")


def _stretches(word):
    """rc_quarter.h:624-628: per stretch first k-mer | length << 8; x = stretch 0 | stretch 1 << 16, y = stretch 2 | n << 16"""
    x, y = int(word) & 0xFFFFFFFF, int(word) >> 32
    n = y >> 16
    rs = [x & 0xFFFF, x >> 16, y & 0xFFFF][:n]
    return n, [(r & 0xFF, (r & 0xFF) + (r >> 8) - 1) for r in rs]


def _check(d, exp, want, got, tag, no_single=False):
    """(a) and (b) on one batch; returns the device routes"""
    seqs, _ = _all_reads(d)
    routes = [_route(int(c), int(f)) for c, f in zip(got["cls"], got["cand"])]
    print("%s: device T/S/D/C = %s, model T/S/other = %s" % (tag, [routes.count(x) for x in "TSDC"], [sum(e["route"] == x for e in exp) for x in ("T", "S", "other")]))
    # the three kernels together give the oracle's bytes (what the parity suites check; here so that a route is never read off a wrong run)
    for w, g, what in zip(want[:4], (got["ret"], got["l"], got["m"], got["h"]), ("ret", "l", "m", "h")):
        assert np.array_equal(w, g), "%s: %s differs from the oracle at %s" % (tag, what, np.nonzero(w != g)[0][:5])
    for w, g in zip(want[4:], got["arenas"]):
        assert np.array_equal(w, g), "%s: bases differ from the oracle" % tag
    bad = []
    for i, (e, r) in enumerate(zip(exp, routes)):
        o16 = "read %d (%d bases, arena offset %% 16 = %d)" % (i, len(seqs[i]), _offset16(d, i))
        # (b) the hand-over: the flag is condition (2), the stretches are the model's
        if bool(got["cand"][i]) != e["cand"]:
            bad.append("%s: cand = %d, the model's condition (2) says %s" % (o16, got["cand"][i], e["cand"]))
            continue
        if e["cand"]:
            n, zs = _stretches(got["runs"][i])
            if n != len(e["segs"]) or zs != e["segs"] or int(got["cand"][i]) != n:
                bad.append("%s: runs = %d %s (cand %d), the model's stretches are %s" % (o16, n, zs, got["cand"][i], e["segs"]))
        # (a) both directions
        want_r = e["route"]
        have_r = r if r in ("T", "S") else "other"
        if no_single and want_r == "S":   # nobody takes the candidates: what k_single would have finished is D, every other D is as before
            want_r = "D"
            have_r = r
        if want_r != have_r:
            bad.append("%s: route %s, the model says %s%s" % (o16, r, e["route"], " (%s)" % e["why"] if e["why"] else ""))
            continue
        if r in ("T", "S"):
            res = (int(got["ret"][i]), got["seqs"][i], int(got["l"][i]), int(got["m"][i]), int(got["h"][i]))
            if res != e["res"]:
                bad.append("%s: route %s with %s, the model's result is %s" % (o16, r, res, e["res"]))
        else:   # (a D here is a read the model rejects in (3)-(6) or by a device limit: its cand flag equals the model's (1)-(2), checked above)
            if int(got["cls"][i]) != e["cls"]:
                bad.append("%s: work class %d, rc_quarter.h:510 gives %d" % (o16, got["cls"][i], e["cls"]))
    assert not bad, "%s: %d reads\n%s" % (tag, len(bad), "\n".join(bad[:12]))
    return routes


def _offset16(d, i):
    seqs, _ = _all_reads(d)
    return int(sum(len(s) + 1 for s in seqs[:i]) % 16)


# ---- (c) planted reads -------------------------------------------------------------------------------------------------

SEED = 20260
NUC = np.frombuffer(b"ACGT", np.uint8)


@functools.lru_cache(maxsize=None)
def _transcripts(k):
    """three random 600-base transcripts and the table: every canonical k-mer of the first and the third at count 50, of the
    second (the mates with the lower strong threshold) at count 8, and nothing else"""
    rng = np.random.Generator(np.random.PCG64(SEED + k))
    tx = [NUC[rng.integers(0, 4, 600)] for _ in range(2)]
    tx.append(NUC[rng.choice(4, 600, p=[0.04, 0.46, 0.46, 0.04])])   # (few A's and T's: its shortest pieces pass the screens)
    k1 = np.unique(np.concatenate([synth.canonical_codes(tx[0][None, :], k), synth.canonical_codes(tx[2][None, :], k)]))
    k2 = np.unique(synth.canonical_codes(tx[1][None, :], k))
    assert not np.isin(k2, k1).any()
    keys = np.concatenate([k1, k2])
    cnt = np.concatenate([np.full(len(k1), 50, np.int64), np.full(len(k2), 8, np.int64)])
    order = np.argsort(keys)
    return tx, keys[order], cnt[order]


def _padded(keys, cnt, k, pad_to):
    """absent k-mers until the table has the size -- and so the layout -- of a real one (datasets.k_sweep, test_stage_wide.py)"""
    rng = np.random.Generator(np.random.PCG64(SEED + 7))
    mask = np.uint64((1 << (2 * k)) - 1)
    m = pad_to + pad_to // 8
    fwd = (rng.integers(0, 1 << 63, size=m, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=m, dtype=np.uint64)) & mask
    pad = np.unique(np.minimum(fwd, datasets.revcomp_codes(fwd, k)))
    pad = rng.permutation(pad[~np.isin(pad, keys)])[:pad_to - len(keys)]
    return np.concatenate([keys, pad]), np.concatenate([cnt, rng.integers(2, 200, size=len(pad)).astype(np.int64)])


def _anchored(L, k, p):
    """One substitution at base p of an L-base read takes the k-mers lo..hi that hold it out of the table.  What is left on
    either side must be no k-mer or at least two: a lone trusted k-mer is a 1-run of length one, which condition (2) refuses
    (no island there, ErrorCorrection.cpp:870-931) -- at L = 100, k = 23 that is p = 23 and p = 76 -- and a read with no two
    adjacent trusted k-mers has no island at all.  Such a read is k_correct's, not even a candidate."""
    kcnt = L - k + 1
    left, right = max(0, p - k + 1), kcnt - 1 - min(p, kcnt - 1)
    return left != 1 and right != 1 and left + right >= 2


class _Plan:
    """a batch of planted reads: each is a piece of a transcript with substitutions at chosen positions, and the route, the
    number of fixes and the corrected bases it must have -- known from how it was made, not from the model"""

    def __init__(self, k, mfk=4, mode=0):
        self.k, self.mfk, self.mode = k, mfk, mode
        self.tx, self.keys, self.cnt = _transcripts(k)
        self.reads, self.truth, self.route, self.ret, self.subs = [], [], [], [], []

    def add(self, start, length, subs=(), route=None, which=0):
        """subs: positions in the read; route: None = T without and S with substitutions, else a set of allowed routes"""
        t = self.tx[which][start:start + length]
        assert len(t) == length
        r = t.copy()
        for p in subs:
            r[p] = NUC[(int(np.nonzero(NUC == r[p])[0][0]) + 1 + (p % 3)) % 4]
        self.reads.append(r.tobytes())
        self.truth.append(t.tobytes())
        self.subs.append(tuple(subs))
        if route is None:
            route = {"T"} if not subs else ({"S"} if _anchored(length, self.k, subs[0]) else {"C"})
            assert len(subs) <= 1
        self.route.append(route)
        self.ret.append(len(subs))
        return self

    def batch(self, pad_to=0):
        keys, cnt = (self.keys, self.cnt) if not pad_to else _padded(self.keys, self.cnt, self.k, pad_to)
        reads, quals = self.reads, [b"I" * len(r) for r in self.reads]
        d = dict(k=self.k, mfk=self.mfk, rate=0.01, mode=self.mode, keys=keys, counts=cnt, seqs1=reads, quals1=quals, seqs2=None, quals2=None)
        if self.mode == 1:   # reads 2u, 2u + 1 are a pair: first mates, then second mates
            d.update(seqs1=reads[0::2], quals1=quals[0::2], seqs2=reads[1::2], quals2=quals[1::2])
        return d

    def order(self):
        """plan index of every read in the device's order"""
        n = len(self.reads)
        return list(range(0, n, 2)) + list(range(1, n, 2)) if self.mode == 1 else list(range(n))


def _planted_as_made(plan, d):
    """The lookup the expectations rest on: a planted base takes exactly the windows that hold it out of the table (none of them
    recreates a k-mer of a transcript), every other window keeps its count, and no window is poly-A at 2."""
    po = _po()
    T = po.Table(d["k"], len(d["keys"]))
    T.put_many(d["keys"], d["counts"])
    P = po.make_params(d["k"], d["mfk"], d["rate"], d.get("badq", b"H"))
    k = plan.k
    for j, (r, subs) in enumerate(zip(plan.reads, plan.subs)):
        c = po.kmer_counts(P, T, r)
        hit = np.zeros(len(c), bool)
        for p in subs:
            hit[max(0, p - k + 1):p + 1] = True
        assert (c[hit] == 0).all() and (c[~hit] > 0).all() and len(set(c[~hit].tolist())) <= 1, "planted read %d: counts %s" % (j, c)
        assert not M.polya(r, k, 2).any(), "planted read %d has a poly-A window" % j


def _check_plan(plan, d, exp, got, routes, tag):
    """the routes, fix counts and bases the batch was made to have: the model's (CPU) and the device's; nothing is excused"""
    bad = []
    for i, j in enumerate(plan.order()):
        what = "read %d (planted %d: %d bases, substitutions at %s, arena offset %% 16 = %d)" % (i, j, len(plan.reads[j]), list(plan.subs[j]), _offset16(d, i))
        m = exp[i]["route"] if exp[i]["route"] != "other" else ("D" if exp[i]["cand"] else "C")
        if m not in plan.route[j]:
            bad.append("%s: the MODEL says %s, planted as %s" % (what, m, sorted(plan.route[j])))
        if routes[i] not in plan.route[j]:
            bad.append("%s: route %s, planted as %s" % (what, routes[i], sorted(plan.route[j])))
        elif routes[i] in ("T", "S") and (int(got["ret"][i]) != plan.ret[j] or got["seqs"][i] != plan.truth[j]):
            bad.append("%s: route %s with ret %d, planted %d; bases %s the transcript" % (what, routes[i], got["ret"][i], plan.ret[j], "equal" if got["seqs"][i] == plan.truth[j] else "differ from"))
    assert not bad, "%s: %d reads\n%s" % (tag, len(bad), "\n".join(bad[:12]))


def _plan_k23(mfk=4):
    """L = 100: unmodified, one substitution at every position, two and three more than k apart, four, two less than k apart"""
    pl = _Plan(23, mfk)
    lim = min(3, mfk - 1)
    pl.add(0, 100).add(250, 100).add(500, 100)
    for p in range(100):
        pl.add((37 * p) % 500, 100, [p])
    for st in (10, 130, 333):
        pl.add(st, 100, [20, 60], {"S"} if lim >= 2 else {"D"})
        pl.add(st + 5, 100, [3, 50, 96], {"S"} if lim >= 3 else {"D"})
        pl.add(st + 9, 100, [8, 36, 64, 92], {"C", "D"})
        pl.add(st + 13, 100, [40, 52], {"C", "D"})       # the model's class D: not built on the device
        pl.add(st + 17, 100, [30, 52], {"C", "D"})       # (22 apart: one stretch of k + 22 k-mers)
    return pl


# (table, what it must be): the transcripts' k-mers alone; padded to a PACKED table of >= 2^(2k-32) buckets -- k_single<false, ..>;
# padded to fewer -- the EXT instances
TABLES = {"bare": 0, "packed_ext0": 30_000, "packed_ext": 10_000}
PATHS = {"standalone": {}, "fused": {"RC_LOCALITY": "force"}}


def _assert_table_and_path(d, got, table, path, tag):
    k = d["k"]
    if table != "bare":
        assert got["layout"] == 1, tag
        assert (got["buckets"] >= 1 << (2 * k - 32)) == (table == "packed_ext0"), (tag, got["buckets"])
    probe, thr, single = got["launches"]
    if path == "fused":
        assert probe == 1 and thr == 0, "%s: the fused probe + threshold kernel did not run (%s)" % (tag, got["launches"],)
    else:
        assert probe == 1 and thr == 1, "%s: the stand-alone threshold kernel did not run (%s)" % (tag, got["launches"],)
    assert single == 1, "%s: k_single did not run" % tag


@functools.lru_cache(maxsize=None)
def _planted_case(name, pad_to=0):
    pl = PLANS[name]()
    d = pl.batch(pad_to)
    _planted_as_made(pl, d)
    exp, want = _expect(d)
    return pl, d, exp, want


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("table", list(TABLES))
def test_planted_substitutions_at_every_position_both_tables_both_threshold_kernels(monkeypatch, table, path):
    pl, d, exp, want = _planted_case("k23_mfk4", TABLES[table])
    tag = "k23_mfk4/%s/%s" % (table, path)
    got = _run(d, monkeypatch, PATHS[path])
    _assert_table_and_path(d, got, table, path, tag)
    routes = _check(d, exp, want, got, tag)
    _check_plan(pl, d, exp, got, routes, tag)
    assert routes.count("S") == 98 + 6 and routes.count("T") == 3   # (98: every position but the two of _anchored)


def _plan_lengths(k, kcnt):
    """reads of one length: unmodified, and one substitution in the middle, near either end and k-mer-aligned places between"""
    L = kcnt + k - 1
    pl = _Plan(k)
    few = kcnt < 5   # (below the floor the threshold kernel flags nothing, rc_quarter.h:568)
    which = 2 if kcnt <= 8 else 0
    tx = pl.tx[which]

    def unscreened(st):
        """the next piece that passes the screens with a letter to spare (more than L - k A's or T's: ErrorCorrection.cpp:1507-1527,
        rc_quarter.h:310 -- at kcnt = 5 that is five of either in the whole read)"""
        for s in list(range(st, 600 - L + 1)) + list(range(st)):
            if max(int((tx[s:s + L] == 65).sum()), int((tx[s:s + L] == 84).sum())) < L - k:
                return s
        raise AssertionError("no piece of %d bases passes the screens" % L)
    for st in (0, 101, 600 - L):
        pl.add(unscreened(st), L, which=which)
        for p in sorted({L // 2, 0, L - 1, min(k, L - 1), max(L - 1 - k, 0), min(16 * (kcnt // 16), L - 1)}):
            pl.add(unscreened((st + 31 * p) % (600 - L + 1)), L, [p], {"C"} if few else None, which=which)
    return pl


def _plan_ragged():
    """every read 0 modulo 16 bases long, so read i starts at arena offset i modulo 16: offsets 0..15 each hold two reads that
    must be T and four that must be S, their substitution in the middle of each quarter of the read -- the k-mers k_single
    cuts out of the staged words for a stretch span 2 k - 1 bases, more than a quarter, so every staged base of every
    alignment is read by some stretch"""
    pl = _Plan(23)
    for i in range(96):
        L, g = (64, 80, 96, 112, 128, 144, 160)[i % 7], i // 16
        p = (2 * g + 1) * L // 8
        while not _anchored(L, 23, p):
            p += 1
        pl.add((53 * i) % (600 - L), L, [p] if g < 4 else [])
    return pl


def _plan_sizes(n):
    pl = _Plan(23)
    for i in range(n):
        if i % 3 == 1:   # two stretches more than k apart
            pl.add((41 * i) % 500, 100, [(5 * i) % 30, 60 + (3 * i) % 40], {"S"})
        else:
            pl.add((41 * i) % 500, 100, [] if i % 3 == 2 else [(7 * i) % 100])
    return pl


def _plan_pairs(mode):
    """pairs whose second mate is cut from the count-8 transcript: the pair's threshold (pair_t, ErrorCorrection.cpp:832-842)
    replaces the first mate's s and t; pairs of the same transcript; a substitution in the first mate, the second, both, neither"""
    pl = _Plan(23, mode=mode)
    for u in range(24):
        low = u % 2 == 0
        a = [(13 * u + 5) % 100] if u % 4 < 2 else []
        b = [(29 * u + 40) % 100] if u % 8 >= 4 else []
        pl.add((17 * u) % 500, 100, a)
        pl.add((23 * u + 9) % 500, 100, b, which=1 if low else 0)
    return pl


PLANS = {"k23_mfk4": _plan_k23, "k23_mfk3": lambda: _plan_k23(3), "k23_mfk2": lambda: _plan_k23(2), "ragged": _plan_ragged,
         "pairs_1": lambda: _plan_pairs(1), "pairs_2": lambda: _plan_pairs(2), "pairs_0": lambda: _plan_pairs(0)}
for _n in (1, 3, 15, 16, 17, 65):
    PLANS["size_%d" % _n] = functools.partial(_plan_sizes, _n)
# kcnt: the floor (4: nothing is flagged; 5), and either side of the EC = 8 / 9 / 10 register layouts (128 | 129, 144 | 145).  At
# k = 23 a read of 160 bases has 138 k-mers, so 143..146 are reached at k = 15
for _k, _c in [(23, 4), (23, 5), (23, 127), (23, 128), (23, 129), (23, 138), (15, 127), (15, 128), (15, 129), (15, 143), (15, 144), (15, 145), (15, 146),
               (16, 145), (17, 144)]:   # (the last two with the (15, 146): 160 bases at k = 15, 16, 17, the pe_160_k15 shape)
    PLANS["k%d_kcnt%d" % (_k, _c)] = functools.partial(_plan_lengths, _k, _c)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", [n for n in PLANS if n not in ("k23_mfk4",)])
def test_planted_reads_take_the_route_they_were_made_for(monkeypatch, name, path):
    pl, d, exp, want = _planted_case(name)
    tag = "%s/%s" % (name, path)
    got = _run(d, monkeypatch, PATHS[path])
    probe, thr, single = got["launches"]
    assert (thr == 0) == (path == "fused") and single == (1 if pl.mfk >= 2 else 0), (tag, got["launches"])
    routes = _check(d, exp, want, got, tag)
    _check_plan(pl, d, exp, got, routes, tag)
    if name in ("pairs_1", "pairs_2"):   # the mate's lower threshold did replace s (and t follows it): 8 for 50
        low = [i for i, j in enumerate(pl.order()) if j % 2 == 0 and (j // 2) % 2 == 0]
        assert len(low) == 12
        for i in low:
            (s, t), (s_own, t_own) = exp[i]["thresholds"], exp[i]["own_thresholds"]
            assert s == 8 and s_own == 50 and t <= t_own, (i, s, t, s_own, t_own)
        assert {len(pl.subs[pl.order()[i]]) for i in low} == {0, 1}
    if name == "ragged":
        for r in ("S", "T"):
            assert {_offset16(d, i) for i in range(len(routes)) if routes[i] == r} == set(range(16)), r
    if "kcnt" in name and "kcnt4" not in name:
        assert routes.count("S") >= 6 and routes.count("T") == 3


def test_without_k_single_every_isolated_substitution_is_a_declined_candidate(monkeypatch):
    """RC_NO_SINGLE=1: the candidates are flagged and nobody finishes them -- no S, and D exactly where S was expected; the
    threshold kernel's reads stay T.  (So the routes above do tell k_single's work from k_correct's.)"""
    pl, d, exp, want = _planted_case("k23_mfk4")
    got = _run(d, monkeypatch, {"RC_NO_SINGLE": "1"})
    assert got["launches"][2] == 0
    routes = _check(d, exp, want, got, "k23_mfk4/RC_NO_SINGLE", no_single=True)
    assert routes.count("S") == 0 and routes.count("T") == 3
    for i, e in enumerate(exp):
        assert (routes[i] == "D") == (e["route"] == "S" or (e["cand"] and e["route"] == "other")), i
    assert sum(e["route"] == "S" for e in exp) == 104


# ---- (d) the project's own data ----------------------------------------------------------------------------------------

def _first_units(d, units=600):
    d = dict(d)
    if d["mode"] == 1:
        for kk in ("seqs1", "quals1", "seqs2", "quals2"):
            d[kk] = d[kk][:units]
    else:
        n = units * (2 if d["mode"] == 2 else 1)
        d["seqs1"], d["quals1"] = d["seqs1"][:n], d["quals1"][:n]
    return d


@functools.lru_cache(maxsize=None)
def _data_case(name):
    d = _first_units(datasets.make(name))
    exp, want = _expect(d)
    return d, exp, want


@pytest.mark.parametrize("name", ["se_k23", "pe_k23", "il_k23", "skew", "k11", "k32", "pe_151", "pe_160_k15", "polya_k23", "k15", "qv_mixed_pe/high"])
def test_routes_of_the_data_sets_equal_the_model(monkeypatch, name):
    d, exp, want = _data_case(name)
    n = len(exp)
    accepted = sum(e["route"] != "other" for e in exp)
    changed = sum(e["route"] == "S" for e in exp)
    assert accepted > 0.05 * n, (name, accepted)          # (the floors of tests/test_k2s_model.py: the model is not vacuous here)
    if name in ("skew", "k11", "pe_k23"):
        assert changed > 0.02 * n, (name, changed)
    got = _run(d, monkeypatch)
    routes = _check(d, exp, want, got, name)
    assert routes.count("S") == changed and routes.count("T") == accepted - changed


# ---- (e) the hook's refusals ---------------------------------------------------------------------------------------------

def test_debug_routes_refuses_what_it_cannot_describe(monkeypatch):
    import rcorrector_amd
    po = _po()
    pl = _Plan(23).add(0, 100).add(50, 100, [40]).add(100, 161, [80])
    d = pl.batch()
    ctx = rcorrector_amd.Context(k=23, max_fix_per_k=4, device=0)
    try:
        ctx.table_build(d["keys"], d["counts"])
        ctx.set_run_params(0.01, b"H")
        with pytest.raises(rcorrector_amd.RcorrectorError, match="no batch has run"):
            ctx.debug_routes(2)

        def go(reads):
            a, off = po.pack_reads(reads)
            qa, _ = po.pack_reads([b"I" * len(r) for r in reads])
            ctx.correct_batch(0, a, qa, off)
            return po.unpack_reads(a, off)
        assert go(pl.reads[:2]) == pl.truth[:2]
        with pytest.raises(rcorrector_amd.RcorrectorError, match="n = 3, the last batch had 2 reads"):
            ctx.debug_routes(3)
        cls, cand, runs = ctx.debug_routes(2)
        assert [_route(int(c), int(f)) for c, f in zip(cls, cand)] == ["T", "S"] and _stretches(runs[1]) == (1, [(18, 40)])
        go(pl.reads)     # the 161-base read: two length tiers
        with pytest.raises(rcorrector_amd.RcorrectorError, match="length tiers"):
            ctx.debug_routes(3)
        assert go(pl.reads[:2]) == pl.truth[:2]
        assert ctx.debug_routes(2)[0].tolist() == [0, 0]
    finally:
        ctx.close()
