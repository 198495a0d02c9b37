"""CPU: the mate-overlap report without a GPU.  `brute` is a plain numpy restatement of the report's definitions
(include/rcorrector_amd.h: rc_mate_overlap), which the GPU tests use too; the word arithmetic of rc_overlap.h, run lane by lane
by tests/hostmath/mate_overlap.cpp, must equal it on pairs built for the edges; the report file's text comes from a host unit
and is checked against a hand-written one; the wrapper passes the three flags through."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = ("pairs", "overlapping", "compared_before", "disagree_before", "compared_after", "disagree_after", "resolved", "introduced", "kept",
           "pairs_improved", "pairs_worsened", "pairs_same")
ARRAYS = ("frag", "compared5", "disagree5_before", "disagree5_after")
_COMP = np.zeros(256, np.uint8)
for _x, _y in zip(b"ACGT", b"TGCA"):
    _COMP[_x] = _y
_VALID = np.zeros(256, bool)
_VALID[list(b"ACGT")] = True


def revcomp(b):
    """r[j] = comp(b[Lb - 1 - j]); a byte that is no upper-case ACGT becomes 0 (invalid)"""
    return _COMP[np.frombuffer(bytes(b), np.uint8)[::-1]]


def faced(a, r, d):
    """(positions i of a that face r[i - d], both valid there, differ there)"""
    La, Lb = len(a), len(r)
    i = np.arange(max(0, d), min(La, d + Lb))
    x, y = a[i], r[i - d]
    both = _VALID[x] & _VALID[y]
    return i, both, both & (x != y)


def choose(a, r, min_overlap, pct):
    """d*: the accepted offset with the largest v, then the smallest m, then the smallest d; None if there is none"""
    best = None
    for d in range(-(len(r) - 1), len(a)):
        _, both, dif = faced(a, r, d)
        v, m = int(both.sum()), int(dif.sum())
        if v >= min_overlap and 100 * m <= pct * v and (best is None or (v, -m, -d) > (best[0], -best[1], -best[2])):
            best = (v, m, d)
    return None if best is None else best[2]


def brute(pairs, min_overlap=30, pct=10):
    """pairs: (a before, b before, a after, b after) byte strings -> the counts of an rc_mate_overlap, and under "_extra" what
    the struct does not hold: `lost`, the faced positions that differ before and are invalid after (the third term of the fourth
    identity), and how many faced positions hold an N that became a base / a base that became its lower-case letter"""
    out = {n: 0 for n in SCALARS}
    extra = out["_extra"] = dict(lost=0, n_to_base=0, base_to_lower=0)
    out["frag"] = np.zeros(2048, np.uint64)
    for n in ARRAYS[1:]:
        out[n] = np.zeros((2, 1024), np.uint64)
    for a0, b0, a1, b1 in pairs:
        out["pairs"] += 1
        a0, a1 = (np.frombuffer(bytes(x), np.uint8) for x in (a0, a1))
        r0, r1 = revcomp(b0), revcomp(b1)
        d = choose(a0, r0, min_overlap, pct)
        if d is None:
            continue
        Lb = len(r0)
        i, vb, xb = faced(a0, r0, d)
        _, va, xa = faced(a1, r1, d)
        out["overlapping"] += 1
        out["frag"][d + Lb] += 1
        out["compared_before"] += int(vb.sum())
        out["disagree_before"] += int(xb.sum())
        out["compared_after"] += int(va.sum())
        out["disagree_after"] += int(xa.sum())
        out["resolved"] += int((xb & va & ~xa).sum())
        out["introduced"] += int((vb & ~xb & xa).sum())
        out["kept"] += int((xb & xa).sum())
        extra["lost"] += int((xb & ~va).sum())
        for s0, s1 in ((a0[i], a1[i]), (np.frombuffer(bytes(b0), np.uint8)[Lb - 1 - (i - d)], np.frombuffer(bytes(b1), np.uint8)[Lb - 1 - (i - d)])):
            extra["n_to_base"] += int(((s0 == ord("N")) & _VALID[s1]).sum())
            extra["base_to_lower"] += int((_VALID[s0] & (s1 == s0 + 32)).sum())
        ma, mb = int(xa.sum()), int(xb.sum())
        out["pairs_improved" if ma < mb else "pairs_worsened" if ma > mb else "pairs_same"] += 1
        p2 = Lb - 1 - (i - d)
        for name, sel in (("compared5", vb), ("disagree5_before", xb), ("disagree5_after", xa)):
            np.add.at(out[name][0], i[sel], 1)
            np.add.at(out[name][1], p2[sel], 1)
    return out


def check_identities(c, lost=None):
    """lost: the positions that differ before and are invalid after, where the caller knows them (the restatement counts them)"""
    if lost is None and "_extra" in c:
        lost = c["_extra"]["lost"]
    assert int(c["frag"].sum()) == c["overlapping"] == c["pairs_improved"] + c["pairs_worsened"] + c["pairs_same"]
    assert int(c["compared5"][0].sum()) == int(c["compared5"][1].sum()) == c["compared_before"]
    assert int(c["disagree5_before"][0].sum()) == int(c["disagree5_before"][1].sum()) == c["disagree_before"]
    assert int(c["disagree5_after"][0].sum()) == int(c["disagree5_after"][1].sum()) == c["disagree_after"]
    if lost is None:
        assert c["disagree_before"] >= c["resolved"] + c["kept"]
    else:
        assert c["disagree_before"] == c["resolved"] + c["kept"] + lost
    assert c["frag"][0] == 0 and c["frag"][2047] == 0


def assert_equal_counts(got, want, what=""):
    for n in SCALARS:
        assert int(got[n]) == int(want[n]), "%s %s: got %d, want %d" % (what, n, got[n], want[n])
    for n in ARRAYS:
        g, w = np.asarray(got[n]).astype(np.uint64), np.asarray(want[n]).astype(np.uint64)
        assert np.array_equal(g, w), "%s %s differs at %s" % (what, n, np.argwhere(g != w)[:5].tolist())


# ---- pairs built for the edges ------------------------------------------------------------------------------------------------
def _rc(s):
    return bytes(revcomp(s)).replace(b"\0", b"N")


def _rand(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n))


def _mut(s, pos):
    s = bytearray(s)
    for p in pos:
        s[p] = b"ACGT"[(b"ACGT".index(s[p]) + 1) % 4]
    return bytes(s)


def pair_from_fragment(rng, F, La, Lb):
    """mate 1 = the first La bases of a random fragment of F bases, mate 2 = the reverse complement of its last Lb (F >= La, Lb)"""
    f = _rand(rng, F)
    return f[:La], _rc(f[F - Lb:])


def edge_pairs(rng, max_len=1023, min_overlap=30, pct=10):
    """(a, b) pairs: every length class, d* < 0, = 0, containment, the shortest accepted overlap and one below, the mismatch cap
    met exactly and passed by one, N and lower case inside and at the ends, repeats where the tie rule decides, a short exact
    overlap beside a longer one just over the cap"""
    P = []
    lens = [n for n in (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023) if n <= max_len]
    for La in lens:                                   # La != Lb, the overlap as long as the shorter mate allows
        for Lb in (lens[(lens.index(La) + 3) % len(lens)], max(0, La - 1)):
            ov = min(La, Lb)
            F = La + Lb - ov
            P.append(pair_from_fragment(rng, F, La, Lb) if F else (b"", b""))
    for La, Lb, F in ((100, 90, 60), (100, 90, 100), (120, 50, 120), (50, 120, 120), (150, 150, 220), (64, 64, 64), (33, 65, 70)):
        P.append(pair_from_fragment(rng, F, La, Lb))  # read-through (F < La), d* = 0, one mate inside the other
    for La, Lb in ((80, 70), (64, 33), (150, 151)):   # v exactly min_overlap (F = La + Lb - min_overlap), and one below
        P.append(pair_from_fragment(rng, La + Lb - min_overlap, La, Lb))
        P.append(pair_from_fragment(rng, La + Lb - min_overlap + 1, La, Lb))
    for ov in (40, 100):                              # 100 m == pct v exactly, and one mismatch more
        La = Lb = 120
        a, b = pair_from_fragment(rng, La + Lb - ov, La, Lb)
        m = pct * ov // 100
        pos = [La - ov + int(q) for q in rng.choice(ov, size=m + 1, replace=False)]
        P += [(_mut(a, pos[:m]), b)] * 2              # (twice: `corrected` edits the before version of every other pair)
        P.append((_mut(a, pos), b))
    # N / lower case inside and at the ends of a 60-base overlap: a[40 + w] faces b[99 - w], w = 0 .. 59; (mate, w, N?)
    for where in (((0, 0, 0),), ((0, 59, 0),), ((0, 20, 1), (1, 21, 1), (0, 40, 0), (1, 41, 0)), ((0, 0, 1),), ((0, 59, 1),), ((1, 0, 1),), ((1, 59, 1),),
                  ((0, 0, 1), (1, 59, 1)), ((1, 0, 0), (1, 59, 0)), ((0, 0, 1), (0, 1, 1), (1, 58, 1), (1, 59, 1))):
        a, b = (bytearray(x) for x in pair_from_fragment(rng, 140, 100, 100))
        for mate, w, is_n in where:
            s, p = (b, 99 - w) if mate else (a, 40 + w)
            s[p] = ord("N") if is_n else s[p] + 32
        P.append((bytes(a), bytes(b)))
    for unit, La, Lb in ((b"A", 80, 70), (b"AC", 90, 90), (b"ACG", 64, 100), (b"T", 40, 40)):  # many offsets tie
        P.append(((unit * 200)[:La], _rc((unit * 200)[:Lb])))
    # a short exact overlap (35 bases at the end of a) beside a longer one (70 bases) that is just over the cap
    a, b = pair_from_fragment(rng, 130, 100, 100)
    a = _mut(a, [30 + int(q) for q in rng.choice(70, size=pct * 70 // 100 + 1, replace=False)])
    tail = _rc(b)[:35]
    P.append((a[:100 - 35] + tail, b))
    P.append((_rand(rng, 100), _rand(rng, 100)))      # no overlap at all
    return P


def arena_of(reads, lead=0):
    """NUL-terminated reads behind `lead` bytes of padding -> (arena bytes, offsets[n + 1])"""
    off = np.zeros(len(reads) + 1, np.uint32)
    buf = bytearray(b"#" * lead)
    for i, r in enumerate(reads):
        off[i] = len(buf) - lead
        buf += bytes(r) + b"\0"
    off[len(reads)] = len(buf) - lead
    return bytes(buf), off


# ---- the word arithmetic, lane by lane -----------------------------------------------------------------------------------------
def run_host(tmp_path, pairs4, min_overlap, pct, nw, flags=("-O2",)):
    exe = str(tmp_path / ("mate_overlap_%d" % len(flags)))
    if not os.path.exists(exe):
        subprocess.run(["g++", "-std=c++17", "-Wall"] + list(flags) + ["-I", os.path.join(ROOT, "rcorrector_amd", "csrc"),
                                                                      os.path.join(ROOT, "tests", "hostmath", "mate_overlap.cpp"), "-o", exe], check=True)
    path = str(tmp_path / "pairs.txt")
    with open(path, "wb") as f:
        for four in pairs4:
            for s in four:
                f.write(b"=" + bytes(s) + b"\n")
    p = subprocess.run([exe, path, str(min_overlap), str(pct), str(nw)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()
    got = {"frag": np.zeros(2048, np.uint64)}
    for n in ARRAYS[1:]:
        got[n] = np.zeros((2, 1024), np.uint64)
    for ln in p.stdout.decode().splitlines():
        t = ln.split()
        if t[0] == "tot":
            got.update({n: int(v) for n, v in zip(SCALARS, t[1:])})
        elif t[0] == "frag":
            got["frag"][int(t[1])] = int(t[2])
        else:
            for n, v in zip(ARRAYS[1:], t[3:]):
                got[n][int(t[1]), int(t[2])] = int(v)
    return got


def corrected(rng, pairs):
    """a second version of every pair: a few random substitutions; then, not left to chance, every N turned into a base and, in
    every fourth pair, the base 5 from mate 1's 3' end and the base 7 from mate 2's (inside any overlap of 30) turned into lower
    case -- the "after" version of the even pairs (disagreements introduced, N -> base, base -> lower case) and the "before"
    version of the odd ones (resolved, base -> N, lower case -> base)"""
    out = []
    for n, (a, b) in enumerate(pairs):
        a2, b2 = bytearray(a), bytearray(b)
        for s in (a2, b2):
            for p in rng.choice(len(s), size=min(len(s), 3), replace=False) if len(s) else []:
                s[p] = b"ACGT"[int(rng.integers(4))]
        for s0, s, back in ((a, a2, 5), (b, b2, 7)):
            for p in range(len(s0)):
                if s0[p] == ord("N"):
                    s[p] = b"ACGT"[p % 4]
            if n % 4 == 0 and len(s0) >= 40 and s0[len(s0) - back] in b"ACGT":
                s[len(s0) - back] = s0[len(s0) - back] + 32
        out.append((a, b, bytes(a2), bytes(b2)) if n % 2 == 0 else (bytes(a2), bytes(b2), a, b))
    # built, not drawn (a[40 + w] faces b[99 - w]): a disagreement whose base becomes lower case (in neither of resolved / kept),
    # an N of mate 1 and one of mate 2 that become the right base, and one that becomes a wrong base
    a, b = pair_from_fragment(rng, 140, 100, 100)
    low = lambda s, p: s[:p] + bytes([s[p] + 32]) + s[p + 1:]   # noqa: E731
    enn = lambda s, p: s[:p] + b"N" + s[p + 1:]                 # noqa: E731
    out.append((_mut(a, [50]), b, low(_mut(a, [50]), 50), b))
    out.append((a, _mut(b, [30]), a, low(_mut(b, [30]), 30)))
    out.append((enn(a, 60), enn(b, 20), a, b))
    out.append((enn(a, 99), enn(b, 99), _mut(a, [99]), _mut(b, [99])))
    return out


def assert_fixture_has_the_named_changes(want, pct=10):
    """the restatement saw, at faced positions, an N that became a base, a base that became lower case, and -- where an accepted
    offset may have a mismatch at all -- a disagreement whose position is invalid afterwards"""
    e = want["_extra"]
    assert e["n_to_base"] >= 2 and e["base_to_lower"] >= 2 and (e["lost"] >= 1 or pct == 0), e


def test_the_edge_pairs_hold_what_they_are_named_for():
    rng = np.random.default_rng(12)
    P = edge_pairs(rng, 256)
    ends = {(m, e): 0 for m in (0, 1) for e in (0, 1)}       # pairs whose chosen overlap starts / ends on an N of mate 1 / mate 2
    lower_end = 0
    for a, b in P:
        x, r = np.frombuffer(a, np.uint8), revcomp(b)
        d = choose(x, r, 30, 10)
        if d is None:
            continue
        i, _, _ = faced(x, r, d)
        raw_b = np.frombuffer(b, np.uint8)[len(b) - 1 - (i - d)]
        for m, s in ((0, x[i]), (1, raw_b)):
            ends[m, 0] += int(s[0] == ord("N"))
            ends[m, 1] += int(s[-1] == ord("N"))
            lower_end += int(s[0] >= 97) + int(s[-1] >= 97)
    assert all(v >= 1 for v in ends.values()), ends
    assert lower_end >= 4
    c = brute(corrected(rng, P))
    assert_fixture_has_the_named_changes(c)
    check_identities(c)


def test_an_n_that_becomes_a_base_and_a_base_that_becomes_lower_case_by_hand():
    f = b"ACGTTGCAAGGCTTAACCGGATATCGCGTTAAGGCCATGCTA"         # 42 bases; a = f[:37], overlap = a[5:37], 32 bases, d* = 5
    a, b = bytearray(f[:37]), _rc(f[5:])
    a_n = bytes(a[:10] + b"N" + a[11:])
    c = brute([(a_n, b, bytes(a), b)])                          # N -> the right base: compared grows, nothing else
    assert (c["compared_before"], c["compared_after"], c["disagree_before"], c["disagree_after"]) == (31, 32, 0, 0)
    assert (c["resolved"], c["kept"], c["introduced"], c["pairs_same"]) == (0, 0, 0, 1) and c["compared5"][0][10] == 0
    c = brute([(a_n, b, _mut(a, [10]), b)])                     # N -> a wrong base: a disagreement after, but not "introduced"
    assert (c["disagree_after"], c["introduced"], c["pairs_worsened"], c["disagree5_after"][0][10]) == (1, 0, 1, 1)
    a_err = _mut(a, [10])
    a_low = bytes(a_err[:10]) + bytes([a_err[10] + 32]) + bytes(a_err[11:])
    c = brute([(a_err, b, a_low, b)])                           # a differing base -> lower case: neither resolved nor kept
    assert (c["disagree_before"], c["disagree_after"], c["resolved"], c["kept"], c["compared_after"]) == (1, 0, 0, 0, 31)
    assert c["_extra"] == dict(lost=1, n_to_base=0, base_to_lower=1) and c["pairs_improved"] == 1
    check_identities(c)


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "asan_ubsan"])
def test_the_word_arithmetic_equals_the_restatement(flags, tmp_path):
    rng = np.random.default_rng(5)
    for nw, max_len, mo, pct in ((32, 1023, 30, 10), (8, 256, 30, 10), (32, 1023, 1, 0), (8, 256, 17, 50)):
        pairs4 = corrected(rng, edge_pairs(rng, max_len, mo, pct))
        want = brute(pairs4, mo, pct)
        check_identities(want)
        assert want["overlapping"] > 20 and want["overlapping"] < want["pairs"]
        assert_fixture_has_the_named_changes(want, pct)
        assert_equal_counts(run_host(tmp_path, pairs4, mo, pct, nw, flags), want, "nw %d min %d pct %d:" % (nw, mo, pct))


def test_a_mate_longer_than_the_instance_is_cut_not_indexed_outside(tmp_path):
    rng = np.random.default_rng(6)
    pairs = [pair_from_fragment(rng, 500, 400, 300), pair_from_fragment(rng, 280, 270, 260)]
    got = run_host(tmp_path, [(a, b, a, b) for a, b in pairs], 30, 10, 8, ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert_equal_counts(got, brute([(a[:256], b[:256], a[:256], b[:256]) for a, b in pairs]), "cut to 256:")


def test_the_restatement_on_a_pair_worked_by_hand():
    f = b"ACGTTGCAAGGCTTAACCGGATATCGCGTTAAGGCCATGC"           # 40 bases
    a, b = f[:35], _rc(f[5:])                                  # both 35 long, overlap 30, d* = 5, F = 40
    c = brute([(a, b, a, b)])
    assert c["overlapping"] == 1 and c["frag"][40] == 1 and c["compared_before"] == 30 and c["disagree_before"] == 0
    assert np.array_equal(np.nonzero(c["compared5"][0])[0], np.arange(5, 35)) and np.array_equal(np.nonzero(c["compared5"][1])[0], np.arange(5, 35))
    a_err = _mut(a, [10])                                      # an error in mate 1, corrected: resolved
    c = brute([(a_err, b, a, b)])
    assert (c["disagree_before"], c["disagree_after"], c["resolved"], c["kept"], c["introduced"], c["pairs_improved"]) == (1, 0, 1, 0, 0, 1)
    assert c["disagree5_before"][0][10] == 1 and c["disagree5_before"][1][35 - 1 - (10 - 5)] == 1
    c = brute([(a, b, a_err, b)])                              # a miscorrection: introduced
    assert (c["disagree_before"], c["disagree_after"], c["resolved"], c["kept"], c["introduced"], c["pairs_worsened"]) == (0, 1, 0, 0, 1, 1)
    assert brute([(a[:34], b, a[:34], b)])["overlapping"] == 0  # 29 faced bases: one below min_overlap


# ---- the report file's text --------------------------------------------------------------------------------------------------
def test_the_report_text_is_the_documented_one(tmp_path):
    import test_hostmain as th
    exe = str(tmp_path / "overlap_text")
    th.build_host_test(os.path.join(ROOT, "tests", "hostmain", "overlap_text.cpp"), exe)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    want = ("min_overlap\t30\nmax_mismatch_pct\t10\npairs\t1000\noverlapping\t900\ncompared\tbefore\t72000\ncompared\tafter\t72001\n"
            "disagree\tbefore\t700\ndisagree\tafter\t90\nresolved\t620\nkept\t78\nintroduced\t12\npairs\timproved\t500\npairs\tworsened\t9\n"
            "pairs\tsame\t391\nfrag\t1\t3\nfrag\t220\t890\nfrag\t2046\t7\npos5\t1\t0\t5\t0\t0\npos5\t1\t149\t800\t9\t2\npos5\t2\t1023\t4\t4\t3\n"
            "sum\tpairs\t2000\tfrag220\t1780\tmin_overlap\t30\n")
    assert p.returncode == 0 and p.stdout.decode() == want, p.stdout.decode()


# ---- the wrapper ---------------------------------------------------------------------------------------------------------------
def test_run_rcorrector_gpu_passes_the_flags_through(tmp_path):
    fake = tmp_path / "rcorrector"
    fake.write_text("#!/bin/sh\necho \"$@\" > %s/args.txt\n" % tmp_path)
    fake.chmod(0o755)
    fq = tmp_path / "r_1.fq"
    fq.write_text("@r\nACGT\n+\nIIII\n")
    env = dict(os.environ, RCORRECTOR_BIN=str(fake))
    wrapper = os.path.join(ROOT, "tools", "run_rcorrector_gpu")
    p = subprocess.run([sys.executable, wrapper, "-1", str(fq), "-2", str(fq), "-od", str(tmp_path), "-overlap", "ov.txt", "-overlap-min", "25",
                        "-overlap-mm", "5"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=str(tmp_path), timeout=120)
    assert p.returncode == 0, p.stdout.decode()
    args = (tmp_path / "args.txt").read_text().split()
    for flag, val in (("-overlap", "ov.txt"), ("-overlap-min", "25"), ("-overlap-mm", "5")):
        assert args[args.index(flag) + 1] == val
    assert "-overlap FILE" in open(wrapper).read()
