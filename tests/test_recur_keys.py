"""CPU: the recurrence census's site keys (rcorrector_amd/csrc/rc_recur.h, what a lane of k_change_keys computes) as a host
program -- tests/hostmath/recur_key.cpp -- held to the pure-Python model (tests/recur_model.py), and the data set the GPU
tests run on (tests/recur_data.py) held, on the oracle, to the conditions that make those tests mean something.  The host
program is built and run twice: plain, and as a stand-alone program with AddressSanitizer + UndefinedBehaviorSanitizer
(every string is read from a heap block of exactly its bytes)."""
import collections
import os
import random
import subprocess

import pytest

import recur_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostmath", "recur_key.cpp")
FLAGS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(FLAGS))
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("recur_key_" + request.param) / "recur_key")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + FLAGS[request.param] + ["-I", os.path.join(ROOT, "rcorrector_amd", "csrc"), SRC, "-o", out],
                   check=True)
    return out


def keys_of(exe, pairs):
    """[(changes, contexted, [keys in position order])] per (before, after)"""
    p = subprocess.run([exe, "keys"], input=("".join("%s\t%s\n" % ba for ba in pairs)).encode(), stdout=subprocess.PIPE, check=True)  # (run directly: nothing preloaded)
    out = []
    for line in p.stdout.decode().splitlines():
        w = line.split()
        out.append((int(w[0]), int(w[1]), [int(x, 16) for x in w[2:]]))
    assert len(out) == len(pairs)
    return out


def model_of(pairs):
    out = []
    for b, a in pairs:
        ch = rm.read_changes(b, a)
        out.append((len(ch), sum(1 for _, k in ch if k is not None), [k for _, k in ch if k is not None]))
    return out


def rand_read(rng, L):
    return "".join(rng.choice("ACGT") for _ in range(L))


def change(s, p, to=None):
    to = to or {"A": "C", "C": "G", "G": "T", "T": "A"}.get(s[p], "A")
    return s[:p] + to + s[p + 1:]


def test_self_test_of_the_arithmetic(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("ok "), out
    assert int(out.split()[1]) > 1000000


def test_model_reverse_complement_is_an_involution_without_fixed_points():
    rng = random.Random(5)
    for _ in range(2000):
        w = rand_read(rng, rm.WINDOW)
        assert rm.revcomp(rm.revcomp(w)) == w and rm.revcomp(w) != w
        for orig in "ACGTNa":
            twin_orig = rm.COMP.get(orig, orig)
            assert rm.key_of(w, orig) == rm.key_of(rm.revcomp(w), twin_orig)
            f, to, text = rm.decode(rm.key_of(w, orig))
            assert text in (w, rm.revcomp(w)) and to == text[rm.FLANK]
            assert f == ("N" if orig not in "ACGT" else (orig if text == w else rm.COMP[orig]))


def test_host_program_against_the_model(exe):
    rng = random.Random(11)
    pairs = []
    # every length 0..70 and a few long ones, a change at the edges of the contexted range and at both ends
    for L in list(range(0, 71)) + [255, 256, 257, 1023]:
        a = rand_read(rng, L)
        pairs.append((a, a))
        for p in sorted({0, 13, 14, L - 15, L - 14, L - 1, L // 2}):
            if 0 <= p < L:
                pairs.append((change(a, p), a))
        if L:
            pairs.append(("".join(change(a, p)[p] for p in range(L)), a))   # every base changed
    # adjacent changes, N / lower case in the window and as the original byte
    for _ in range(200):
        L = rng.randrange(29, 120)
        a = rand_read(rng, L)
        b = a
        for p in rng.sample(range(L), rng.randrange(1, 6)):
            b = change(b, p, rng.choice(["N", "a", "c", "g", "t", "n", None, None, None]))
        p = rng.randrange(L - 1)
        b = change(change(b, p), p + 1)
        if rng.random() < 0.5:
            q = rng.randrange(L)
            a2 = a[:q] + rng.choice("Nacgtn") + a[q + 1:]     # the corrected read holds a letter outside ACGT
            pairs.append((b, a2))
        pairs.append((b, a))
    got, want = keys_of(exe, pairs), model_of(pairs)
    for g, w, ba in zip(got, want, pairs):
        assert g == w, ba


def test_edges_letters_and_twins(exe):
    rng = random.Random(3)
    L = 60
    a = rand_read(rng, L)
    res = keys_of(exe, [(change(a, p), a) for p in (13, 14, L - 15, L - 14)])
    assert [r[:2] for r in res] == [(1, 0), (1, 1), (1, 1), (1, 0)]
    # L < 29: no keys, whatever changes
    for Ls in (1, 14, 28):
        s = rand_read(rng, Ls)
        assert keys_of(exe, [("".join(change(s, p)[p] for p in range(Ls)), s)])[0] == (Ls, 0, [])
    # L == 29: the centre alone is contexted
    s = rand_read(rng, 29)
    assert [r[:2] for r in keys_of(exe, [(change(s, p), s) for p in (13, 14, 15)])] == [(1, 0), (1, 1), (1, 0)]
    # an N or a lower-case letter anywhere in the window clips the change; outside it, it does not
    p = 30
    for q in range(L):
        for bad in "Nn" + a[q].lower():
            a2 = a[:q] + bad + a[q + 1:]
            if q == p:
                continue
            r = keys_of(exe, [(change(a2, p), a2)])[0]
            assert r[:2] == (1, 0 if abs(q - p) <= 14 else 1), (q, bad)
    # the original byte: N / lower case give from = 4; the twin of a change is the same site
    for orig in "ACGTNacgtn":
        if orig == a[p]:
            continue
        b = change(a, p, orig)
        k = keys_of(exe, [(b, a)])[0][2][0]
        assert rm.decode(k)[0] == ("N" if orig not in "ACGT" else rm.decode(rm.key_of(a[p - 14:p + 15], orig))[0])
        if orig in "ACGT":
            twin = keys_of(exe, [(rm.revcomp(b), rm.revcomp(a))])[0]
            assert twin == (1, 1, [k])
        else:
            assert k & 7 == 4


@pytest.fixture(scope="module")
def oracle_runs():
    import datasets
    import recur_data
    from oracle import pyoracle as po
    po.build()
    out = {}
    for mode in (0, 1, 2):
        d = recur_data.make(mode)
        res = datasets.run_oracle(po, d)
        off = po.pack_reads(d["seqs1"])[1]
        outs = [res[4][off[i]:off[i + 1] - 1].tobytes() for i in range(len(off) - 1)]
        if mode == 1:
            off2 = po.pack_reads(d["seqs2"])[1]
            outs += [res[5][off2[i]:off2[i + 1] - 1].tobytes() for i in range(len(off2) - 1)]
        out[mode] = (recur_data.all_reads(d), outs)
    return out


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_the_data_set_recurs_on_the_oracle(oracle_runs, mode):
    """Conditions on the INPUT of the GPU tests, not tolerances: a site corrected at least eight times from reads of both
    orientations, at least 20 singleton sites, a clipped change, a change from a letter outside ACGT."""
    ins, outs = oracle_runs[mode]
    C = rm.Census().add(ins, outs)
    orient = collections.defaultdict(set)
    from4 = 0
    for b, a in zip(ins, outs):
        b, a = b.decode(), a.decode()
        for p, key in rm.read_changes(b, a):
            from4 += rm.from_code(b[p]) == 4
            if key is not None:
                w = a[p - rm.FLANK:p + rm.FLANK + 1]
                orient[key].add(rm.pack(w) < rm.pack(rm.revcomp(w)))
    assert any(c >= 8 and len(orient[k]) == 2 for k, c in C.keys.items())
    assert sum(1 for c in C.keys.values() if c == 1) >= 20
    assert C.changes - C.contexted >= 1
    assert from4 >= 1
