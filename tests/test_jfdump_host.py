"""CPU: the k-mer dump's text on the host alone -- rc_jfdump.cpp's whole-file read, cut, parser (fast path + general tokeniser),
join, ERROR_RATE scan length and writer -- through tests/hostmain/jfdump_test.cpp, which links that unit and nothing else.

* against the oracle's loader (itself pinned to the reference on these dumps by tests/test_oracle_vs_ref.py): the 20 quirky
  dumps of test_gpu_parity.py::test_jfdump_loader_on_quirky_dumps and hand-written texts of a few bytes;
* independence of the split: 1, 2, 3, 7 and 32 pieces give the same codes, inv_mid, put list, totals and scan length, also on
  files far below the size at which the library itself starts a second thread;
* the writer byte for byte against b">%d\\n%s\\n", and its text read back through the parser;
* the same program under ASan + UBSan and under TSan (run directly, nothing preloaded); any report fails."""
import os
import subprocess

import numpy as np
import pytest

import io_quirks
from test_sanitizers import ASAN, ENV, TSAN, _sanitizer_works

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rcorrector_amd", "csrc")
SEEDS = list(range(400, 420))
PIECES = "1,2,3,7,32"

# k = 5.  (text, load_state_invalid, scan length): the invalid state is that of the last entry with a count above 1 -- a letter
# outside ACGT among its last k leaves it set -- and an invalid state after the load pass ends the ERROR_RATE scan before its
# first entry; otherwise the scan runs up to the first entry with such a letter before its last base, or over all entries
HAND = {
    "empty": (b"", 0, 0),
    "white_space": (b" \n\t\r\n\f\v ", 0, 0),
    "no_final_newline": (b">7\nACGTA", 0, 1),
    "one_line": (b">7 ACGTA\n", 0, 1),
    "plus": (b">+7\nACGTA\n", 0, 1),
    "minus": (b">-3\nACGTA\n", 0, 1),
    "junk_behind_count": (b">7x9\nACGTA\n", 0, 1),
    "beyond_long": (b">99999999999999999999\nACGTA\n", 0, 1),
    "one_and_zero": (b">1\nACGTA\n>0\nCCGTA\n>3\nGGGTA\n", 0, 3),
    "too_long": (b">4\nACGTACGT\n", 0, 1),
    "too_short": (b">4\nACG\n", 0, 1),
    "n_last": (b">5\nCCCCC\n>4\nACGTN\n", 1, 0),
    "n_last_then_more": (b">4\nACGTN\n>5\nCCCCC\n", 0, 2),
    "n_middle": (b">5\nCCCCC\n>4\nACNTA\n>6\nAAAAC\n", 0, 1),
    "gt_in_kmer": (b">5\nCCCCC\n\n>6\nAC>TA\n>7\nAAAAC\n", 0, 1),
    "twice": (b">5\nCCCCC\n>9\nCCCCC\n", 0, 2),
    "split_on_gt": (b">5\nCCCCC\n>6\nAAAAC\n", 0, 2),
}
assert HAND["split_on_gt"][0][len(HAND["split_on_gt"][0]) // 2:][:1] == b">"


def build(exe, flags):
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + list(flags) + ["-I", CSRC, os.path.join(ROOT, "tests", "hostmain", "jfdump_test.cpp"),
                    os.path.join(CSRC, "rc_jfdump.cpp"), "-o", exe, "-lpthread"], check=True)
    return exe


def run(exe, args, env=None):
    p = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, env=env)
    return p.returncode, p.stdout.decode()


def parse_output(out):
    """-> (one dict per piece count, {canonical code: count})"""
    rows, table = [], {}
    for line in out.splitlines():
        w = line.split()
        if w[0] == "pieces":
            rows.append({w[i]: int(w[i + 1]) for i in range(0, len(w), 2)})
        else:
            assert w[0] == "put", out[-2000:]
            table[int(w[1])] = int(w[2])
    return rows, table


def oracle_table(oracle, k, path):
    T = oracle.Table(k, 1 << 12)
    stored = T.load_dump(path)
    codes, counts = T.export()
    assert len(set(codes.tolist())) == len(codes)
    return stored, dict(zip(codes.tolist(), counts.tolist()))


@pytest.fixture(scope="session")
def exe(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("jfdump") / "jfdump_test"), ["-O2"])


@pytest.fixture(scope="session")
def dumps(tmp_path_factory, oracle):
    """{name: (path, k, stored, table of the oracle)} of the quirky dumps (by seed) and the hand-written texts (by name); left unchanged"""
    d = tmp_path_factory.mktemp("dumps")
    out = {}
    for seed in SEEDS:
        path = str(d / ("%d.jf" % seed))
        io_quirks.make_quirky_dump(seed, path, n=60000 if seed % 4 == 0 else 4000, mid_n=seed % 2 == 0)
        out[seed] = (path, 23) + oracle_table(oracle, 23, path)
    for name, (text, _, _) in HAND.items():
        path = str(d / (name + ".jf"))
        open(path, "wb").write(text)
        out[name] = (path, 5) + oracle_table(oracle, 5, path)
    return out


def check_against_oracle(out, stored, want):
    rows, table = parse_output(out)
    assert [r["pieces"] for r in rows] == [int(p) for p in PIECES.split(",")]
    for r in rows:   # every split: the same vectors as one piece (compared in the program), the same totals
        assert r["same"] == 1 and {k: v for k, v in r.items() if k != "pieces"} == {k: v for k, v in rows[0].items() if k != "pieces"}, r
    assert rows[0]["accepted"] == stored
    assert table == want
    return rows[0]


@pytest.mark.parametrize("seed", SEEDS)
def test_parser_equals_the_oracles_loader_on_quirky_dumps_in_any_split(exe, dumps, seed):
    path, k, stored, want = dumps[seed]
    assert (os.path.getsize(path) > (1 << 20)) == (seed % 4 == 0)   # some above, most below the library's threading threshold
    rc, out = run(exe, ["parse", path, k, PIECES])
    assert rc == 0, out[-2000:]
    row = check_against_oracle(out, stored, want)
    assert row["entries"] >= (60000 if seed % 4 == 0 else 4000) and row["scan"] <= row["entries"]
    if seed % 2:   # (no letter outside ACGT before a last base anywhere: nothing but the load pass's state can end the scan)
        assert row["scan"] == (0 if row["invalid"] else row["entries"])


@pytest.mark.parametrize("name", list(HAND))
def test_parser_on_hand_written_texts(exe, dumps, name):
    path, k, stored, want = dumps[name]
    rc, out = run(exe, ["parse", path, k, PIECES])
    assert rc == 0, out[-2000:]
    row = check_against_oracle(out, stored, want)
    assert (row["invalid"], row["scan"]) == HAND[name][1:], row


def test_read_errors_keep_their_texts(exe, tmp_path):
    missing = str(tmp_path / "none.jf")
    rc, out = run(exe, ["parse", missing, 23, "1"])
    assert rc == 1 and out == "error -3 Could not open file %s\n" % missing


def expected_dump(k, n):
    mask = (1 << (2 * k)) - 1
    counts = (2, 65535, 65536, 2 ** 31 - 1)
    out = []
    for i in range(n):
        code = ((i * 0x9E3779B97F4A7C15 + 12345) & 0xFFFFFFFFFFFFFFFF) & mask
        out.append(b">%d\n%s\n" % (counts[i & 3], bytes(b"ACGT"[(code >> (2 * j)) & 3] for j in range(k - 1, -1, -1))))
    return b"".join(out)


@pytest.mark.parametrize("k", [15, 23, 32])
@pytest.mark.parametrize("n", [1, 2, 70000])
def test_writer_is_byte_equal_and_reads_back(exe, tmp_path, k, n):
    path = str(tmp_path / "w.jf")
    rc, out = run(exe, ["format", path, k, n, 3])
    assert rc == 0 and out == "roundtrip 1\n", out[-2000:]
    assert open(path, "rb").read() == expected_dump(k, n)


@pytest.mark.parametrize("kind", ["asan_ubsan", "tsan"])
def test_dump_text_under_sanitizers(tmp_path, dumps, exe, kind):
    flags = ASAN if kind == "asan_ubsan" else TSAN
    if not _sanitizer_works(flags, tmp_path):
        pytest.skip("no %s run-time for g++ on this box" % kind)
    san = build(str(tmp_path / "jfdump_san"), ("-g",) + flags)
    jobs = [["parse", dumps[name][0], dumps[name][1], PIECES] for name in [400, 401, 404] + list(HAND)]   # (404: several threads parse)
    jobs.append(["format", str(tmp_path / "w.jf"), 32, 70000, 7])
    for args in jobs:
        rc, out = run(san, args, env=ENV)
        assert rc == 0 and "Sanitizer" not in out and "runtime error" not in out, out[-4000:]
        assert out == run(exe, args)[1]
