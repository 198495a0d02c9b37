"""CPU: the duplicate census's 128-bit keys (rcorrector_amd/csrc/rc_dups.h, what k_read_keys computes sixteen lanes to a read)
as a host program -- tests/hostmath/dup_key.cpp: the keys are distinct exactly where the strings are.  Every length 0..70, 255,
256, 257 and 1023; two 16-byte chunks swapped; the first and the last byte changed; a string against itself with A appended;
N against n against A; pairs against swapped pairs; every split of one 40-byte string into two mates; 1 M seeded random reads
of 20..160 bases with no two keys equal in either 64-bit lane.  Built and run twice: plain, and as a stand-alone program with
AddressSanitizer + UndefinedBehaviorSanitizer (every string is keyed from a heap block of exactly its bytes).  The program's
`keys` mode, which the GPU tests compare rc_read_keys_device with word for word, is held here to the same definitions."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostmath", "dup_key.cpp")


def build(tmp_path, flags):
    exe = str(tmp_path / "dup_key")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + ["-I", os.path.join(ROOT, "rcorrector_amd", "csrc"), SRC, "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_keys_are_distinct_exactly_where_the_strings_are(flags, tmp_path):
    exe = build(tmp_path, flags)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)   # (run directly: nothing preloaded)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("ok "), out
    assert int(out.split()[1]) > 1000000


def keys_of(exe, reads, mode):
    p = subprocess.run([exe, "keys", str(mode)], input=("\n".join(reads) + "\n").encode(), stdout=subprocess.PIPE, check=True)
    return [tuple(int(w, 16) for w in line.split()) for line in p.stdout.decode().splitlines()]


def test_keys_mode_groups_the_reads_as_the_modes_do(tmp_path):
    exe = build(tmp_path, ["-O2"])
    reads = ["ACGT", "", "ACGTA", "AC", "GT", "ACG", "T", "ACGT"]
    single = keys_of(exe, reads, 0)
    assert len(single) == 8 and single[0] == single[7] and len(set(single)) == 7
    paired = keys_of(exe, reads, 1)        # (r, 4 + r)
    inter = keys_of(exe, reads, 2)         # (2u, 2u + 1)
    assert len(paired) == 4 and len(inter) == 4
    # the same pair of strings keyed through either grouping
    assert keys_of(exe, ["AC", "ACG", "GT", "T"], 1) == keys_of(exe, ["AC", "GT", "ACG", "T"], 2)
    k = keys_of(exe, ["AC", "GT", "ACG", "T", "GT", "AC"], 2)
    assert len(set(k)) == 3                # ("AC", "GT"), ("ACG", "T"), ("GT", "AC")
    assert keys_of(exe, ["AC", "GT"], 2)[0] not in single
