"""CPU: the word-level reduce of the weak-k-mer profile (rcorrector_amd/csrc/rc_weak.h: rc_weak_reduce, what k_weak_reduce
runs per read) as a host program against a per-base loop -- tests/hostmath/weak_reduce.cpp: random bit planes, k in {3, 15,
23, 31, 32}, read lengths 0, 1, k-1, k, k+1, 63, 64, 65, 127, 128, 129, 1023, the read starting at every bit offset of a plane
word, fixed seeds.  Built and run twice: plain, and with AddressSanitizer + UndefinedBehaviorSanitizer (the planes are
allocated to exactly the words a read touches, so a read past them is caught)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_weak_reduce_equals_the_per_base_loop(flags, tmp_path):
    exe = str(tmp_path / "weak_reduce")
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I", os.path.join(ROOT, "rcorrector_amd", "csrc"),
                                                             os.path.join(ROOT, "tests", "hostmath", "weak_reduce.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)   # (run directly: nothing preloaded)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("ok "), out
    assert int(out.split()[1]) == 3 * 5 * 12 * 2 * 64
