"""CPU: the word extraction of the trust profile's accumulate (rcorrector_amd/csrc/rc_trust.h: what k_trust_accumulate runs per
read and word) as a host program against a bit-by-bit loop -- tests/hostmath/trust_words.cpp: random bit planes of three
densities, nwin = 0 .. 200 and 1000 .. 1024, the read starting at every bit offset of a plane word, fixed seeds.  Built and
run twice: plain, and with AddressSanitizer + UndefinedBehaviorSanitizer (the planes are allocated to exactly the words a
read's windows lie in, so a fetch past them is caught).  The same comparison must FAIL for a right-aligned word that lacks
the cut where the window string starts inside the word."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = 3 * (201 + 25) * 2 * 64


def build(flags, exe):
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I", os.path.join(ROOT, "rcorrector_amd", "csrc"),
                                                             os.path.join(ROOT, "tests", "hostmath", "trust_words.cpp"), "-o", exe], check=True)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_trust_words_equal_the_bit_by_bit_loop(flags, tmp_path):
    exe = str(tmp_path / "trust_words")
    build(flags, exe)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)   # (run directly: nothing preloaded)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("ok "), out
    assert int(out.split()[1]) == CASES


def test_the_comparison_fails_without_the_negative_start_mask(tmp_path):
    exe = str(tmp_path / "trust_words")
    build(["-O2"], exe)
    p = subprocess.run([exe, "dropmask"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 1 and out.startswith("word3: nwin "), out
    assert int(out.split()[2]) < 64 or int(out.split()[2]) % 64 != 0   # (a word the string starts inside of)


def test_the_header_states_the_contract():
    h = open(os.path.join(ROOT, "include", "rcorrector_amd.h")).read()
    assert "#define RC_TRUST_MAX_LEN 1024" in h and "} rc_trust_counts;" in h and "rc_trust_profile;" in h
    sec = h[h.index("k-mer trust profile by read position"):h.index("int rc_trust_profile_end")]
    assert "No reference counterpart" in sec and "can never index outside the arrays" in sec and "aligned 16-byte" in sec
