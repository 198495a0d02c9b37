"""CPU: the mask arithmetic of the per-read screen (rcorrector_amd/csrc/rc_screen.h: rc_screen_add_word, what k_read_screen runs
on its ballots) as a host program against a brute force that marks every base and scans every window --
tests/hostmath/screen_mask.cpp: 0, 1, 63, 64, 65, 127, 128, 129 and 1001 windows at k = 3, 15, 23 and 32 with no hit, all hits,
alternating hits and one hit at the first / last window; two hits k - 1, k and k + 1 windows apart; runs that end at bit 63,
start at bit 64 and cross word boundaries; 200 seeded random masks.  Built and run twice: plain, and with AddressSanitizer +
UndefinedBehaviorSanitizer (the words are allocated to exactly what the mask needs).  And the feature's public surface: the
header as C, the struct, the binding, the tool's usage."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rc_read_screen_device", "rc_read_screen_into"]
FIELDS = ["valid", "hits", "covered", "longest"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_mask_arithmetic_equals_the_brute_force(flags, tmp_path):
    exe = str(tmp_path / "screen_mask")
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I", os.path.join(ROOT, "rcorrector_amd", "csrc"),
                                                             os.path.join(ROOT, "tests", "hostmath", "screen_mask.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)   # (run directly: nothing preloaded)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("ok "), out
    assert int(out.split()[1]) == 9 * 4 * 5 + 4 * (3 * 2 + 3) + 200


def test_the_header_parses_as_c_with_the_new_declarations(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "rcorrector_amd.h"\n'
                   "_Static_assert(sizeof(rc_read_screen) == 16, \"16 bytes per read\");\n"
                   "int (*dev)(rc_ctx *, const rc_ctx *, const uint8_t *, const uint32_t *, uint32_t, uint64_t, int32_t, int32_t, rc_read_screen *) = "
                   "rc_read_screen_device;\n"
                   "int (*into)(rc_ctx *, int, const rc_ctx *, int32_t, rc_read_screen *) = rc_read_screen_into;\n"
                   "int first(const rc_read_screen *d) { return d->valid + d->hits + d->covered + d->longest; }\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    import rcorrector_amd
    assert set(SYMBOLS) <= set(rcorrector_amd.ABI_SYMBOLS)
    h = open(os.path.join(ROOT, "include", "rcorrector_amd.h")).read()
    m = re.search(r"typedef struct \{ int32_t ([\w, ]+); \} rc_read_screen;", h)
    assert m and [x.strip() for x in m.group(1).split(",")] == FIELDS
    assert "8 = per-read screen" in h                    # the kernel-timer index follows the last one the header listed


def test_context_has_the_read_screen_methods():
    import rcorrector_amd
    for m in ("read_screen_device", "read_screen_into", "read_screen_withdraw"):
        assert callable(getattr(rcorrector_amd.Context, m, None)), m


def test_the_tool_without_arguments_prints_its_usage():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "read_screen")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode != 0 and p.stdout == b""
    assert b"usage: read_screen -k INT (-s DUMP | -s-seq FILE ...)" in p.stderr and p.stderr.count(b"\n") == 1
