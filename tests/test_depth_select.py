"""CPU: the selection of the per-read k-mer depth (rcorrector_amd/csrc/rc_depth.h: rc_depth_select, what k_read_depth runs per
read) as a host program against a sort -- tests/hostmath/depth_select.cpp: n = 0..9, 63, 64, 65, 127, 128, 129 and 1001 (the most
windows a 1 023-base read has, at k = 23), all counts equal, counts in {0, 2^27 - 1} only, strictly increasing and decreasing
counts, each with and without invalid windows in between, 200 seeded random cases with heavy ties, and the rank arithmetic for
n = 1..9.  Built and run twice: plain, and with AddressSanitizer + UndefinedBehaviorSanitizer (the counts are allocated to
exactly the slots a wavefront's lanes hold).  And the feature's public surface: the header as C, the struct, the binding."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rc_read_depth_device", "rc_read_depth_into"]
FIELDS = ["valid", "q1", "median", "q3"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_depth_select_equals_the_sort(flags, tmp_path):
    exe = str(tmp_path / "depth_select")
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I", os.path.join(ROOT, "rcorrector_amd", "csrc"),
                                                             os.path.join(ROOT, "tests", "hostmath", "depth_select.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)   # (run directly: nothing preloaded)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("ok "), out
    assert int(out.split()[1]) == 17 * 2 * 9 + 200 + 9


def test_the_header_parses_as_c_with_the_new_declarations(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "rcorrector_amd.h"\n'
                   "_Static_assert(sizeof(rc_read_depth) == 16, \"16 bytes per read\");\n"
                   "int (*dev)(rc_ctx *, const uint8_t *, const uint32_t *, uint32_t, uint64_t, int32_t, rc_read_depth *) = rc_read_depth_device;\n"
                   "int (*into)(rc_ctx *, int, rc_read_depth *) = rc_read_depth_into;\n"
                   "int first(const rc_read_depth *d) { return d->valid + d->q1 + d->median + d->q3; }\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    import rcorrector_amd
    assert set(SYMBOLS) <= set(rcorrector_amd.ABI_SYMBOLS)
    h = open(os.path.join(ROOT, "include", "rcorrector_amd.h")).read()
    m = re.search(r"typedef struct \{ int32_t ([\w, ]+); \} rc_read_depth;", h)
    assert m and [x.strip() for x in m.group(1).split(",")] == FIELDS
    assert "7 = per-read k-mer depth" in h               # the kernel-timer index follows the last one the header listed


def test_context_has_the_read_depth_methods():
    import rcorrector_amd
    for m in ("read_depth_device", "read_depth_into", "read_depth_withdraw"):
        assert callable(getattr(rcorrector_amd.Context, m, None)), m


def test_cli_and_wrapper_help_list_the_depth_flags():
    import rcorrector_amd
    rcorrector_amd.build_library()
    e = subprocess.run([os.path.join(ROOT, "rcorrector_amd", "rcorrector"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE).stderr
    assert e.index(b"MI355X build only:") < e.index(b"\t-depth-tags:") < e.index(b"\t-depth STRING:") < e.index(b"\t-depth-max INT:")
    assert b"kdepth=Q1:MED:Q3" in e and b"-verbose" in e[e.index(b"\t-depth-tags:"):e.index(b"\t-depth STRING:")]
    w = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_rcorrector_gpu")], stdout=subprocess.PIPE, stderr=subprocess.PIPE).stderr
    assert w.index(b"\t-depth-tags:") < w.index(b"\t-depth FILE:") < w.index(b"\t-depth-max INT:")
