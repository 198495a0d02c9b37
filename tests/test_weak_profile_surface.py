"""CPU: the weak-k-mer profile's public surface -- the two C ABI symbols in the binding's list and in the header with
`rc_read_weak`, the 16-byte struct in the binding, the two `Context` methods, `-weak-ends` / `-weak-min` in `rcorrector`'s help
(the build's own part, behind -report) and in the run_rcorrector.pl-style wrapper.  (What they compute:
tests/test_weak_profile.py, tests/test_weak_profile_cli.py, tests/test_weak_reduce.py.)"""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rc_weak_profile_device", "rc_weak_profile_into"]
FIELDS = ["weak", "bad_prefix", "bad_suffix", "uncovered"]


def test_weak_entry_points_and_struct_are_declared():
    import rcorrector_amd
    assert set(SYMBOLS) <= set(rcorrector_amd.ABI_SYMBOLS)
    h = open(os.path.join(ROOT, "include", "rcorrector_amd.h")).read()
    m = re.search(r"typedef struct \{ int32_t ([\w, ]+); \} rc_read_weak;", h)
    assert m and [x.strip() for x in m.group(1).split(",")] == FIELDS
    for s in SYMBOLS:
        assert re.search(r"^int %s\(rc_ctx \*ctx" % s, h, re.M), s
    # each entry's comment ends "No reference counterpart" and cites the reference's dormant fields
    assert len(re.findall(r"No reference counterpart: the dormant fields of Reads\.h:20,371-372,396-412\. \*/\nint rc_weak_profile_", h)) == 2


def test_the_binding_mirrors_the_struct():
    from rcorrector_amd import binding
    assert [n for n, _ in binding._ReadWeak._fields_] == FIELDS
    assert ctypes.sizeof(binding._ReadWeak) == 16


def test_context_has_the_weak_profile_methods():
    import rcorrector_amd
    for m in ("weak_profile_device", "weak_profile_into"):
        assert callable(getattr(rcorrector_amd.Context, m, None)), m


def test_cli_help_lists_weak_ends():
    import rcorrector_amd
    rcorrector_amd.build_library()
    p = subprocess.run([os.path.join(ROOT, "rcorrector_amd", "rcorrector"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    e = p.stderr
    assert b"\t-weak-ends:" in e and b"\t-weak-min INT:" in e
    # the reference's part of the help comes first, unchanged; the new flags are in the build's own part, behind -report
    assert e.index(b"MI355X build only:") < e.index(b"\t-report STRING:") < e.index(b"\t-weak-ends:") < e.index(b"\t-weak-min INT:")
    assert b"bad_prefix=" in e and b"bad_suffix=" in e and b"-verbose" in e[e.index(b"\t-weak-ends:"):e.index(b"\t-weak-min INT:")]


def test_wrapper_help_lists_weak_ends():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_rcorrector_gpu")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    e = p.stderr
    assert e.index(b"-report FILE") < e.index(b"\t-weak-ends:") < e.index(b"\t-weak-min INT:")
