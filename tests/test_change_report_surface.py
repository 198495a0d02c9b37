"""CPU: the correction report's public surface -- the three C ABI symbols in the binding's list and in the header with
`rc_change_report` and its two limits, the three `Context` methods, `-report` in `rcorrector`'s help (the build's own part,
behind -histo-after) and in the run_rcorrector.pl-style wrapper.  (What they compute: tests/test_change_report.py,
tests/test_change_report_cli.py.)"""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rc_change_report_begin", "rc_change_report_get", "rc_change_report_end"]
FIELDS = ["reads", "reads_changed", "reads_unfixable", "changes", "len_hist", "by_pos5", "by_pos3", "subst", "by_qual", "per_read"]


def test_report_entry_points_and_struct_are_declared():
    import rcorrector_amd
    assert set(SYMBOLS) <= set(rcorrector_amd.ABI_SYMBOLS)
    h = open(os.path.join(ROOT, "include", "rcorrector_amd.h")).read()
    assert re.search(r"\}\s*rc_change_report;", h)
    assert re.search(r"^#define RC_REPORT_MAX_LEN 1024$", h, re.M)
    assert re.search(r"^#define RC_REPORT_MAX_PER_READ 64$", h, re.M)
    for s in SYMBOLS:
        assert re.search(r"^int %s\(rc_ctx \*ctx" % s, h, re.M), s
    body = h[h.index("typedef struct {", h.index("RC_REPORT_MAX_PER_READ 64")):h.index("} rc_change_report;")]
    assert re.findall(r"uint64_t (\w+)\[", body) == FIELDS   # every count 64 bits, in this order


def test_the_binding_mirrors_the_struct():
    from rcorrector_amd import binding
    assert [n for n, _ in binding._ChangeReport._fields_] == FIELDS
    # 8 per-mate totals, six tables of 1024, 20 substitutions, 3 quality classes, 65 per-read bins
    assert ctypes.sizeof(binding._ChangeReport) == 8 * (8 + 6 * 1024 + 20 + 3 + 65)
    assert binding.REPORT_MAX_LEN == 1024 and binding.REPORT_MAX_PER_READ == 64


def test_context_has_the_report_methods():
    import rcorrector_amd
    for m in ("change_report_begin", "change_report", "change_report_end"):
        assert callable(getattr(rcorrector_amd.Context, m, None)), m


def test_cli_help_lists_report():
    import rcorrector_amd
    rcorrector_amd.build_library()
    p = subprocess.run([os.path.join(ROOT, "rcorrector_amd", "rcorrector"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"\t-report STRING:" in p.stderr
    # the reference's part of the help comes first, unchanged; the new flag is in the build's own part, behind -histo-after
    assert p.stderr.index(b"MI355X build only:") < p.stderr.index(b"\t-histo-after STRING:") < p.stderr.index(b"\t-report STRING:")
    assert b"-gpus" in p.stderr[p.stderr.index(b"\t-report STRING:"):p.stderr.index(b"\t-verbose-iter")]  # (says what several GPUs do)


def test_wrapper_help_lists_report():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_rcorrector_gpu")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"-report FILE" in p.stderr
