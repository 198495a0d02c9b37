"""CPU: the recount session's public surface -- the five C ABI symbols in the binding's list and in the header with
`rc_recount_stats`, the five `Context` methods, `-histo-after` in `rcorrector`'s help (the build's own part) and in the
run_rcorrector.pl-style wrapper.  (What they compute: tests/test_recount.py, tests/test_recount_cli.py.)"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rc_recount_begin", "rc_recount_add", "rc_recount_add_device", "rc_recount_follow", "rc_recount_finish"]


def test_recount_entry_points_are_declared():
    import rcorrector_amd
    assert set(SYMBOLS) <= set(rcorrector_amd.ABI_SYMBOLS)
    h = open(os.path.join(ROOT, "include", "rcorrector_amd.h")).read()
    assert re.search(r"\}\s*rc_recount_stats;", h)
    for s in SYMBOLS:
        assert re.search(r"^int %s\(rc_ctx \*ctx" % s, h, re.M), s
    assert "absent_distinct" in h and "absent_total" in h


def test_context_has_the_recount_methods():
    import rcorrector_amd
    for m in ("recount_begin", "recount_add", "recount_add_device", "recount_follow", "recount_finish"):
        assert callable(getattr(rcorrector_amd.Context, m, None)), m


def test_cli_help_lists_histo_after():
    import rcorrector_amd
    rcorrector_amd.build_library()
    p = subprocess.run([os.path.join(ROOT, "rcorrector_amd", "rcorrector"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"\t-histo-after STRING:" in p.stderr
    # the reference's part of the help comes first, unchanged; the new flag is in the build's own part, behind -histo-max
    assert p.stderr.index(b"MI355X build only:") < p.stderr.index(b"\t-histo-max INT:") < p.stderr.index(b"\t-histo-after STRING:")
    assert b"-gpus" in p.stderr[p.stderr.index(b"\t-histo-after STRING:"):]  # (says where several GPUs count)


def test_wrapper_help_lists_histo_after():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_rcorrector_gpu")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"-histo-after FILE" in p.stderr
