"""CPU: the k-mer count spectrum's public surface -- the C ABI symbols in the binding's list, the `-histo` / `-histo-max`
flags in `rcorrector`'s help and in the run_rcorrector.pl-style wrapper.  (What they compute: tests/test_kmer_spectrum.py.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spectrum_entry_points_are_declared():
    import rcorrector_amd
    assert {"rc_table_count_spectrum", "rc_table_spectrum"} <= set(rcorrector_amd.ABI_SYMBOLS)
    h = open(os.path.join(ROOT, "include", "rcorrector_amd.h")).read()
    assert "rc_spectrum_stats" in h
    assert hasattr(rcorrector_amd.Context, "count_spectrum") and hasattr(rcorrector_amd.Context, "kmer_spectrum")


def test_cli_help_lists_histo_flags():
    import rcorrector_amd
    rcorrector_amd.build_library()
    p = subprocess.run([os.path.join(ROOT, "rcorrector_amd", "rcorrector"), "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"\t-histo STRING:" in p.stderr and b"\t-histo-max INT:" in p.stderr
    # the reference's part of the help comes first, unchanged; the new flags are in the build's own part
    assert p.stderr.index(b"MI355X build only:") < p.stderr.index(b"-histo")


def test_wrapper_help_lists_histo_flags():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_rcorrector_gpu")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"-histo FILE" in p.stderr and b"-histo-max INT" in p.stderr
