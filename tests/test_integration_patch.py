"""The drop-in boundary, proved on the reference's own main.cpp: build() applies tools/apply_integration.py
(the INTEGRATION.md section 2 patch) to a temporary copy, compiles the result against include/rcorrector_amd.h
and links it against librcorrector_amd.so (oracle/Makefile: oracle/_ref/rcorrector_patched, where the reference
sources exist).  On the CPU the binary's imports are checked (no run); on a GPU it must reproduce the golden
fixtures -- the reference's I/O and output code around our hot path."""
import os
import subprocess
import sys

import pytest

import golden_util as gu

PATCHED = os.path.join(gu.ROOT, "oracle", "_ref", "rcorrector_patched")


def _symbols(path, *flags):
    return subprocess.run(["nm"] + list(flags) + [path], stdout=subprocess.PIPE, check=True).stdout.decode()


@pytest.mark.skipif(not os.path.exists(PATCHED), reason="oracle/_ref/rcorrector_patched was not built (no reference sources where build() ran)")
def test_patch_applies_compiles_and_links(tmp_path):
    """build() applied the patch to the reference's main.cpp, compiled it against include/rcorrector_amd.h and linked it
    against librcorrector_amd.so (oracle/Makefile: _ref/rcorrector_patched): the binary takes the hot path's calls from
    the library and no longer starts the reference's worker threads."""
    lib = os.path.join(gu.ROOT, "rcorrector_amd", "librcorrector_amd.so")
    assert os.path.exists(lib), "build the library first"
    needed = subprocess.run(["readelf", "-d", PATCHED], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert "[librcorrector_amd.so]" in needed
    imported = {ln.split()[-1].split("@")[0] for ln in _symbols(PATCHED, "-D", "--undefined-only").splitlines() if ln.strip()}
    for call in ("rc_create", "rc_table_load_jfdump", "rc_estimate_error_rate", "rc_set_run_params", "rc_correct_batch"):
        assert call in imported, call
    assert "pthread_create" not in imported
    assert os.path.getsize(PATCHED) > 10000
    # a different main.cpp is refused, not mangled
    bad = tmp_path / "other.cpp"
    bad.write_text("int main() { return 0; }\n")
    assert subprocess.run([sys.executable, os.path.join(gu.ROOT, "tools", "apply_integration.py"), str(bad), str(tmp_path / "x.cpp")]).returncode != 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fx_sample", "fx_se_k23", "fx_pe_k23", "fx_il_k23", "fx_k31_mc8", "fx_skew", "fx_edge", "fx_varlen_n"])
def test_patched_reference_binary_reproduces_goldens(name, tmp_path):
    if not os.path.exists(PATCHED):
        pytest.skip("oracle/_ref/rcorrector_patched was not built (no reference sources where build() ran)")
    p = gu.run_fixture(PATCHED, name, tmp_path)
    gu.assert_same_as_reference(name, tmp_path, p.stderr)
