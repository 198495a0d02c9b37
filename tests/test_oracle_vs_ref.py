"""CPU (build container only): the oracle's CLI against the UNMODIFIED reference binary on the same
random inputs the GPU fuzz test uses -- this is what makes `oracle_cli` a valid stand-in for the
reference on the GPU box.  Skipped where oracle/_ref was not built (no /root/reference)."""
import os
import subprocess

import pytest

from test_gpu_fuzz import _random_case


@pytest.mark.parametrize("seed", list(range(900, 940)))
def test_oracle_cli_equals_reference_on_random_inputs(oracle, seed, tmp_path):
    if not os.path.exists(oracle.REF_BIN):
        pytest.skip("oracle/_ref not built here (no /root/reference)")
    d = str(tmp_path)
    args = _random_case(seed, d)
    outs = {}
    for name, binary, more in (("ref", oracle.REF_BIN, ["-t", "3"] if seed % 2 else []), ("cpu", oracle.CLI_BIN, ["-t", "2"])):
        od = os.path.join(d, name)
        os.makedirs(od)
        p = subprocess.run([binary] + args + ["-od", od] + more, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()
        outs[name] = (p.stderr, {f: open(os.path.join(od, f), "rb").read() for f in sorted(os.listdir(od))})
    assert outs["ref"][1].keys() == outs["cpu"][1].keys() and outs["ref"][1]
    for f in outs["ref"][1]:
        assert outs["ref"][1][f] == outs["cpu"][1][f], "%s differs (seed %d, args %s)" % (f, seed, args)
    assert outs["ref"][0] == outs["cpu"][0], "stderr differs (seed %d)" % seed


@pytest.mark.parametrize("seed", list(range(300, 330)))
def test_oracle_cli_equals_reference_on_io_quirks(oracle, seed, tmp_path):
    """Input quirks with defined behaviour in the reference (tests/io_quirks.py): the oracle's
    command-line front end must write the reference's bytes and stderr lines."""
    import io_quirks
    import subprocess
    if not os.path.exists(oracle.REF_BIN):
        pytest.skip("oracle/_ref not built (needs /root/reference)")
    d = str(tmp_path)
    args = io_quirks.make_case(seed, d, modes=(0, 1, 2))
    res = []
    for name, binary in (("ref", oracle.REF_BIN), ("ora", oracle.CLI_BIN)):
        od = os.path.join(d, name)
        os.makedirs(od)
        p = subprocess.run([binary] + args + ["-od", od, "-verbose"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        res.append((p.returncode, p.stderr, {f: open(os.path.join(od, f), "rb").read() for f in sorted(os.listdir(od))}, p.stdout))
    assert res[0][0] == 0 and res[0] == res[1]


@pytest.mark.parametrize("seed", list(range(400, 412)))
def test_oracle_dump_loader_equals_reference_on_quirky_dumps(oracle, seed, tmp_path):
    """tests/io_quirks.py: make_quirky_dump -- 'Stored N kmers', the ERROR_RATE estimate and the
    corrected reads must be the reference's when the dump departs from the clean jellyfish layout."""
    import io_quirks
    import subprocess
    import synth
    if not os.path.exists(oracle.REF_BIN):
        pytest.skip("oracle/_ref not built (needs /root/reference)")
    d = str(tmp_path)
    io_quirks.make_quirky_dump(seed, os.path.join(d, "d.jf"), mid_n=seed % 2 == 0)
    s1, q1, _, _, _ = synth.make_reads(seed, 30, 60, n_tx=2, l_tx=200, e=0.01)
    synth.write_fastq(os.path.join(d, "a.fq"), s1, q1)
    res = []
    for name, binary in (("ref", oracle.REF_BIN), ("ora", oracle.CLI_BIN)):
        od = os.path.join(d, name)
        os.makedirs(od)
        p = subprocess.run([binary, "-r", "a.fq", "-k", "23", "-c", "d.jf", "-od", od, "-wk", "0.5"], cwd=d,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        res.append((p.returncode, p.stderr, open(os.path.join(od, "a.cor.fq"), "rb").read()))
    assert res[0][0] == 0 and res[0] == res[1]


@pytest.mark.parametrize("name", ["huge_k23_ext0/B", "huge_k27_ext8/B"])
def test_oracle_cli_equals_reference_on_counts_up_to_int_max(oracle, name, tmp_path):
    """The huge_ data sets (tests/datasets.py) as files: counts of 10^5 .. 2^31 - 1 in the dump, so GetBound's (int)
    conversions, the thresholds beyond 65536 and the ERROR_RATE sample (main.cpp:329-345, sums of such counts) are the
    reference's own in the oracle that the GPU tests of these sets lean on."""
    import datasets
    if not os.path.exists(oracle.REF_BIN):
        pytest.skip("oracle/_ref not built (needs /root/reference)")
    d = str(tmp_path)
    ds = datasets.make(name)
    assert max(c for _, c in ds["pinned"]) == (datasets.INT_MAX if ds["ext"] == 0 else ds["limit"])
    args = datasets.write_cli_case(ds, d)
    res = []
    for tag, binary, more in (("ref", oracle.REF_BIN, []), ("ora", oracle.CLI_BIN, ["-t", "2"])):
        od = os.path.join(d, tag)
        os.makedirs(od)
        p = subprocess.run([binary] + args + ["-od", od] + more, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        res.append((p.returncode, p.stderr, {f: open(os.path.join(od, f), "rb").read() for f in sorted(os.listdir(od))}))
    assert res[0][0] == 0 and res[0][2] and res[0] == res[1]
    heads = b"".join(res[0][2].values()).split(b"\n")[0::4]
    assert sum(h.endswith(b" cor") for h in heads) >= len(heads) // 3   # (a third of the reads corrected, in the reference's own output)


@pytest.mark.parametrize("name", ["qv_pair/straddle", "qv_ends/straddle", "qv_dense_mfk2/straddle", "qv_dense_mfk1/straddle", "qv_mixed_pe/straddle",
                                  "qv_mixed_il/straddle", "qv_lengths/straddle", "qv_pair_k32/straddle", "qv_mixed_pe/fasta"])
def test_oracle_cli_equals_reference_where_qualities_decide(oracle, name, tmp_path):
    """The qv_ data sets (tests/datasets.py) as files, -maxcorK as the data set says: the GPU tests of the vetoes lean on the
    oracle exactly here.  (FASTA with -t 2: the reference's -t 1 loop does not survive input without qualities.)"""
    import datasets
    if not os.path.exists(oracle.REF_BIN):
        pytest.skip("oracle/_ref not built (needs /root/reference)")
    d = str(tmp_path)
    ds = datasets.for_cli(datasets.make(name))
    if "lengths" in name:   # (1023 bases and a newline do not fit the reference's line buffer: those reads lose their last base)
        assert sum(len(r) == 1023 for r in ds["seqs1"]) >= 10
        ds = dict(ds, seqs1=[r[:1022] for r in ds["seqs1"]], quals1=[q[:1021] + q[-1:] if len(q) == 1023 else q for q in ds["quals1"]])
    args = datasets.write_cli_case(ds, d) + (["-t", "2"] if ds["fasta"] else [])
    res = []
    for tag, binary in (("ref", oracle.REF_BIN), ("ora", oracle.CLI_BIN)):
        od = os.path.join(d, tag)
        os.makedirs(od)
        p = subprocess.run([binary] + args + ["-od", od], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        res.append((p.returncode, p.stderr, {f: open(os.path.join(od, f), "rb").read() for f in sorted(os.listdir(od))}))
    assert res[0][0] == 0 and res[0][2] and res[0] == res[1]
    assert ds["fasta"] or b"Bad quality threshold is 'H'" in res[0][1], res[0][1]   # (datasets.for_cli: the bytes do straddle it)
    before = b"".join(open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.startswith("reads"))
    assert b"".join(res[0][2].values()) != before   # (something was corrected)
