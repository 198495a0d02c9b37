"""GPU: `rcorrector -histo-after FILE` -- the k-mer count spectrum of the corrected reads and the line on stderr that says
how many of their k-mers the table does not hold.

For every golden fixture the CLI parity test uses, the `cmd.txt` command plus `-histo-after` must write the file a numpy
model (tests/test_recount.py) computes from the sequences of the REFERENCE's own `ref/*.cor.f[aq]`, with table membership
taken from `dump.jf` (entries with count >= 2); the outputs and the rest of stderr stay the goldens byte for byte, and the
new line carries the model's numbers.  One paired fixture is repeated without -c, with -packed, in many small batches with
four in flight, from .gz input, on two contexts, to stdout, and with a small -histo-max.

That the cases discriminate (numpy over tests/golden/*/ref and dump.jf, count >= 2) -- distinct k-mers in the table / in the
reference's corrected reads / of those absent from the table (occurrences): fx_pe_k23 14 515 / 23 887 / 9 372 (9 570),
fx_se_k23 5 684 / 18 245 / 12 561 (12 714), fx_k15 4 107 / 10 348 / 6 241 (6 363), fx_edge 4 328 / 21 916 / 18 374 (23 993),
fx_sample 253 / 325 / 72 (72): neither the table's spectrum nor zeros would pass.  The tests compute their expectations
themselves.
"""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import golden_util as gu
from test_recount import canonical_codes, model

pytestmark = pytest.mark.gpu
CLI = os.path.join(gu.ROOT, "rcorrector_amd", "rcorrector")
PAIRED = "fx_pe_k23"


def fixture_args(name):
    return open(os.path.join(gu.GOLDEN, name, "cmd.txt")).read().split()


def sequences(path):
    """the sequence lines of a FASTQ / FASTA file as one NUL-separated arena (the reference leaves an empty line behind some
    records of fx_io_quirks: skipped where a header is due)"""
    lines = open(path, "rb").read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    step, mark = (4, b"@") if path.endswith("q") else (2, b">")
    seqs, i = [], 0
    while i < len(lines):
        if lines[i] == b"":
            i += 1
            continue
        assert lines[i].startswith(mark) and i + step <= len(lines), "%s: line %d" % (path, i + 1)
        seqs.append(lines[i + 1])
        i += step
    return b"".join(s + b"\0" for s in seqs)


def dump_codes(path, k, min_count=2):
    tok = open(path, "rb").read().split()
    counts = np.array([int(t[1:]) for t in tok[0::2]], dtype=np.int64)
    kmers = [t for t, c in zip(tok[1::2], counts) if c >= min_count]
    assert all(len(t) == k for t in kmers)
    return canonical_codes(b"".join(t + b"\0" for t in kmers), k)


def expected(name, max_bin=10000, table=None):
    d = os.path.join(gu.GOLDEN, name)
    args = fixture_args(name)
    k = int(args[args.index("-k") + 1])
    ref = os.path.join(d, "ref")
    arenas = [sequences(os.path.join(ref, f)) for f in sorted(os.listdir(ref)) if ".cor.f" in f]
    assert arenas
    return model(arenas, k, dump_codes(os.path.join(d, "dump.jf"), k) if table is None else table, max_bin)


def histo_text(freq):
    return "".join("%d %d\n" % (c, f) for c, f in enumerate(freq.tolist()) if c >= 1 and f).encode()


def summary_line(st):
    return ("Corrected reads: %d distinct k-mers, %d seen once, %d not in the table (%d occurrences)\n"
            % (st["distinct"], st["unique"], st["absent_distinct"], st["absent_total"])).encode()


def check_run(p, histo, want, golden_stderr):
    assert open(histo, "rb").read() == histo_text(want[0])
    assert p.stderr == golden_stderr + summary_line(want[1])


@pytest.mark.parametrize("name", gu.FIXTURES)
def test_histo_after_of_every_golden_fixture(name, tmp_path):
    want = expected(name)
    assert want[1]["distinct"] > 0
    histo = str(tmp_path / "after.histo")
    p = gu.run_fixture(CLI, name, tmp_path, extra=["-histo-after", histo])
    golden = open(os.path.join(gu.GOLDEN, name, "ref", "stderr.txt"), "rb").read()
    gu.assert_same_as_reference(name, tmp_path, None, check_stderr=False)
    check_run(p, histo, want, golden)
    # ... and the same run without the flag writes the goldens, and no such line
    od2 = tmp_path / "plain"
    p2 = gu.run_fixture(CLI, name, od2)
    gu.assert_same_as_reference(name, od2, p2.stderr)


VARIANTS = {
    "packed": (["-packed"], {}),
    "small_batches": (["-batch", "60", "-inflight", "4"], {}),
    "small_batches_packed_lanes_off": (["-packed", "-batch", "60", "-inflight", "4"], {"RC_SLOT_LANES": "0"}),
    "two_contexts": (["-gpus", "2", "-batch", "64", "-inflight", "2"], {"RC_SHARED_GPU": "1"}),
    "two_contexts_packed": (["-gpus", "2", "-batch", "64", "-packed"], {"RC_SHARED_GPU": "1"}),
    "threads": (["-t", "8", "-batch", "100"], {}),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_histo_after_does_not_depend_on_transport_batching_or_contexts(variant, tmp_path):
    extra, env = VARIANTS[variant]
    want = expected(PAIRED)
    d = os.path.join(gu.GOLDEN, PAIRED)
    n_reads = len(open(os.path.join(d, "reads_1.fq"), "rb").read().split(b"\n")) // 4
    assert n_reads * 2 >= 5 * 64   # (-batch counts reads: at least five batches)
    histo = str(tmp_path / "after.histo")
    p = subprocess.run([CLI] + fixture_args(PAIRED) + ["-od", str(tmp_path), "-histo-after", histo] + extra, cwd=d, env=dict(os.environ, **env),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    gu.assert_same_as_reference(PAIRED, tmp_path, None, check_stderr=False)
    check_run(p, histo, want, open(os.path.join(d, "ref", "stderr.txt"), "rb").read())


def test_histo_after_without_a_dump(tmp_path):
    """no -c: the k-mers are counted here (one pass where it fits: the resident transport; two passes with RC_RESIDENT=0, and on
    two contexts) -- the flag changes no output byte and no other byte of stderr, and the file is the model's over the
    run's own corrected reads, with the table the counter built (count >= 2) from the input reads"""
    d = os.path.join(gu.GOLDEN, PAIRED)
    args = [a for a in fixture_args(PAIRED)]
    i = args.index("-c")
    del args[i:i + 2]
    k = int(args[args.index("-k") + 1])
    inputs = [sequences(os.path.join(d, f)) for f in ("reads_1.fq", "reads_2.fq")]
    u, c = np.unique(np.concatenate([canonical_codes(a, k) for a in inputs]), return_counts=True)
    table = u[c >= 2]
    results = {}
    for tag, extra, env in (("plain", [], {}), ("one_pass", ["-batch", "100"], {"RC_RESIDENT": "1"}), ("two_pass", ["-batch", "100"], {"RC_RESIDENT": "0"}),
                            ("two_ctx", ["-gpus", "2", "-batch", "100"], {"RC_SHARED_GPU": "1", "RC_RESIDENT": "1"})):
        for flag in (False, True):
            od = tmp_path / ("%s_%d" % (tag, flag))
            histo = str(tmp_path / ("%s.histo" % tag))
            p = subprocess.run([CLI] + args + ["-od", str(od)] + extra + (["-histo-after", histo] if flag else []), cwd=d, env=dict(os.environ, **env),
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert p.returncode == 0, p.stderr.decode()
            outs = {f: open(os.path.join(str(od), f), "rb").read() for f in sorted(os.listdir(str(od)))}
            if not flag:
                results[tag] = (outs, p.stderr)
                continue
            assert outs == results[tag][0]
            assert outs == results["plain"][0]
            want = model([sequences(os.path.join(str(od), f)) for f in sorted(outs)], k, table)
            check_run(p, histo, want, results[tag][1])


def test_histo_after_from_gz_input_to_stdout_and_with_a_small_bound(tmp_path):
    src = os.path.join(gu.GOLDEN, PAIRED)
    golden = open(os.path.join(src, "ref", "stderr.txt"), "rb").read()
    work = tmp_path / "in"
    work.mkdir()
    for n in ("reads_1.fq", "reads_2.fq"):
        with open(os.path.join(src, n), "rb") as f, gzip.open(work / (n + ".gz"), "wb") as g:
            shutil.copyfileobj(f, g)
    out = tmp_path / "out"
    histo = str(tmp_path / "gz.histo")
    p = gu.run_fixture(CLI, PAIRED, out, args_override=["-p", str(work / "reads_1.fq.gz"), str(work / "reads_2.fq.gz"), "-k", "23", "-c",
                                                        os.path.join(src, "dump.jf"), "-batch", "100", "-histo-after", histo])
    for n in ("reads_1", "reads_2"):
        assert gzip.open(out / (n + ".cor.fq.gz"), "rb").read() == open(os.path.join(src, "ref", n + ".cor.fq"), "rb").read()
    check_run(p, histo, expected(PAIRED), golden)
    # -stdout: the records go to stdout as without the flag, the spectrum to its file
    histo = str(tmp_path / "stdout.histo")
    plain = gu.run_fixture(CLI, PAIRED, tmp_path / "s0", extra=["-stdout"])
    p = gu.run_fixture(CLI, PAIRED, tmp_path / "s1", extra=["-stdout", "-histo-after", histo])
    assert p.stdout == plain.stdout
    check_run(p, histo, expected(PAIRED), plain.stderr)
    # -histo-max bounds this file too: counts >= 3 fold into the last bin; the line's numbers do not change
    histo = str(tmp_path / "max3.histo")
    p = gu.run_fixture(CLI, PAIRED, tmp_path / "m3", extra=["-histo-after", histo, "-histo-max", "3"])
    want = expected(PAIRED, 3)
    assert len(histo_text(want[0]).splitlines()) == 3 and want[1] == expected(PAIRED)[1]
    check_run(p, histo, want, golden)
    # -histo and -histo-after side by side: two files, the first one the dump's spectrum as before
    before, after = str(tmp_path / "b.histo"), str(tmp_path / "a.histo")
    p = gu.run_fixture(CLI, PAIRED, tmp_path / "both", extra=["-histo", before, "-histo-after", after])
    check_run(p, after, expected(PAIRED), golden)
    alone = str(tmp_path / "alone.histo")
    gu.run_fixture(CLI, PAIRED, tmp_path / "alone", extra=["-histo", alone])
    assert open(before, "rb").read() == open(alone, "rb").read() != open(after, "rb").read()


def test_histo_after_of_a_fasta_file(tmp_path):
    name = "fa_se_k23"
    d = os.path.join(gu.GOLDEN, name)
    if not os.path.isdir(d):
        pytest.fail("the FASTA fixture %s is missing" % name)
    want = expected(name)
    histo = str(tmp_path / "after.histo")
    p = gu.run_fixture(CLI, name, tmp_path, extra=["-histo-after", histo])
    gu.assert_same_as_reference(name, tmp_path, None, check_stderr=False)
    check_run(p, histo, want, open(os.path.join(d, "ref", "stderr.txt"), "rb").read())


def test_histo_after_stops_before_correcting_when_the_bases_will_not_fit(tmp_path):
    d = os.path.join(gu.GOLDEN, PAIRED)
    p = subprocess.run([CLI] + fixture_args(PAIRED) + ["-od", str(tmp_path), "-histo-after", str(tmp_path / "h")], cwd=d,
                       env=dict(os.environ, RC_HBM_FREE_MB="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"-histo-after" in p.stderr and b"Processed" not in p.stderr
