"""GPU, end to end: tools/read_normalize over rc_read_depth_device + rc_norm_select_device.  The reads of fx_pe_k23 (-p, -i; its
pairs' depths lie between 0 and 15) and of fx_highcov (-r; depths up to 7 457), each with a poly-N unit, a unit with one valid
mate, a unit too short for a window and a unit of k-mers the dump lacks written behind them into tmp_path; against the dump
(-c) and against the table counted from the input.  The report, the list and every output file are compared byte for byte
with what tests/test_read_depth.py's restatement and tests/norm_model.py give.  Before anything runs, the MODEL's outcome is
held to show all four outcomes and both ways of being kept.  The runs are the tool's main() in this process; one test runs the
command itself, twice."""
import gzip
import importlib.machinery
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import norm_model as nm
from test_read_depth import restate
from test_read_screen import counts_of_reads
from test_weak_profile import dump_counts

pytestmark = pytest.mark.gpu
TOOL = os.path.join(gu.ROOT, "tools", "read_normalize")
K = 23


@pytest.fixture(scope="module")
def tool():
    loader = importlib.machinery.SourceFileLoader("read_normalize", TOOL)
    spec = importlib.util.spec_from_loader("read_normalize", loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


def fastq_records(path):
    """(name, sequence, the record's four lines) of a four-line FASTQ file"""
    lines = open(path, "rb").read().split(b"\n")
    return [(lines[i].split()[0][1:], lines[i + 1], b"\n".join(lines[i:i + 4]) + b"\n") for i in range(0, len(lines) - 1, 4)]


def extra_units(rng, mate1_of, mate2_of):
    """the units no fixture holds, as (name stem, sequence of mate 1, sequence of mate 2)"""
    novel = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 90)) for _ in range(2)]
    return [("polyN", b"N" * 70, b"N" * 64), ("onevalid", b"N" * 50, mate2_of), ("othervalid", mate1_of, b"ACGTNACGT" * 6),
            ("short", b"ACGTACGTAC", b"ACGTACGTACGTACGTACGTAC"), ("novel", novel[0], novel[1])]


def fq(name, seq):
    return (name, seq, b"@" + name + b" added\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """the input files and, per input kind, its units: lists of mates, a mate a (name, sequence, text) triple"""
    d = tmp_path_factory.mktemp("norm_in")
    rng = np.random.default_rng(20250611)
    pe = [fastq_records(os.path.join(gu.GOLDEN, "fx_pe_k23", "reads_%d.fq" % m)) for m in (1, 2)]
    pairs = [list(p) for p in zip(*pe)]
    for stem, s1, s2 in extra_units(rng, pe[0][0][1], pe[1][0][1]):
        pairs.append([fq(stem.encode() + b"/1", s1), fq(stem.encode() + b"/2", s2)])
    paths = {"left": str(d / "left.fq"), "right": str(d / "right.fq"), "inter": str(d / "inter.fq"), "left_gz": str(d / "lz.fq.gz"),
             "right_gz": str(d / "rz.fq.gz"), "single": str(d / "single.fq"), "fasta": str(d / "single.fa")}
    open(paths["left"], "wb").write(b"".join(p[0][2] for p in pairs))
    open(paths["right"], "wb").write(b"".join(p[1][2] for p in pairs))
    open(paths["inter"], "wb").write(b"".join(m[2] for p in pairs for m in p))
    for src, dst in (("left", "left_gz"), ("right", "right_gz")):
        with gzip.open(paths[dst], "wb") as f:
            f.write(open(paths[src], "rb").read())
    se = fastq_records(os.path.join(gu.GOLDEN, "fx_highcov", "reads.fq"))
    singles = [[r] for r in se] + [[fq(stem.encode(), s1)] for stem, s1, _ in extra_units(rng, se[0][1], se[1][1])]
    open(paths["single"], "wb").write(b"".join(u[0][2] for u in singles))
    # the same reads as FASTA wrapped at 60: a record comes back as its header line and its sequence on one line
    with open(paths["fasta"], "wb") as f:
        for (name, seq, _), in singles:
            f.write(b">" + name + b" as fasta\n" + b"".join(seq[j:j + 60] + b"\n" for j in range(0, len(seq), 60)))
    fasta_units = [[(name, seq, b">" + name + b" as fasta\n" + seq + b"\n")] for (name, seq, _), in singles]
    return {"paths": paths, "pairs": pairs, "singles": singles, "fasta_units": fasta_units,
            "dump": {n: os.path.join(gu.GOLDEN, n, "dump.jf") for n in ("fx_pe_k23", "fx_highcov")}}


_rows_cache = {}


def expected(units, counts, key, target, min_cov, seed, depth_max, files):
    """what a run must give: {"report", "list", "stderr", "outs": one text per output file, "keep", "depths"}; files: for every
    mate of a unit the output file its record goes to.  The depth rows are computed once per (input, table) -- `key`"""
    if key not in _rows_cache:
        _rows_cache[key] = [tuple(restate(m[1], K, counts) for m in u) for u in units]
    mates = len(units[0])
    rows = [r for u in _rows_cache[key] for r in u]
    keep, tally, depths = nm.select(rows, len(units), 0 if mates == 1 else 2, 0, target, min_cov, seed, depth_max)
    nb = depth_max + 1
    lines = ["k\t%d" % K, "target\t%d" % target, "min_cov\t%d" % min_cov, "seed\t%d" % seed, "table_kmers\t%d" % len(counts),
             "units\t%d\t%s" % (len(units), "pairs" if mates == 2 else "reads"),
             "kept\t%d" % keep.count(nm.KEPT), "over\t%d" % keep.count(nm.OVER), "low\t%d" % keep.count(nm.LOW), "novalid\t%d" % keep.count(nm.NOVALID)]
    folded = [None if d is None else min(d, depth_max) for d in depths]
    for d in sorted({x for x in folded if x is not None}):
        lines.append("depth\t%d\t%d\t%d" % (d, folded.count(d), sum(1 for x, o in zip(folded, keep) if x == d and o == nm.KEPT)))
    assert tally[4:4 + nb] == [folded.count(d) for d in range(nb)]          # (the model's tally says the same)
    outs = [b""] * (max(files) + 1)
    for u, o in zip(units, keep):
        if o == nm.KEPT:
            for f, m in zip(files, u):
                outs[f] += m[2]
    listing = b"".join(u[0][0] + ("\t%d\t%s\n" % (d or 0, nm.NAMES[o])).encode() for u, d, o in zip(units, depths, keep))
    err = "read_normalize: %d %s, %d kept (%.2f %%)" % (len(units), "pairs" if mates == 2 else "reads", keep.count(nm.KEPT),
                                                        100.0 * keep.count(nm.KEPT) / len(units))
    return {"report": "\n".join(lines) + "\n", "list": listing, "stderr": err, "outs": outs, "keep": keep, "depths": depths}


def assert_all_outcomes(want, target):
    """on the MODEL's output: the four outcomes occur, and so do both ways of being kept"""
    keep, depths = want["keep"], want["depths"]
    assert set(keep) == {nm.OVER, nm.KEPT, nm.LOW, nm.NOVALID}
    assert any(o == nm.KEPT and d <= target for o, d in zip(keep, depths)) and any(o == nm.KEPT and d > target for o, d in zip(keep, depths))


def run(tool, capfd, args, want, out_names, tmp_path, tag):
    """tool.main(args + outputs) in this process; every file against `want`.  Returns the output directory."""
    od = tmp_path / tag
    report, listing = str(tmp_path / (tag + ".report")), str(tmp_path / (tag + ".list"))
    capfd.readouterr()
    rc = tool.main(list(args) + ["-od", str(od), "-o", report, "-list", listing])
    cap = capfd.readouterr()
    assert rc == 0, cap.err
    assert open(report).read() == want["report"]
    assert open(listing, "rb").read() == want["list"]
    assert sorted(os.listdir(str(od))) == sorted(out_names)
    for name, text in zip(out_names, want["outs"]):
        assert open(str(od / name), "rb").read() == text, name
    assert cap.err.splitlines()[-1] == want["stderr"] and cap.out == ""
    return od


def counted(units):
    return counts_of_reads([m[1] for u in units for m in u], K)


# ---- paired input: -p and -i, counted and against the dump, batches, seeds, .gz ------------------------------------------------
def test_pairs_counted_and_from_a_dump_in_two_files_and_interleaved(tool, data, capfd, tmp_path):
    p, pairs = data["paths"], data["pairs"]
    base = ["-k", str(K), "-target", "5", "-min-cov", "2", "-seed", "11"]
    cc, dc = counted(pairs), dump_counts("fx_pe_k23")
    want_c = expected(pairs, cc, "pe counted", 5, 2, 11, 10000, (0, 1))
    want_d = expected(pairs, dc, "pe dump", 5, 2, 11, 10000, (0, 1))
    for want in (want_c, want_d):
        assert_all_outcomes(want, 5)
    assert want_d["depths"][-1] == 0 and want_c["depths"][-1] == 1 and want_d["keep"][-1] == nm.LOW       # the unit of k-mers the dump lacks
    assert want_d["depths"][-5:-1] == [None, want_d["depths"][-4], want_d["depths"][-3], None] and want_d["depths"][-4] is not None
    names = ["left.norm.fq", "right.norm.fq"]
    # counted, the default batch; -batch 7: the same files byte for byte
    od = run(tool, capfd, base + ["-p", p["left"], p["right"]], want_c, names, tmp_path, "pc")
    run(tool, capfd, base + ["-p", p["left"], p["right"], "-batch", "7"], want_c, names, tmp_path, "pc7")
    left, right = (open(str(od / n), "rb").read().split(b"\n") for n in names)
    assert len(left) == len(right) and [x.split(b"/")[0] for x in left[0::4]] == [x.split(b"/")[0] for x in right[0::4]]      # the files stay in step
    # against the dump; interleaved keeps both mates of a kept pair; .gz input
    run(tool, capfd, base + ["-p", p["left"], p["right"], "-c", data["dump"]["fx_pe_k23"], "-batch", "64"], want_d, names, tmp_path, "pd")
    want_i = expected(pairs, dc, "pe dump", 5, 2, 11, 10000, (0, 0))
    run(tool, capfd, base + ["-i", p["inter"], "-c", data["dump"]["fx_pe_k23"]], want_i, ["inter.norm.fq"], tmp_path, "id")
    assert want_i["outs"][0] == b"".join(m[2] for u, o in zip(pairs, want_d["keep"]) if o == nm.KEPT for m in u)
    run(tool, capfd, base + ["-p", p["left_gz"], p["right_gz"], "-batch", "100"], want_c, ["lz.norm.fq", "rz.norm.fq"], tmp_path, "gz")
    # another seed: another kept set, the same low and novalid units
    other = expected(pairs, cc, "pe counted", 5, 2, 12, 10000, (0, 1))
    assert other["keep"] != want_c["keep"] and [o in (nm.LOW, nm.NOVALID) and o for o in other["keep"]] == [o in (nm.LOW, nm.NOVALID) and o for o in want_c["keep"]]
    run(tool, capfd, base[:-1] + ["12", "-p", p["left"], p["right"]], other, names, tmp_path, "seed12")
    # a target above every depth keeps every unit with D >= min_cov
    high = expected(pairs, cc, "pe counted", 1000, 2, 11, 10000, (0, 1))
    assert nm.OVER not in high["keep"] and all((o == nm.KEPT) == (d is not None and d >= 2) for o, d in zip(high["keep"], high["depths"]))
    run(tool, capfd, ["-k", str(K), "-target", "1000", "-min-cov", "2", "-seed", "11", "-p", p["left"], p["right"]], high, names, tmp_path, "high")


# ---- single-end input: FASTQ and FASTA, a folded depth histogram, the command itself -------------------------------------------
def test_single_reads_from_a_dump_with_a_folded_histogram_and_as_fasta(tool, data, capfd, tmp_path):
    p = data["paths"]
    dc = dump_counts("fx_highcov")
    args = ["-k", str(K), "-target", "2000", "-min-cov", "100", "-seed", "3", "-depth-max", "7000", "-c", data["dump"]["fx_highcov"]]
    want = expected(data["singles"], dc, "se dump", 2000, 100, 3, 7000, (0,))
    assert_all_outcomes(want, 2000)
    assert max(d for d in want["depths"] if d is not None) > 7000 and "\ndepth\t7000\t" in want["report"]      # the last line folds
    run(tool, capfd, args + ["-r", p["single"], "-batch", "77"], want, ["single.norm.fq"], tmp_path, "se")
    want_fa = expected(data["fasta_units"], dc, "se dump", 2000, 100, 3, 7000, (0,))
    assert want_fa["keep"] == want["keep"]
    run(tool, capfd, args + ["-r", p["fasta"]], want_fa, ["single.norm.fa"], tmp_path, "fa")
    # two files in one run: the unit numbers run on across the files
    both = expected(data["singles"] + data["fasta_units"], dc, "se dump twice", 2000, 100, 3, 7000, (0,))
    n = len(data["singles"])
    both["outs"] = [b"".join(u[0][2] for u, o in zip(data["singles"], both["keep"][:n]) if o == nm.KEPT),
                    b"".join(u[0][2] for u, o in zip(data["fasta_units"], both["keep"][n:]) if o == nm.KEPT)]
    assert both["keep"][n:] != both["keep"][:n]
    run(tool, capfd, args + ["-r", p["single"], p["fasta"]], both, ["single.norm.fq", "single.norm.fa"], tmp_path, "two")
    # counted from the reads themselves, singletons included
    cc = counted(data["singles"])
    want_c = expected(data["singles"], cc, "se counted", 40, 2, 3, 10000, (0,))
    assert_all_outcomes(want_c, 40)
    run(tool, capfd, ["-k", str(K), "-target", "40", "-min-cov", "2", "-seed", "3", "-r", p["single"]], want_c, ["single.norm.fq"], tmp_path, "sc")


def test_the_command_itself_twice_with_one_seed(data, tmp_path):
    p = data["paths"]
    want = expected(data["pairs"], dump_counts("fx_pe_k23"), "pe dump", 5, 2, 11, 10000, (0, 1))
    runs = []
    for tag in ("a", "b"):
        od = tmp_path / tag
        r = subprocess.run([sys.executable, TOOL, "-k", str(K), "-target", "5", "-min-cov", "2", "-seed", "11", "-c", data["dump"]["fx_pe_k23"],
                            "-p", p["left"], p["right"], "-od", str(od)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout.decode() == want["report"] and r.stderr.decode().splitlines()[-1] == want["stderr"]      # the report on stdout
        runs.append([open(str(od / n), "rb").read() for n in ("left.norm.fq", "right.norm.fq")])
    assert runs[0] == runs[1] == want["outs"]


def test_a_read_of_more_than_1023_bases_is_refused_by_name(tool, data, capfd, tmp_path):
    long_fq = tmp_path / "long.fq"
    long_fq.write_bytes(b"@fine\nACGT\n+\nIIII\n@toolong extra\n" + b"A" * 1024 + b"\n+\n" + b"I" * 1024 + b"\n")
    for extra in ([], ["-c", data["dump"]["fx_pe_k23"]]):          # in the counting pass, and in the selection pass
        capfd.readouterr()
        rc = tool.main(["-k", str(K), "-target", "5", "-r", str(long_fq), "-od", str(tmp_path / "x")] + extra)
        cap = capfd.readouterr()
        assert rc == 1 and cap.out == "" and "read toolong of 1024 bases exceeds the library's 1023" in cap.err and cap.err.count("\n") == 1
    long_fq.write_bytes(b"@fine\nACGT\n+\nIIII\n@justfits\n" + b"A" * 1023 + b"\n+\n" + b"I" * 1023 + b"\n")
    assert tool.main(["-k", str(K), "-target", "2000", "-r", str(long_fq), "-od", str(tmp_path / "y"), "-o", str(tmp_path / "y.report")]) == 0
    assert "\nunits\t2\treads\nkept\t1\nover\t0\nlow\t0\nnovalid\t1\n" in open(str(tmp_path / "y.report")).read()
