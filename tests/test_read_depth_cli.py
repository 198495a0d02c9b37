"""GPU: `rcorrector -depth-tags` / `-depth FILE [-depth-max INT]` -- ` kdepth=Q1:MED:Q3` on the records, the quartiles of the counts
that every corrected read's k-mers have in the table, and the reads by median.

On three golden fixtures (paired FASTQ, single-end FASTQ with reads that have no valid k-mer window, FASTA): the output with the
tags taken out is the golden ref/ output byte for byte, every record's tag is what tests/test_read_depth.py's pure-Python
restatement gives for that record's sequence against the dump, reads without a valid window carry none, the report is the
histogram of the restatement's medians and the extra stderr line counts what the restatement counts -- through the byte and the
packed transport, one and four batches in flight, and from .gz input."""
import gzip
import os
import re

import pytest

import golden_util as gu
from test_read_depth import restate
from test_weak_profile_cli import CLI, dump_dict, fixture_args, outputs, run

pytestmark = pytest.mark.gpu
NAMES = ["fx_pe_k23", "fx_edge", "fa_se_k23"]
TAG = re.compile(rb" kdepth=(\d+):(\d+):(\d+)")
HEAD = re.compile(rb"^(.*? l:-?\d+ m:-?\d+ h:-?\d+)( unfixable_error| cor)?((?: bad_prefix=\d+)?(?: bad_suffix=\d+)?)((?: kdepth=\d+:\d+:\d+)?)$")
DEPTH_LINE = re.compile(rb"K-mer depth: (\d+) reads with a valid k-mer window, (\d+) of them with a median of 0; the median of the reads' medians is (\d+)"
                        rb"( or more \(the last bin, -depth-max\))?\n")
_counts = {}


def counts_of(name):
    if name not in _counts:
        _counts[name] = dump_dict(os.path.join(gu.GOLDEN, name, "dump.jf"))
    return _counts[name]


def records(files, mates_by_file):
    """(mate, header, sequence) of every record; mates_by_file: the output files in mate order"""
    for mate, f in enumerate(mates_by_file):
        lines = files[f].split(b"\n")
        step = 4 if lines[0].startswith(b"@") else 2
        for i in range(0, len(lines) - 1, step):
            yield mate, lines[i], lines[i + 1]


def check_tags(files, k, counts, depth_max=10000):
    """every record's tag against the restatement of that record's own sequence; returns what the report and the stderr line hold"""
    order = sorted(files)
    reads, novalid, hist, tagged = [0, 0], [0, 0], [{}, {}], 0
    for mate, head, seq in records(files, order):
        n, q1, med, q3 = restate(seq, k, counts)
        m = HEAD.match(head)
        assert m, head                                          # l:m:h, cor, the -weak-ends tags, then kdepth: the stated order
        reads[mate] += 1
        if n == 0:
            novalid[mate] += 1
            assert m.group(4) == b"", head                      # no valid window: no tag
            continue
        assert m.group(4) == b" kdepth=%d:%d:%d" % (q1, med, q3), (head, (n, q1, med, q3))
        tagged += 1
        d = min(med, depth_max)
        hist[mate][d] = hist[mate].get(d, 0) + 1
    assert tagged > 0
    return reads, novalid, hist


def report_text(k, reads, novalid, hist, mates):
    t = "k\t%d\n" % k
    t += "".join("reads\t%d\t%d\n" % (m + 1, reads[m]) for m in range(mates))
    t += "".join("novalid\t%d\t%d\n" % (m + 1, novalid[m]) for m in range(mates))
    for d in sorted(set(hist[0]) | set(hist[1])):
        t += "median\t%d\t%s\n" % (d, "\t".join(str(hist[m].get(d, 0)) for m in range(mates)))
    return t.encode()


def stderr_counts(hist):
    both = {}
    for h in hist:
        for d, c in h.items():
            both[d] = both.get(d, 0) + c
    n = sum(both.values())
    seen = 0
    for d in sorted(both):
        seen += both[d]
        if seen > (n - 1) // 2:
            return n, both.get(0, 0), d
    return 0, 0, 0


@pytest.mark.parametrize("variant", ["bytes", "packed", "inflight1", "inflight4", "depth_max_3", "with_weak_ends"])
@pytest.mark.parametrize("name", NAMES)
def test_depth_tags_and_report_against_the_restatement(name, variant, tmp_path):
    args = fixture_args(name)
    k = int(args[args.index("-k") + 1])
    mates = 2 if "-p" in args else 1
    extra = ["-batch", "100"] + {"packed": ["-packed"], "inflight1": ["-inflight", "1"], "inflight4": ["-inflight", "4"]}.get(variant, [])
    depth_max = 3 if variant == "depth_max_3" else 10000
    rep = str(tmp_path / "depth.tsv")
    flags = ["-depth-tags", "-depth", rep] + (["-depth-max", "3"] if variant == "depth_max_3" else []) + (["-weak-ends"] if variant == "with_weak_ends" else [])
    od = tmp_path / "with"
    p = run(name, od, args, extra + flags)
    got = outputs(od)
    assert len(got) == mates
    weak = re.compile(rb" bad_prefix=\d+| bad_suffix=\d+")
    for f in got:
        plain = TAG.sub(b"", got[f])
        if variant == "with_weak_ends":
            assert weak.search(plain)
            plain = weak.sub(b"", plain)
        assert plain == open(os.path.join(gu.GOLDEN, name, "ref", f), "rb").read(), f     # sequence and quality lines never change
    reads, novalid, hist = check_tags(got, k, counts_of(name), depth_max)
    if name == "fx_edge":
        assert novalid[0] > 0
    assert open(rep, "rb").read() == report_text(k, reads, novalid, hist, mates)
    if variant == "depth_max_3":
        assert max(hist[0]) == 3                                                           # (the last bin is in use)
    m = DEPTH_LINE.search(p.stderr)
    n, zero, mm = stderr_counts(hist)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (n, zero, mm), p.stderr
    assert (m.group(4) is not None) == (mm == depth_max)
    want_err = open(os.path.join(gu.GOLDEN, name, "ref", "stderr.txt"), "rb").read()
    rest = DEPTH_LINE.sub(b"", p.stderr)
    if variant == "with_weak_ends":
        assert p.stderr.index(b"Weak ends (") < p.stderr.index(b"K-mer depth:")
        rest = re.sub(rb"Weak ends \(.*\n", b"", rest)
    assert rest == want_err and p.stdout == b""


@pytest.mark.parametrize("flag", ["tags_only", "report_only"])
def test_either_flag_alone_and_gz_input(flag, tmp_path):
    name = "fx_pe_k23"
    d = os.path.join(gu.GOLDEN, name)
    for f in ("reads_1.fq", "reads_2.fq"):
        with gzip.open(str(tmp_path / (f + ".gz")), "wb") as z:
            z.write(open(os.path.join(d, f), "rb").read())
    args = ["-p", str(tmp_path / "reads_1.fq.gz"), str(tmp_path / "reads_2.fq.gz"), "-k", "23", "-c", "dump.jf"]
    rep = str(tmp_path / "depth.tsv")
    od = tmp_path / "out"
    p = run(name, od, args, ["-batch", "64"] + (["-depth-tags"] if flag == "tags_only" else ["-depth", rep]))
    got = {f[:-3]: gzip.decompress(t) for f, t in outputs(od).items()}
    ref = {f: open(os.path.join(d, "ref", f), "rb").read() for f in got}
    assert len(got) == 2 and DEPTH_LINE.search(p.stderr)
    if flag == "tags_only":
        assert {f: TAG.sub(b"", t) for f, t in got.items()} == ref and not os.path.exists(rep)
        check_tags(got, 23, counts_of(name))
    else:
        assert got == ref                                              # the report alone annotates nothing
        reads, novalid, hist = [0, 0], [0, 0], [{}, {}]
        for mate, _, seq in records(ref, sorted(ref)):
            n, _, med, _ = restate(seq, 23, counts_of(name))
            reads[mate] += 1
            novalid[mate] += n == 0
            if n:
                hist[mate][med] = hist[mate].get(med, 0) + 1
        assert open(rep, "rb").read() == report_text(23, reads, novalid, hist, 2)


def test_stdout_carries_the_tags(tmp_path):
    name = "fx_pe_k23"
    p = run(name, tmp_path, fixture_args(name), ["-stdout", "-depth-tags", "-batch", "100"])
    p0 = run(name, tmp_path, fixture_args(name), ["-stdout", "-batch", "100"])
    assert TAG.search(p.stdout) and TAG.sub(b"", p.stdout) == p0.stdout and DEPTH_LINE.sub(b"", p.stderr) == p0.stderr


def test_usage_errors(tmp_path):
    for flags, words in ((["-depth-tags", "-verbose"], [b"-depth-tags", b"-verbose"]), (["-depth", str(tmp_path / "d.tsv"), "-verbose"], [b"-depth", b"-verbose"]),
                         (["-depth-tags", "-depth-max", "0"], [b"-depth-max"])):
        p = run("fx_pe_k23", tmp_path, fixture_args("fx_pe_k23"), flags, ok=False)
        assert p.returncode != 0 and b"usage" in p.stderr and all(w in p.stderr for w in words)
        assert outputs(tmp_path) == {} or all(len(t) == 0 for t in outputs(tmp_path).values())


@pytest.mark.parametrize("name", NAMES)
def test_without_the_flags_the_run_is_the_golden_run(name, tmp_path):
    p = gu.run_fixture(CLI, name, tmp_path)
    gu.assert_same_as_reference(name, tmp_path, p.stderr)
    assert p.stdout == b"" and not TAG.search(b"".join(outputs(tmp_path).values())) and b"K-mer depth" not in p.stderr
