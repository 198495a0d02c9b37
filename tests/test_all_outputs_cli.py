"""GPU: every extra output of `rcorrector` armed in one run -- -histo -histo-after -report -weak-ends -depth-tags -depth -dups
-recurrent -trust-by-pos -overlap -- on the smallest paired golden fixture, on one context and on two.

rc_outputs.cpp arms them one after the other before the pipeline and collects them one after the other behind it; the suites
of the single outputs pin what each one writes on its own.  Here: each file of the run with everything armed is byte for byte
the file of a run of the same binary with that output alone, the records carry both kinds of tags, and stderr is the fixture's
golden stderr followed by the outputs' lines in the order they have always had: weak ends, depth, duplicates, recurrent
corrections, trust by position, mate overlap, corrected reads (-report and -histo print none).  That order was recorded from
the binary of the commit before the outputs moved out of main(), on this command line."""
import os
import re
import subprocess

import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu
CLI = os.path.join(gu.ROOT, "rcorrector_amd", "rcorrector")
NAME = "fx_pe_k23"
FILES = ["-histo", "-histo-after", "-report", "-depth", "-dups", "-recurrent", "-trust-by-pos", "-overlap"]   # flag FILE
TAGS = ["-weak-ends", "-depth-tags"]
LINES = [("-weak-ends", b"Weak ends "), ("-depth", b"K-mer depth: "), ("-dups", b"Duplicates: "), ("-recurrent", b"Recurrent corrections: "),
         ("-trust-by-pos", b"Trust by position "), ("-overlap", b"Mate overlap "), ("-histo-after", b"Corrected reads: ")]
RECORDS = ["reads_1.cor.fq", "reads_2.cor.fq"]


def run(od, flags, extra=(), env=None):
    """the fixture's command with `flags` armed (a FILE flag writes <od>/<flag>.out): (stderr, {flag: bytes}, the records)"""
    args = []
    for f in flags:
        args += [f, os.path.join(str(od), f + ".out")] if f in FILES else [f]
    d = os.path.join(gu.GOLDEN, NAME)
    cmd = [CLI] + open(os.path.join(d, "cmd.txt")).read().split() + ["-od", str(od)] + args + list(extra)
    p = subprocess.run(cmd, cwd=d, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    files = {f: open(os.path.join(str(od), f + ".out"), "rb").read() for f in flags if f in FILES}
    return p.stderr, files, [open(os.path.join(str(od), r), "rb").read() for r in RECORDS]


@pytest.fixture(scope="module")
def alone(tmp_path_factory):
    """every output armed alone, on one context: {flag: (stderr, its file or None, the records)}"""
    out = {}
    for f in FILES + TAGS:
        err, files, records = run(tmp_path_factory.mktemp("alone"), [f])
        out[f] = (err, files.get(f), records)
    return out


@pytest.mark.parametrize("contexts", [1, 2])
def test_all_outputs_at_once_equal_each_alone(contexts, alone, tmp_path):
    extra, env = ([], {}) if contexts == 1 else (["-gpus", "2", "-batch", "64"], {"RC_SHARED_GPU": "1"})
    err, files, records = run(tmp_path, FILES + TAGS, extra, env)
    for f in FILES:
        assert alone[f][1] and files[f] == alone[f][1], "%s differs from the run with %s alone" % (f, f)
    # the records: without the tags the golden output, without one kind of tag the run with the other kind alone
    golden_err = open(os.path.join(gu.GOLDEN, NAME, "ref", "stderr.txt"), "rb").read()
    weak, depth = rb" bad_(?:prefix|suffix)=\d+", rb" kdepth=\d+:\d+:\d+"
    for i, r in enumerate(RECORDS):
        assert re.search(weak, records[i]) and re.search(depth, records[i])
        assert re.sub(depth, b"", records[i]) == alone["-weak-ends"][2][i] and re.sub(weak, b"", records[i]) == alone["-depth-tags"][2][i]
        assert re.sub(weak, b"", re.sub(depth, b"", records[i])) == open(os.path.join(gu.GOLDEN, NAME, "ref", r), "rb").read()
        assert alone["-report"][2][i] == alone["-overlap"][2][i] == open(os.path.join(gu.GOLDEN, NAME, "ref", r), "rb").read()
    # stderr: the golden lines, then one line per output in the fixed order, each the line of the run with that output alone
    want = golden_err
    for f, prefix in LINES:
        assert alone[f][0].startswith(golden_err)
        line = alone[f][0][len(golden_err):]
        assert line.startswith(prefix) and line.count(b"\n") == 1 and line.endswith(b"\n"), (f, line)
        want += line
    assert alone["-depth-tags"][0] == alone["-depth"][0]
    assert alone["-histo"][0] == alone["-report"][0] == golden_err
    assert err == want, "stderr:\n%s\nexpected:\n%s" % (err.decode(), want.decode())
