"""CPU: the command line of `rcorrector` (rc_options.cpp).  parse_options and the checks on the kinds of the inputs come before
the first call into the library, so the built binary answers everything here without a GPU: the help text, every usage error
with its exact message and status 1, a flag whose value is missing, which of two mistakes is reported, an unknown argument --
and tests/hostmain/options_test.cpp calls parse_options directly for the clamps and the order of the inputs.

tests/golden/cli/help.txt and the messages of TWO_MISTAKES were recorded from the binary of the commit before the command line
became a table; USAGE passed against that binary too, except its last two rows (there the checks followed the table build)."""
import os
import subprocess

import pytest

import rcorrector_amd
from test_hostmain import ROOT, build_host_test

TOP = 1 << 28
BASE = ["-p", "nope_1.fq", "nope_2.fq", "-k", "23"]   # (files that do not exist: nothing is opened before the checks)
VERBOSE_SMALL = "(small batches through the transcript's entry point: run the %s without it)"
USAGE = [   # arguments behind BASE -> the whole of stderr
    (["-weak-ends", "-verbose"], "rcorrector: usage: -weak-ends cannot be combined with -verbose (the transcript's entry point takes no weak-k-mer profile)\n"),
    (["-depth-tags", "-verbose"], "rcorrector: usage: -depth-tags cannot be combined with -verbose (the transcript's entry point takes no k-mer depth)\n"),
    (["-depth", "F", "-verbose"], "rcorrector: usage: -depth cannot be combined with -verbose (the transcript's entry point takes no k-mer depth)\n"),
    (["-depth-max", "0"], "rcorrector: usage: -depth-max must be 1..%d\n" % TOP),
    (["-dups", "F", "-verbose"], "rcorrector: usage: -dups cannot be combined with -verbose " + VERBOSE_SMALL % "census" + "\n"),
    (["-recurrent", "F", "-verbose"], "rcorrector: usage: -recurrent cannot be combined with -verbose " + VERBOSE_SMALL % "census" + "\n"),
    (["-recurrent", "F", "-recurrent-max", "0"], "rcorrector: usage: -recurrent-max must be 1..%d\n" % TOP),
    (["-recurrent", "F", "-recurrent-min", "0"], "rcorrector: usage: -recurrent-min must be 1..-recurrent-max\n"),
    (["-recurrent", "F", "-recurrent-top", "-1"], "rcorrector: usage: -recurrent-top must be 0..%d\n" % TOP),
    (["-trust-by-pos", "F", "-verbose"], "rcorrector: usage: -trust-by-pos cannot be combined with -verbose " + VERBOSE_SMALL % "profile" + "\n"),
    (["-overlap", "F", "-verbose"], "rcorrector: usage: -overlap cannot be combined with -verbose " + VERBOSE_SMALL % "report" + "\n"),
    (["-overlap", "F", "-overlap-min", "0"], "rcorrector: usage: -overlap-min must be 1..1023\n"),
    (["-overlap", "F", "-overlap-mm", "51"], "rcorrector: usage: -overlap-mm must be 0..50\n"),
    (["-dups", "F", "-dups-max", "0"], "rcorrector: usage: -dups-max must be 1..%d\n" % TOP),
    (["-weak-min", "0"], "rcorrector: usage: -weak-min must be at least 1\n"),
    (["-histo", "F", "-histo-max", "0"], "rcorrector: -histo-max must be 1..%d\n" % TOP),
    # what depends on the kinds of the inputs alone (keep these two last: see the docstring)
    (["-r", "nope.fq", "-dups", "F"], "rcorrector: usage: -dups counts reads or pairs, not both in one census: give single-end files (-r) or paired ones (-p / -i), not a mix\n"),
    (["-r", "nope.fq", "-overlap", "F"], "rcorrector: usage: -overlap compares the two mates of a pair: give paired files (-p / -i), no single-end ones (-r)\n"),
]
TWO_MISTAKES = [
    (["-weak-ends", "-verbose", "-depth-max", "0"], USAGE[0][1]),
    (["-recurrent", "F", "-recurrent-max", "0", "-recurrent-min", "0"], USAGE[6][1]),
    (["-overlap", "F", "-overlap-min", "0", "-overlap-mm", "99"], USAGE[11][1]),
]
VALUE_FLAGS = ["-r", "-p", "-i", "-od", "-c", "-k", "-t", "-maxcor", "-maxcorK", "-wk", "-verbose-iter", "-gpus", "-batch", "-inflight", "-write-dump",
               "-histo", "-histo-max", "-histo-after", "-report", "-dups", "-dups-max", "-recurrent", "-recurrent-min", "-recurrent-top",
               "-recurrent-max", "-trust-by-pos", "-overlap", "-overlap-min", "-overlap-mm", "-weak-min", "-depth", "-depth-max"]


@pytest.fixture(scope="module")
def cli():
    rcorrector_amd.build_library()
    return os.path.join(ROOT, "rcorrector_amd", "rcorrector")


def run(binary, args, cwd):
    return subprocess.run([binary] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_help_is_the_recorded_text(cli, tmp_path):
    want = open(os.path.join(ROOT, "tests", "golden", "cli", "help.txt"), "rb").read()
    for args in (["-h"], [], BASE + ["-h"]):
        p = run(cli, args, tmp_path)
        assert p.returncode == 0 and p.stdout == b"" and p.stderr == want, args


@pytest.mark.parametrize("row", range(len(USAGE)), ids=["_".join(a) for a, _ in USAGE])
def test_usage_errors(cli, row, tmp_path):
    args, message = USAGE[row]
    p = run(cli, BASE + ["-od", "od"] + args, tmp_path)
    assert p.returncode == 1 and p.stderr.decode() == message and p.stdout == b""
    # nothing was opened or created but the -od directory (the reference's main.cpp makes it while it reads the arguments)
    assert os.listdir(str(tmp_path)) == ["od"] and os.listdir(str(tmp_path / "od")) == []


def test_a_flag_without_its_value(cli, tmp_path):
    for flag in VALUE_FLAGS:
        for args in ([flag], BASE + [flag]) + ((["-p", "nope_1.fq"],) if flag == "-p" else ()):
            p = run(cli, args, tmp_path)
            assert p.returncode == 1 and p.stderr.decode() == "rcorrector: usage: %s needs a value\n" % flag, (args, p.returncode, p.stderr)
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("row", range(len(TWO_MISTAKES)))
def test_two_mistakes_report_the_first_check(cli, row, tmp_path):
    args, message = TWO_MISTAKES[row]
    p = run(cli, BASE + args, tmp_path)
    assert p.returncode == 1 and p.stderr.decode() == message


def test_an_unknown_argument_ends_the_run_with_status_0(cli, tmp_path):
    p = run(cli, BASE + ["-nope", "-weak-min", "0"], tmp_path)
    assert p.returncode == 0 and p.stderr == b"Unknown argument: -nope\n" and p.stdout == b""
    # the arguments are read in order: a dump that cannot be opened in front of it is reported first, as it always was
    p = run(cli, BASE + ["-c", "nope.jf", "-nope"], tmp_path)
    assert p.returncode == 1 and p.stderr == b"Could not open file nope.jf\n"


def test_clamps_and_input_order_of_parse_options(cli, tmp_path):
    exe = str(tmp_path / "options_test")
    build_host_test(os.path.join(ROOT, "tests", "hostmain", "options_test.cpp"), exe)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert p.returncode == 0 and p.stdout.decode().rstrip().endswith("ok"), p.stdout.decode()
    # with arguments it parses them as its own command line: the value that is missing ends it like the binary
    p = subprocess.run([exe, "-k", "25", "-p", "a"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stderr == b"rcorrector: usage: -p needs a value\n"
