"""GPU: `rcorrector -weak-ends [-weak-min INT]` -- the reference's dormant ` bad_prefix=N` / ` bad_suffix=N` record tags
(Reads.h:396-412), filled from the weak-k-mer profile of the corrected reads.

For four golden fixtures, through the byte transport (-c), the packed one (-c -packed) and the one-pass resident one (no -c;
-write-dump leaves the table the run counted, so that the yardstick has it): the output with the tags taken out is the output
of the same run without the flag byte for byte (for the -c runs also the golden ref/ files), the tags of every record are what
tests/test_weak_profile.py's pure-Python restatement gives for that record's sequence against the dump, no unfixable record
carries one, and the extra stderr line counts what the restatement counts."""
import os
import re
import subprocess

import pytest

import golden_util as gu
from test_weak_profile import canonical, restate

pytestmark = pytest.mark.gpu
CLI = os.path.join(gu.ROOT, "rcorrector_amd", "rcorrector")
NAMES = ["fx_pe_k23", "fx_il_k23", "fa_se_k23", "fx_edge"]
TAGS = re.compile(rb" bad_prefix=\d+| bad_suffix=\d+")
WEAK_LINE = re.compile(rb"Weak ends \(k-mers counted below (\d+)\): (\d+) reads with a bad prefix, (\d+) with a bad suffix, (\d+) without a solid k-mer\n")


def fixture_args(name):
    return open(os.path.join(gu.GOLDEN, name, "cmd.txt")).read().split()


def run(name, outdir, args, extra=(), env=None, ok=True):
    p = subprocess.run([CLI] + list(args) + ["-od", str(outdir)] + list(extra), cwd=os.path.join(gu.GOLDEN, name),
                       env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert (p.returncode == 0) == ok, p.stderr.decode()
    return p


def outputs(outdir):
    return {f: open(os.path.join(str(outdir), f), "rb").read() for f in sorted(os.listdir(str(outdir))) if ".cor." in f}


def dump_dict(path):
    d, cnt = {}, 0
    for ln in open(path, "rb").read().split():
        if ln.startswith(b">"):
            cnt = int(ln[1:])
        else:
            d[canonical(ln)] = cnt
    return d


def check_tags(files, k, counts, min_count):
    """every record's tags against the restatement on that record's own sequence; returns the three stderr counts and the unfixable records"""
    n_pre = n_suf = n_none = n_tagged = n_unfixable = 0
    for text in files.values():
        lines = text.split(b"\n")
        step = 4 if lines[0].startswith(b"@") else 2
        for i in range(0, len(lines) - 1, step):
            head, seq = lines[i], lines[i + 1]
            _, pre, suf, unc = restate(seq, k, counts, min_count)
            n_pre += pre > 0
            n_suf += suf > 0
            n_none += len(seq) > 0 and unc == len(seq)
            tail = head[re.search(rb" l:-?\d+ m:-?\d+ h:-?\d+", head).end():]
            if tail.startswith(b" unfixable_error"):
                n_unfixable += 1
                assert tail == b" unfixable_error", head          # that branch of the reference has no tags
                continue
            want = (b" cor" if tail.startswith(b" cor") else b"") + (b" bad_prefix=%d" % pre if pre > 0 else b"") + (b" bad_suffix=%d" % suf if suf > 0 else b"")
            assert tail == want, (head, want)
            n_tagged += tail != (b" cor" if tail.startswith(b" cor") else b"")
    assert n_tagged > 0
    return n_pre, n_suf, n_none, n_unfixable


@pytest.mark.parametrize("transport", ["bytes", "packed", "resident"])
@pytest.mark.parametrize("name", NAMES)
def test_weak_ends_tags_and_nothing_else(name, transport, tmp_path):
    args = fixture_args(name)
    k = int(args[args.index("-k") + 1])
    dump = os.path.join(gu.GOLDEN, name, "dump.jf")
    extra, env = ["-batch", "100"], {}
    if transport == "packed":
        extra += ["-packed"]
    elif transport == "resident":
        i = args.index("-c")
        del args[i:i + 2]
        dump = str(tmp_path / "table.jf")
        extra += ["-write-dump", dump]
        env = {"RC_RESIDENT": "1"}
    od, od0 = tmp_path / "with", tmp_path / "without"
    min_count = 3 if name == "fx_il_k23" else 1
    weak = ["-weak-ends"] + (["-weak-min", "3"] if min_count == 3 else [])
    p = run(name, od, args, extra + weak, env)
    p0 = run(name, od0, args, extra, env)
    got, plain = outputs(od), outputs(od0)
    assert got.keys() == plain.keys() and len(got) > 0
    for f in got:
        assert TAGS.sub(b"", got[f]) == plain[f], f
        assert TAGS.search(got[f]) and not TAGS.search(plain[f])
        if transport != "resident":
            assert TAGS.sub(b"", got[f]) == open(os.path.join(gu.GOLDEN, name, "ref", f), "rb").read(), f
    n_pre, n_suf, n_none, n_unfixable = check_tags(got, k, dump_dict(dump), min_count)
    assert n_unfixable > 0 or transport == "resident"   # (the goldens hold unfixable reads; a table counted from the reads themselves may leave none)
    m = WEAK_LINE.search(p.stderr)
    assert m and tuple(int(x) for x in m.groups()) == (min_count, n_pre, n_suf, n_none)
    assert WEAK_LINE.sub(b"", p.stderr) == p0.stderr and not WEAK_LINE.search(p0.stderr)   # one extra line, only under the flag
    assert p.stdout == p0.stdout


@pytest.mark.parametrize("variant", ["two_contexts", "gz", "lanes_off"])
def test_weak_ends_with_several_gpus_gz_and_lanes_off(variant, tmp_path):
    name = "fx_pe_k23"
    args = fixture_args(name)
    k = int(args[args.index("-k") + 1])
    extra, env = ["-batch", "64", "-inflight", "4"], {}
    if variant == "two_contexts":
        extra, env = ["-gpus", "2", "-batch", "64", "-inflight", "2"], {"RC_SHARED_GPU": "1"}
    elif variant == "lanes_off":
        env = {"RC_SLOT_LANES": "0"}
    else:
        import gzip
        d = os.path.join(gu.GOLDEN, name)
        for f in ("reads_1.fq", "reads_2.fq"):
            with gzip.open(str(tmp_path / (f + ".gz")), "wb") as z:
                z.write(open(os.path.join(d, f), "rb").read())
        args = ["-p", str(tmp_path / "reads_1.fq.gz"), str(tmp_path / "reads_2.fq.gz"), "-k", str(k), "-c", "dump.jf"]
    od = tmp_path / "with"
    p = run(name, od, args, extra + ["-weak-ends"], env)
    got = outputs(od)
    if variant == "gz":
        import gzip
        got = {f[:-3]: gzip.decompress(t) for f, t in got.items()}
    for f in got:
        assert TAGS.sub(b"", got[f]) == open(os.path.join(gu.GOLDEN, name, "ref", f), "rb").read(), f
    counts = check_tags(got, k, dump_dict(os.path.join(gu.GOLDEN, name, "dump.jf")), 1)
    m = WEAK_LINE.search(p.stderr)
    assert m and tuple(int(x) for x in m.groups()) == (1,) + counts[:3] and counts[3] > 0


def test_weak_ends_with_verbose_is_a_usage_error(tmp_path):
    p = run("fx_pe_k23", tmp_path, fixture_args("fx_pe_k23"), ["-weak-ends", "-verbose"], ok=False)
    assert p.returncode != 0 and b"usage" in p.stderr and b"-weak-ends" in p.stderr and b"-verbose" in p.stderr
    assert outputs(tmp_path) == {} or all(len(t) == 0 for t in outputs(tmp_path).values())
    p = run("fx_pe_k23", tmp_path, fixture_args("fx_pe_k23"), ["-weak-ends", "-weak-min", "0"], ok=False)
    assert b"usage" in p.stderr and b"-weak-min" in p.stderr
