"""The recurrent-correction census (include/rcorrector_amd.h: rc_recur_census) as a pure-Python model over strings: the reads
as they went in and the reads as they came out.  The yardstick of the tests, never the library: nothing here imports it.

A change is a position where the two strings differ.  It is contexted when 14 bytes lie on either side of it inside the read
and all 29 bytes of that window of the CORRECTED read are upper-case ACGT; every other change is clipped (counted, no key).
The key packs the window two bits a base (A C G T = 0 1 2 3, first base most significant) with the from code (0..3 for an
upper-case ACGT original byte, else 4) in the low three bits, in the orientation -- as read, or reverse-complemented with the
from code complemented -- whose window is the smaller number."""
import collections

FLANK = 14
WINDOW = 2 * FLANK + 1
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def pack(window):
    w = 0
    for c in window:
        w = (w << 2) | CODE[c]
    return w


def from_code(c):
    return CODE.get(c, 4)


def key_of(window, orig):
    """the key of a 29-letter ACGT window and the original byte (a one-character str)"""
    assert len(window) == WINDOW
    f = from_code(orig)
    w, r = pack(window), pack(revcomp(window))
    assert w != r
    if r < w:
        return (r << 3) | (f if f == 4 else 3 - f)
    return (w << 3) | f


def decode(key):
    """(from_letter, to_letter, 29-mer) of a key"""
    f, w = key & 7, key >> 3
    text = "".join("ACGT"[(w >> (2 * (WINDOW - 1 - i))) & 3] for i in range(WINDOW))
    return "ACGTN"[f], text[FLANK], text


def _s(x):
    return x.decode("latin-1") if isinstance(x, (bytes, bytearray)) else x


def read_changes(before, after):
    """[(p, key or None)] for one read: None = clipped"""
    before, after = _s(before), _s(after)
    assert len(before) == len(after)
    L = len(after)
    out = []
    for p in range(L):
        if before[p] == after[p]:
            continue
        key = None
        if p >= FLANK and p + FLANK < L:
            win = after[p - FLANK:p + FLANK + 1]
            if all(c in CODE for c in win):
                key = key_of(win, before[p])
        out.append((p, key))
    return out


class Census:
    """the census of a sequence of (before, after) reads"""

    def __init__(self):
        self.changes = 0
        self.contexted = 0
        self.keys = collections.Counter()

    def add(self, befores, afters):
        befores, afters = list(befores), list(afters)
        assert len(befores) == len(afters)
        for b, a in zip(befores, afters):
            for _, key in read_changes(b, a):
                self.changes += 1
                if key is not None:
                    self.contexted += 1
                    self.keys[key] += 1
        return self

    def key_list(self):
        return sorted(self.keys.elements())

    def result(self, max_bin, min_count=2, max_sites=1000):
        """what rc_recur_census_get gives, as plain Python"""
        recur = [0] * (max_bin + 1)
        for c in self.keys.values():
            recur[min(c, max_bin)] += 1
        top = sorted(((c, k) for k, c in self.keys.items() if c >= min_count), key=lambda t: (-t[0], t[1]))[:max_sites]
        return {"changes": self.changes, "contexted": self.contexted, "clipped": self.changes - self.contexted,
                "sites": len(self.keys), "sites_recurrent": sum(1 for c in self.keys.values() if c >= 2),
                "changes_at_recurrent": sum(c for c in self.keys.values() if c >= 2), "recur": recur, "n_top": len(top),
                "top_key": [k for _, k in top], "top_count": [c for c, _ in top],
                "top_sites": [(c,) + decode(k) for c, k in top]}

    def file_text(self, max_bin=10000, min_count=5, max_sites=1000):
        """the -recurrent file"""
        r = self.result(max_bin, min_count, max_sites)
        lines = ["flank\t%d" % FLANK, "min_count\t%d" % min_count, "changes\t%d" % r["changes"], "contexted\t%d" % r["contexted"],
                 "clipped\t%d" % r["clipped"], "sites\t%d" % r["sites"]]
        lines += ["recur\t%d\t%d" % (c, n) for c, n in enumerate(r["recur"]) if c and n]
        lines += ["site\t%d\t%s\t%s\t%s" % s for s in r["top_sites"]]
        return "\n".join(lines) + "\n"

    def stderr_line(self, min_count=5):
        at = [c for c in self.keys.values() if c >= min_count]
        return "Recurrent corrections: %d contexted changes at %d sites; %d changes at %d sites corrected at least %d times" % (
            self.contexted, len(self.keys), sum(at), len(at), min_count)


def assert_result(got, want):
    """a Context.recur_census() dict against Census.result(): exact"""
    for f in ("changes", "contexted", "clipped", "sites", "sites_recurrent", "changes_at_recurrent", "n_top"):
        assert got[f] == want[f], (f, got[f], want[f])
    assert [int(x) for x in got["recur"]] == want["recur"]
    assert [int(x) for x in got["top_key"]] == want["top_key"]
    assert [int(x) for x in got["top_count"]] == want["top_count"]
    assert [tuple(s) for s in got["top_sites"]] == want["top_sites"]
    assert sum(int(x) for x in got["recur"]) == got["sites"] and got["contexted"] + got["clipped"] == got["changes"]
