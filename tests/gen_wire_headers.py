"""Records what the wire formats' header functions answer to every case of tests/wire_header_cases.py, with the library of the tree this
file stands in (aeonflux_amd.lib(): it loads on a host without a GPU), into tests/golden/wire_headers.json.

    python tests/gen_wire_headers.py COMMIT [output path]

COMMIT names the commit whose built library is recording - the fixture pins the header functions' behaviour AT that commit, so it is
recorded once, in a checkout of it, and never again from the code a later change puts under test (tests/test_wire_headers.py replays
it).  The fixture holds outcomes, not blobs: a table of the distinct outcomes (error texts as indices into a string table), per case
the index of its outcome as run lengths, the layout sweep, and the digest of the cases it was recorded for."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import wire_header_cases as whc   # noqa: E402


class Table:
    """distinct values in order of first appearance"""
    def __init__(self, values=()):
        self.values, self.index = [], {}
        for v in values:
            self.add(v)

    def add(self, v):
        key = json.dumps(v)
        if key not in self.index:
            self.index[key] = len(self.values)
            self.values.append(v)
        return self.index[key]


def run_lengths(seq):
    out = []
    for v in seq:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return out


def record(lib, strings, outcomes):
    """the cases' outcome indices, in order; fills the two tables"""
    idx = []
    for f, _, blob in whc.cases():
        pair = []
        for o in whc.outcome(lib, f, blob):
            if o[1] is not None:
                o[1] = strings.add(o[1])
            pair.append(o)
        idx.append(outcomes.add(pair))
    return idx


def main():
    import aeonflux_amd as afx
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "wire_headers.json")
    strings, outcomes = Table(), Table()
    idx = record(afx.lib(), strings, outcomes)
    doc = {"recorded_at": commit, "cases": len(idx), "cases_sha256": whc.digest(), "strings": strings.values, "outcomes": outcomes.values,
           "case_outcomes": run_lengths(idx), "sweep": whc.sweep(afx.lib())}
    with open(out, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    print("%d cases, %d distinct outcomes, %d error texts -> %s (%d bytes)" % (len(idx), len(outcomes.values), len(strings.values), out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
