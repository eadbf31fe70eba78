"""Host share of a small call, on a CPU: the engine's host half of a tree built plain against the fake HIP runtime (tests/hostsim, the
source list of tests/test_launch_kinds_host.py), where a call is almost purely assemble / reuse, relocate and run_plans.
    python tools/host_call_overhead.py [--tree DIR] [--rounds 5] [--calls 2000]
times `--calls` verify_presentations calls of 1 item and of 16 items on the C3 fixture, end to end, and as many calls of their serialized
twin - afx_verify_presentations_wire on the same presentations packed as one AFXP batch - in a fresh process per round; with --tree (a
checkout of another commit: tools/ab_trees.sh says how to make one) the two trees alternate.  Prints us per call and, at the end, every
tree's median and its spread (max - min) over the rounds."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ("engine", "plans", "statements", "statements_prove", "statements_setup", "statements_blind", "statements_messages", "group", "mixed", "wire")
FAKES = ("fake_hip.cpp", "fake_plaintext.cpp", "fake_blind.cpp", "fake_batchable.cpp", "fake_draw.cpp", "fake_messages.cpp")

ROUND = r"""
import sys, time
sys.path.insert(0, %(tree)r)
import numpy as np
import aeonflux_amd as afx
afx.LIB_PATH = %(lib)r
import bench
from aeonflux_amd import batch, wire
p3, k3, i3 = bench.load_fixture("c3_8attrs_SSPPeeee")
ctx = afx.Context(p3, k3, i3)
kinds = [afx.ATTR_PUBLIC_SCALAR] * 2 + [afx.ATTR_PUBLIC_POINT] * 2 + [afx.ATTR_SECRET_POINT] * 4
shape = batch.shape_of_kinds(kinds)
out, out_wire = [], []
for n in (1, 16):
    z = lambda *s: np.zeros(s, np.uint8)
    pres = {"challenge": z(n, 32), "responses": z(shape.n_responses, n, 32), "C_x_0": z(n, 32), "C_x_1": z(n, 32), "C_V": z(n, 32), "C_y": z(8, n, 32),
            "attr_values": z(8, n, 32), "enc": [{f: (z(6, n, 32) if f == "responses" else z(n, 32)) for f in batch.ENC_FIELDS} for _ in range(4)]}
    for _ in range(50):
        batch.verify_presentations(ctx, shape, pres)
    t0 = time.perf_counter()
    for _ in range(%(calls)d):
        batch.verify_presentations(ctx, shape, pres)
    out.append((time.perf_counter() - t0) / %(calls)d * 1e6)
    blob = wire.pack_presentations(shape, pres)
    for _ in range(50):
        wire.verify_wire(ctx, blob)
    t0 = time.perf_counter()
    for _ in range(%(calls)d):
        wire.verify_wire(ctx, blob)
    out_wire.append((time.perf_counter() - t0) / %(calls)d * 1e6)
print("%%.2f %%.2f %%.2f %%.2f" %% tuple(out + out_wire))
"""


def build(tree, out):
    srcs = [os.path.join(tree, "aeonflux_amd", "csrc", f + ".cpp") for f in HOST]
    srcs += [p for p in (os.path.join(tree, "tests", "hostsim", f) for f in FAKES) if os.path.exists(p)]
    subprocess.run(["g++", "-O1", "-fPIC", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-shared", "-pthread", "-o", out] + srcs, check=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    a = ap.parse_args()
    trees = [("HEAD", ROOT)] + ([("other", os.path.abspath(a.tree))] if a.tree else [])
    with tempfile.TemporaryDirectory() as tmp:
        libs = {}
        for name, tree in trees:
            libs[name] = os.path.join(tmp, "libafx_hostsim_%s.so" % name)
            build(tree, libs[name])
        cols = ("1 item us", "16 items us", "wire 1 us", "wire 16 us")
        print("%-6s %-6s" % ("round", "tree") + " %12s" * 4 % cols)
        seen = {name: [] for name, _ in trees}
        for r in range(a.rounds):
            for name, tree in trees:
                got = subprocess.run([sys.executable, "-c", ROUND % {"tree": tree, "lib": libs[name], "calls": a.calls}], capture_output=True, text=True, cwd=tree, check=True)
                seen[name].append([float(x) for x in got.stdout.split()[-4:]])
                print("%-6d %-6s" % (r + 1, name) + " %12.2f" * 4 % tuple(seen[name][-1]), flush=True)
        for name, _ in trees:
            by_col = list(zip(*seen[name]))
            print("%-6s %-6s" % ("median", name) + " %12.2f" * 4 % tuple(statistics.median(c) for c in by_col))
            print("%-6s %-6s" % ("spread", name) + " %12.2f" * 4 % tuple(max(c) - min(c) for c in by_col))


if __name__ == "__main__":
    main()
