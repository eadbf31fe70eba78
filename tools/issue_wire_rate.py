"""Issuer::issue from request bytes to response bytes (afx_issue_wire) against the column path it replaces, on one GPU.

C5 layout (flow c5_16attrs of tests/golden/flows.json: 16 attributes S x8 P x4 E x4), 2^20 requests in host memory, secret modes 2
and 0.  Three paths in the same process, alternated, each timed 5 times (median reported):
  (a) afx_issue: host columns in, host columns out;
  (b) (a) followed by afx_issuance_wire_pack: the AFXI batch a server has to send back today;
  (c) afx_issue_wire: one AFXR section in, the AFXI batch out.
Also the core clock of a separate (c) run (afx_ctx_get_core_clock_mhz) and whether (b) and (c) wrote the same bytes.
    python tools/issue_wire_rate.py [--count N] [--reps R] [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aeonflux_amd as afx  # noqa: E402
import bench  # noqa: E402
from aeonflux_amd import batch, wire  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    count, layout = args.count, "S" * 8 + "P" * 4 + "E" * 4
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    params, key, ip = bench.load_fixture("c5_16attrs")
    ctx = afx.Context(params, key, ip)
    ctx.set_secret_independent_addressing(0)   # input generation only
    rng = np.random.default_rng(20261016)
    rb = lambda *s: rng.integers(0, 256, size=s, dtype=np.uint8)
    kinds = [{"S": afx.ATTR_PUBLIC_SCALAR, "P": afx.ATTR_PUBLIC_POINT, "E": afx.ATTR_EITHER_POINT}[c] for c in layout]
    values = np.zeros((16, count, 32), np.uint8)
    for i, c in enumerate(layout):
        for o in range(0, count, 1 << 18):
            w = rb(min(1 << 18, count - o), 64)
            values[i, o:o + w.shape[0]] = batch.scalars_from_wide(ctx, w) if c == "S" else batch.points_from_uniform(ctx, w)
    tw, uw, sd = rb(count, 64), rb(count, 64), rb(count, 32)
    lib = afx.lib()
    # (a): column arrays, allocated and touched once
    req, rnd, out, o, cnt, keep = batch._issue_args(ctx.n, kinds, values, tw, uw, sd)
    for v in o.values():
        v.fill(1)
    st_a = np.zeros(count, np.uint8)
    nr = ctx.n + 5
    blen = C.c_size_t(0)
    afx.check(lib.afx_issuance_wire_pack(C.byref(req), C.byref(out), nr, count, None, 0, C.byref(blen)))
    blob_b = np.ones(blen.value, np.uint8)
    # (c): one AFXR section, the AFXI buffer and statuses allocated and touched once
    request = wire.pack_requests(kinds, values)
    olen, ocnt = C.c_size_t(0), C.c_size_t(0)
    afx.check(lib.afx_issue_wire(ctx.h, request, len(request), None, None, 0, C.byref(olen), None, 0, C.byref(ocnt)))
    blob_c = np.ones(olen.value, np.uint8)
    st_c = np.zeros(count, np.uint8)

    def path_a():
        afx.check(lib.afx_issue(ctx.h, C.byref(req), C.byref(rnd), count, C.byref(out), st_a.ctypes.data))

    def path_b():
        path_a()
        afx.check(lib.afx_issuance_wire_pack(C.byref(req), C.byref(out), nr, count, blob_b.ctypes.data, blob_b.size, C.byref(blen)))

    def path_c():
        afx.check(lib.afx_issue_wire(ctx.h, request, len(request), C.byref(rnd), blob_c.ctypes.data, blob_c.size, C.byref(olen),
                                     st_c.ctypes.data, count, C.byref(ocnt)))
    say("afx_issue_wire against the column path: C5 (c5_16attrs, S x8 P x4 E x4), %d requests in host memory, one MI355X" % count)
    say("per item: (a) 512 B values + 160 B randomness in, 800 B out; (c) 512 B records + 160 B randomness in, %d B AFXI record out"
        % ((4 + nr + 16) * 32))
    for mode in (2, 0):
        ctx.set_secret_independent_addressing(mode)
        for f in (path_a, path_b, path_c):   # warm-up: plans, staging buffers, pinned images
            f()
        times = {"a": [], "b": [], "c": []}
        for _ in range(args.reps):
            for name, f in (("a", path_a), ("b", path_b), ("c", path_c)):
                t0 = time.perf_counter()
                f()
                times[name].append(time.perf_counter() - t0)
        same = bytes(blob_b) == bytes(blob_c) and np.array_equal(st_a, st_c) and not st_c.any()
        ctx.set_timing(True)
        path_c()
        mhz = ctx.core_clock_mhz()
        ctx.set_timing(False)
        med = {k: statistics.median(v) for k, v in times.items()}
        say("mode %d (%s):" % (mode, "secret-independent prover-side addressing" if mode == 2 else "fastest tables"))
        for k, label in (("a", "(a) afx_issue, columns in/out            "), ("b", "(b) afx_issue + afx_issuance_wire_pack   "),
                         ("c", "(c) afx_issue_wire, bytes in/out         ")):
            say("  %s median %8.1f ms  %6.3f M issuances/s  (runs: %s)" % (label, 1e3 * med[k], count / med[k] / 1e6,
                                                                               " ".join("%.1f" % (1e3 * t) for t in times[k])))
        say("  (c) against (a): %+.1f %% time; against (b): %+.1f %% time" % (100 * (med["c"] / med["a"] - 1), 100 * (med["c"] / med["b"] - 1)))
        say("  core clock during a (c) run: %.0f MHz;  (b) and (c) byte-equal (AFXI bytes and statuses, all OK): %s" % (mhz, same))
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
