"""Randomness drawn on the device (afx_issue_wire_rng, afx_show_wire_rng) against the wire calls that take it from the host, on one GPU.

Issue: C5 (c5_16attrs: S x8 P x4 E x4), 2^20 requests in host memory, secret modes 2 and 0.  Show: bench.py's show shape
(readme_4attrs_sSPe, s S P e: one hidden point), 2^20 credentials, modes 2 and 0.  Three paths in the same process, alternated, each
timed 5 times (median reported):
  (a) os.urandom draws + the explicit call (the draw time is reported on its own line);
  (b) the explicit call with the draws made beforehand;
  (c) the rng call: 40 bytes of seed and stream in, every draw made by k_draw.
    python tools/device_rng_rate.py [--count N] [--reps R] [--out FILE]"""
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


def timed(paths, reps):
    for f in paths.values():   # warm-up: plans, staging buffers, pinned images
        f()
    times = {k: [] for k in paths}
    for _ in range(reps):
        for k, f in paths.items():
            t0 = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t0)
    return times


def report(say, times, draw_s, count, what):
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, label in (("a", "(a) os.urandom + explicit call"), ("b", "(b) explicit call, draws ready"), ("c", "(c) rng call, drawn on the GPU ")):
        say("  %s median %8.1f ms  %6.3f M %s/s  (runs: %s)" % (label, 1e3 * med[k], count / med[k] / 1e6, what, " ".join("%.1f" % (1e3 * t) for t in times[k])))
    say("      of which os.urandom alone: median %.1f ms (%.2f GB/s)" % (1e3 * statistics.median(draw_s), statistics.median([b / t / 1e9 for b, t in draw_s.bytes_per])))
    say("  (c) against (b): %+.1f %% time; against (a): %+.1f %% time" % (100 * (med["c"] / med["b"] - 1), 100 * (med["c"] / med["a"] - 1)))


class DrawTimes(list):
    def __init__(self):
        super().__init__()
        self.bytes_per = []

    def note(self, nbytes, seconds):
        self.append(seconds)
        self.bytes_per.append((nbytes, seconds))


def issue_leg(say, count, reps):
    layout = "S" * 8 + "P" * 4 + "E" * 4
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
    lib = afx.lib()
    request = wire.pack_requests(kinds, values)
    olen, ocnt = C.c_size_t(0), C.c_size_t(0)
    afx.check(lib.afx_issue_wire(ctx.h, request, len(request), None, None, 0, C.byref(olen), None, 0, C.byref(ocnt)))
    blob, st = np.ones(olen.value, np.uint8), np.zeros(count, np.uint8)
    ready = np.frombuffer(os.urandom(160 * count), np.uint8)
    rnd_ready = afx.IssueRandomness(ready.ctypes.data, ready.ctypes.data + 64 * count, ready.ctypes.data + 128 * count)
    draw_s = DrawTimes()
    seed = afx.DeviceRng(None, 0)

    def path_a():
        t0 = time.perf_counter()
        r = np.frombuffer(os.urandom(160 * count), np.uint8)
        draw_s.note(160 * count, time.perf_counter() - t0)
        rnd = afx.IssueRandomness(r.ctypes.data, r.ctypes.data + 64 * count, r.ctypes.data + 128 * count)
        afx.check(lib.afx_issue_wire(ctx.h, request, len(request), C.byref(rnd), blob.ctypes.data, blob.size, C.byref(olen), st.ctypes.data, count, C.byref(ocnt)))

    def path_b():
        afx.check(lib.afx_issue_wire(ctx.h, request, len(request), C.byref(rnd_ready), blob.ctypes.data, blob.size, C.byref(olen), st.ctypes.data, count,
                                     C.byref(ocnt)))

    def path_c():
        afx.check(lib.afx_issue_wire_rng(ctx.h, request, len(request), C.byref(seed), blob.ctypes.data, blob.size, C.byref(olen), st.ctypes.data, count,
                                         C.byref(ocnt)))
    say("issue: C5 (c5_16attrs, S x8 P x4 E x4), %d requests in host memory; (a)/(b) send 160 B of draws per request, (c) 40 B per call" % count)
    for mode in (2, 0):
        ctx.set_secret_independent_addressing(mode)
        del draw_s[:]
        draw_s.bytes_per.clear()
        times = timed({"a": path_a, "b": path_b, "c": path_c}, reps)
        say("mode %d (%s):" % (mode, "secret-independent prover-side addressing" if mode == 2 else "fastest tables"))
        report(say, times, draw_s, count, "issuances")
        say("  every status OK after (c): %s" % (not st.any()))
    ctx.close()


def show_leg(say, count, reps):
    params, key, ip = bench.load_fixture("readme_4attrs_sSPe")
    issuer = afx.Context(params, key, ip)
    user = afx.Context(params, None, ip)
    n, layout, hide = 4, "SSPE", [0, 3]
    rng = np.random.default_rng(20261016 + count)
    rb = lambda *s: rng.integers(0, 256, size=s, dtype=np.uint8)
    issuer.set_secret_independent_addressing(0)
    values, M2, m3 = (np.zeros((n, count, 32), np.uint8) for _ in range(3))
    kinds = []
    for i, c in enumerate(layout):
        for o in range(0, count, 1 << 18):
            k = min(1 << 18, count - o)
            if c == "S":
                values[i, o:o + k] = batch.scalars_from_wide(issuer, rb(k, 64))
            else:
                values[i, o:o + k] = batch.points_from_uniform(issuer, rb(k, 64))
                if c == "E":
                    M2[i, o:o + k] = batch.points_from_uniform(issuer, rb(k, 64))
                    m3[i, o:o + k] = batch.scalars_from_wide(issuer, rb(k, 64))
        kinds.append({"S": afx.ATTR_PUBLIC_SCALAR, "P": afx.ATTR_PUBLIC_POINT, "E": afx.ATTR_EITHER_POINT}[c])
    iss, st = batch.issue(issuer, kinds, values, rb(count, 64), rb(count, 64), rb(count, 32))
    assert not st.any()
    skinds = list(kinds)
    for i in hide:
        skinds[i] = afx.ATTR_SECRET_SCALAR if skinds[i] == afx.ATTR_PUBLIC_SCALAR else afx.ATTR_SECRET_POINT
    ms = rb(count, 64)
    kp = [np.zeros((count, 32), np.uint8) for _ in range(4)]
    afx.check(afx.lib().afx_keypairs_derive(issuer.h, ms.ctypes.data, count, *(x.ctypes.data for x in kp)))
    issuer.close()
    lib = afx.lib()
    ready = np.frombuffer(os.urandom(128 * count), np.uint8)
    cs, kpp, rnd, _, _, cnt, keep = batch._show_args(skinds, values, iss["t"], iss["U"], iss["V"], dict(zip(("a", "a0", "a1", "pk"), kp)),
                                                     ready[:64 * count].reshape(count, 64), ready[64 * count:96 * count].reshape(count, 32),
                                                     ready[96 * count:].reshape(1, count, 32), M2, m3, outputs=False)
    grp = (afx.ShowGroup * 1)()
    grp[0].creds, grp[0].rnd, grp[0].count, grp[0].keypairs = cs, rnd, count, C.pointer(kpp)
    olen = C.c_size_t(0)
    afx.check(lib.afx_show_wire(user.h, grp, 1, None, 0, C.byref(olen), None, 0))
    blob, st_c = np.ones(olen.value, np.uint8), np.zeros(count, np.uint8)
    draw_s = DrawTimes()
    seed = afx.DeviceRng(None, 0)

    def path_a():
        t0 = time.perf_counter()
        r = np.frombuffer(os.urandom(128 * count), np.uint8)
        draw_s.note(128 * count, time.perf_counter() - t0)
        g = (afx.ShowGroup * 1)()
        g[0] = grp[0]
        g[0].rnd = afx.ShowRandomness(r.ctypes.data, r.ctypes.data + 64 * count, r.ctypes.data + 96 * count)
        afx.check(lib.afx_show_wire(user.h, g, 1, blob.ctypes.data, blob.size, C.byref(olen), st_c.ctypes.data, count))

    def path_b():
        afx.check(lib.afx_show_wire(user.h, grp, 1, blob.ctypes.data, blob.size, C.byref(olen), st_c.ctypes.data, count))

    def path_c():
        afx.check(lib.afx_show_wire_rng(user.h, grp, 1, C.byref(seed), blob.ctypes.data, blob.size, C.byref(olen), st_c.ctypes.data, count))
    say("show: bench.py's show shape (readme_4attrs_sSPe, s S P e, one hidden point), %d credentials in host memory; (a)/(b) send 128 B of "
        "draws per credential, (c) 40 B per call" % count)
    for mode in (2, 0):
        user.set_secret_independent_addressing(mode)
        del draw_s[:]
        draw_s.bytes_per.clear()
        times = timed({"a": path_a, "b": path_b, "c": path_c}, reps)
        say("mode %d (%s):" % (mode, "secret-independent prover-side addressing" if mode == 2 else "fastest tables"))
        report(say, times, draw_s, count, "presentations")
        say("  every status OK after (c): %s" % (not st_c.any()))
    user.close()
    del keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("randomness drawn on the device against draws from the host, one MI355X")
    issue_leg(say, args.count, args.reps)
    show_leg(say, args.count, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
