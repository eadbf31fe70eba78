"""The blind issuer from request bytes to issuance bytes (afx_issue_blind_wire, afx_issue_blind_wire_rng) against the column path and
what a server does around it today, on one GPU.

C5 layout (16 attributes, S x8 P x4 E x4) with 0, 1 and 4 of its positions hidden from the issuer, 2^16 and 2^20 requests in host
memory, secret-independent addressing 2.  The requests come from afx_blind_request (not timed).  Five paths in the same process,
alternated, each timed 5 times after a warm-up (median and all runs reported):
  (a) afx_issue_blind: host columns in, host columns out;
  (b) numpy unpacking of the AFXQ section into those columns, (a), and pack_blind_issuances: what a server does today (the unpacked
      columns and the packed bytes are made anew every time, as unpacking and packing make them; the call's output columns are
      allocated and touched once, outside the timing, like the output buffers of (a) and (c));
  (c) afx_issue_blind_wire: one AFXQ section in, the AFXJ section out;
  (d) afx_issue_blind_wire_rng: (c) with the four draws per request made on the device;
  (e) os.urandom draws of the 224 bytes per request, then (c).
(b) and (c) must write the same bytes.  The first shape is run once in full before anything is reported and that leg is thrown away
(printed as such): whatever only the process's first leg pays - first touches, clocks - is not charged to a shape.  With --tree DIR, (a) alone is timed on another checkout's library (the parent commit's, built
there) in a child process on the same box: the column path did not move.
    python tools/blind_wire_rate.py [--sizes 65536,1048576] [--reps R] [--tree DIR] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LAYOUT = 16, "SSSSSSSSPPPPEEEE"
HIDDEN = {0: [], 1: [0], 4: [0, 1, 8, 12]}          # as tools/blind_issue_rate.py: none; one scalar; two scalars and two points


def kinds_of(afx, hidden):
    plain = [{"S": afx.ATTR_PUBLIC_SCALAR, "P": afx.ATTR_PUBLIC_POINT, "E": afx.ATTR_EITHER_POINT}[c] for c in LAYOUT]
    return [(afx.ATTR_SECRET_SCALAR if LAYOUT[i] == "S" else afx.ATTR_SECRET_POINT) if i in hidden else k for i, k in enumerate(plain)]


def synthetic_values(batch, user, count):
    rng = np.random.default_rng(4242 + count)
    values = np.zeros((N, count, 32), np.uint8)
    for i, c in enumerate(LAYOUT):
        for o in range(0, count, 1 << 18):
            w = rng.integers(0, 256, size=(min(1 << 18, count - o), 64), dtype=np.uint8)
            values[i, o:o + w.shape[0]] = batch.scalars_from_wide(user, w) if c == "S" else batch.points_from_uniform(user, w)
    return values


def make_requests(afx, batch, user, values, count, hidden):
    rng = np.random.default_rng(5150 + count + len(hidden))
    rb = lambda *shape: rng.integers(0, 256, size=shape, dtype=np.uint8)
    kinds = kinds_of(afx, hidden)
    h, _ = batch.blind_layout(kinds)
    req, st = batch.blind_request(user, kinds, values, batch.scalars_from_wide(user, rb(count, 64)), rb(h, count, 64), rb(count, 32))
    assert not st.any()
    return kinds, req, [rb(count, 64), rb(count, 64), rb(count, 64), rb(count, 32)]


def output_columns(batch, count):
    """the output arrays of afx_issue_blind, allocated and touched -> (issuance dict, statuses)"""
    o = {f: np.ones((count, 32), np.uint8) for f in batch.BLIND_ISSUANCE_FIELDS[:5]}
    o["responses"] = np.ones((N + 6, count, 32), np.uint8)
    return o, np.zeros(count, np.uint8)


def column_call(afx, batch, issuer, kinds, values, req, wides, count, outputs=None):
    """afx_issue_blind with every array allocated and touched once (outputs: arrays to write into) -> (call, issuance dict, statuses)"""
    h, hs = batch.blind_layout(kinds)
    o, st = outputs or output_columns(batch, count)
    a = batch._blind_attrs(kinds, values, batch._hptr)
    soa = afx.BlindRequestSoA(*(batch._hptr(req[f]) for f in batch.REQUEST_FIELDS))
    rnd = afx.BlindIssueRandomness(*(w.ctypes.data for w in wides))
    out = afx.BlindIssuanceSoA(*(o[f].ctypes.data for f in batch.BLIND_ISSUANCE_FIELDS))
    lib = afx.lib()

    def call():
        afx.check(lib.afx_issue_blind(issuer.h, C.byref(a), C.byref(soa), 1 + h + hs, C.byref(rnd), count, C.byref(out), st.ctypes.data))
    call.keep = (a, soa, rnd, out)
    return call, o, st


def device_name(afx):
    """what HIP calls device 0 (asked through the library's handle: the runtime is among its dependencies)"""
    try:
        name = C.create_string_buffer(256)
        if afx.lib().hipDeviceGetName(name, 256, 0) == 0 and name.value:
            return name.value.decode(errors="replace")
    except (AttributeError, OSError):
        pass
    return "device 0"


def child(args):
    """(a) alone, in a process of its own, on the package and library of the checkout at args.root"""
    sys.path.insert(0, args.root)
    import aeonflux_amd as afx
    import bench
    from aeonflux_amd import batch
    params, key, ip = bench.load_fixture("c5_16attrs")
    issuer, user = afx.Context(params, key, ip), afx.Context(params, None, ip)
    user.set_secret_independent_addressing(0)
    res = {}
    sizes = [int(x) for x in args.sizes.split(",")]
    legs = [(c, nh) for c in sizes for nh in sorted(HIDDEN)]
    values = {}
    for k, (count, nh) in enumerate(legs[:1] + legs):          # (the first leg twice, its first run thrown away, as in the parent process)
        if count not in values:
            values = {count: synthetic_values(batch, user, count)}
        kinds, req, wides = make_requests(afx, batch, user, values[count], count, HIDDEN[nh])
        call, o, st = column_call(afx, batch, issuer, kinds, values[count], req, wides, count)
        call()
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
        assert not st.any()
        if k:
            res["%d/%d" % (count, nh)] = times
    print("CHILD " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")          # (internal: what --tree starts)
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    if args.child:
        return child(args)
    sys.path.insert(0, ROOT)
    import aeonflux_amd as afx
    import bench
    from aeonflux_amd import batch, wire
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    params, key, ip = bench.load_fixture("c5_16attrs")
    issuer, user = afx.Context(params, key, ip), afx.Context(params, None, ip)
    say("afx_issue_blind_wire and afx_issue_blind_wire_rng against the column path: C5 (c5_16attrs, S x8 P x4 E x4), requests in host memory,")
    say("one GPU (%s), one process, calls alternating, secret-independent addressing 2; medians of %d" % (device_name(afx), args.reps))
    user.set_secret_independent_addressing(0)      # input generation and the (untimed) requests: synthetic values are no secrets
    lib = afx.lib()
    other = None
    if args.tree:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", os.path.abspath(args.tree), "--sizes", args.sizes, "--reps", str(args.reps)],
                           capture_output=True, text=True, cwd=os.path.abspath(args.tree))
        tail = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
        if r.returncode == 0 and tail:
            other = json.loads(tail[-1][6:])
        else:
            say("(--tree %s: the other checkout's run failed: %s)" % (os.path.basename(os.path.normpath(args.tree)), (r.stderr or r.stdout)[-300:].replace("\n", " | ")))
    sizes = [int(x) for x in args.sizes.split(",")]
    legs = [(c, nh) for c in sizes for nh in sorted(HIDDEN)]
    values = {}
    for leg, (count, nh) in enumerate(legs[:1] + legs):
        report = say if leg else (lambda s: say("  [first leg of the process, thrown away] " + s.strip()))
        if count not in values:
            values = {count: synthetic_values(batch, user, count)}
        kinds, req, wides = make_requests(afx, batch, user, values[count], count, HIDDEN[nh])
        h, hs = batch.blind_layout(kinds)
        blob = wire.pack_blind_requests(kinds, values[count], req)
        call_a, o, st_a = column_call(afx, batch, issuer, kinds, values[count], req, wides, count)
        rnd = afx.BlindIssueRandomness(*(w.ctypes.data for w in wides))
        olen, ocnt = C.c_size_t(0), C.c_size_t(0)
        afx.check(lib.afx_issue_blind_wire(issuer.h, blob, len(blob), None, None, 0, C.byref(olen), None, 0, C.byref(ocnt)))
        out_c, out_d, st_c = np.ones(olen.value, np.uint8), np.ones(olen.value, np.uint8), np.zeros(count, np.uint8)
        rng = afx.DeviceRng(None, 0)
        kept = {}
        outputs_b = output_columns(batch, count)

        def path_b():
            k2, v2, q2 = wire.unpack_blind_requests(blob)
            call, o2, st2 = column_call(afx, batch, issuer, k2, v2, q2, wides, count, outputs_b)
            call()
            kept["b"] = wire.pack_blind_issuances(k2, o2)

        def path_c(r=rnd):
            afx.check(lib.afx_issue_blind_wire(issuer.h, blob, len(blob), C.byref(r), out_c.ctypes.data, out_c.size, C.byref(olen), st_c.ctypes.data, count, C.byref(ocnt)))

        def path_d():
            rng.stream += 1
            afx.check(lib.afx_issue_blind_wire_rng(issuer.h, blob, len(blob), C.byref(rng), out_d.ctypes.data, out_d.size, C.byref(olen), st_c.ctypes.data, count,
                                                   C.byref(ocnt)))

        def path_e():
            fresh = [np.frombuffer(os.urandom(count * w), np.uint8) for w in (64, 64, 64, 32)]
            path_c(afx.BlindIssueRandomness(*(f.ctypes.data for f in fresh)))
        paths = (("a", call_a), ("b", path_b), ("c", path_c), ("d", path_d), ("e", path_e))
        for _, f in paths[:4]:          # warm-up: plans, staging buffers, pinned images
            f()
        same = kept["b"] == bytes(out_c) and not st_a.any() and not st_c.any()
        times = {k: [] for k, _ in paths}
        for _ in range(args.reps):
            for k, f in paths:
                t0 = time.perf_counter()
                f()
                times[k].append(time.perf_counter() - t0)
        ok_d = not st_c.any()
        med = {k: statistics.median(v) for k, v in times.items()}
        report("%d hidden position%s, %d requests (AFXQ record %d B + 224 B randomness in, AFXJ record %d B out); (b) and (c) byte-equal, statuses 0: %s; (d), (e) statuses 0: %s"
               % (nh, "" if nh == 1 else "s", count, (3 + 2 * h + hs + N) * 32, (N + 11) * 32, same, ok_d))
        for k, label in (("a", "(a) afx_issue_blind, columns in/out          "), ("b", "(b) numpy unpack + (a) + pack_blind_issuances"),
                         ("c", "(c) afx_issue_blind_wire, bytes in/out       "), ("d", "(d) afx_issue_blind_wire_rng                 "),
                         ("e", "(e) os.urandom draws + (c)                   ")):
            report("  %s median %8.1f ms  %6.3f M issuances/s  (runs: %s)" % (label, 1e3 * med[k], count / med[k] / 1e6, " ".join("%.1f" % (1e3 * t) for t in times[k])))
        report("  (c) against (a): %+.1f %% time; (c) against (b): %+.1f %%; (d) against (e): %+.1f %%; (d) against (c): %+.1f %%"
               % (100 * (med["c"] / med["a"] - 1), 100 * (med["c"] / med["b"] - 1), 100 * (med["d"] / med["e"] - 1), 100 * (med["d"] / med["c"] - 1)))
        if other and leg:
            t = other.get("%d/%d" % (count, nh))
            if t:
                m = statistics.median(t)
                report("  (a) on the other checkout (%s): median %8.1f ms (runs: %s); this tree's (a) against it: %+.1f %%"
                       % (os.path.basename(os.path.normpath(args.tree)), 1e3 * m, " ".join("%.1f" % (1e3 * x) for x in t), 100 * (med["a"] / m - 1)))
    issuer.close()
    user.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
