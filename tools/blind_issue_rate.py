"""Blind against plain issuance on one GPU (include/aeonflux_gpu.h "Blind issuance").

afx_issue_blind_dev alternating with afx_issue_dev in ONE process: the C5 layout (16 attributes, S x8 P x4 E x4) with 0, 1 and 4 of its
positions hidden from the issuer, 2^16 and 2^20 items, device-resident.  The requests come from afx_blind_request_dev (not timed).
Each call is timed 5 times after a warm-up with device events around the whole call on the context's stream (median and all runs
reported).  There is no target: the yardstick is afx_issue_dev on the same box and run; the expected extra is the request's
verification plus 1 + h more key terms (r'*D and y_i on A_i beside B_i) and one fixed-base term (r'*G).
    python tools/blind_issue_rate.py [--reps R] [--sizes 65536,1048576] [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aeonflux_amd as afx  # noqa: E402
import bench  # noqa: E402
from aeonflux_amd import batch  # noqa: E402

N, LAYOUT = 16, "SSSSSSSSPPPPEEEE"
# which positions the user hides: none; one scalar; two scalars and two points
HIDDEN = {0: [], 1: [0], 4: [0, 1, 8, 12]}


def synthetic_values(user, count):
    """attribute values of the layout: scalars and points made on the device from seeded bytes"""
    rng = np.random.default_rng(4242 + count)
    values = np.zeros((N, count, 32), np.uint8)
    for i, c in enumerate(LAYOUT):
        for o in range(0, count, 1 << 18):
            w = rng.integers(0, 256, size=(min(1 << 18, count - o), 64), dtype=np.uint8)
            values[i, o:o + w.shape[0]] = batch.scalars_from_wide(user, w) if c == "S" else batch.points_from_uniform(user, w)
    return values


def leg(say, torch, issuer, user, d_values, count, hidden, reps):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5150 + count + len(hidden))
    rb = lambda *shape: rng.integers(0, 256, size=shape, dtype=np.uint8)
    plain_kinds = [{"S": afx.ATTR_PUBLIC_SCALAR, "P": afx.ATTR_PUBLIC_POINT, "E": afx.ATTR_EITHER_POINT}[c] for c in LAYOUT]
    kinds = [(afx.ATTR_SECRET_SCALAR if LAYOUT[i] == "S" else afx.ATTR_SECRET_POINT) if i in hidden else k for i, k in enumerate(plain_kinds)]
    h, hs = batch.blind_layout(kinds)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)
    d_d = t(batch.scalars_from_wide(user, rb(count, 64)))
    d_rw, d_rseed = (t(rb(h, count, 64)) if h else None), t(rb(count, 32))
    d_tw, d_uw, d_rp, d_seed = t(rb(count, 64)), t(rb(count, 64)), t(rb(count, 64)), t(rb(count, 32))
    req = dict(D=z(count, 32), A=z(h, count, 32) if h else None, B=z(h, count, 32) if h else None, challenge=z(count, 32), responses=z(1 + h + hs, count, 32))
    st = {k: torch.full((count,), 255, dtype=torch.uint8, device=dev) for k in ("request", "plain", "blind", "unblind")}
    batch.blind_request_dev(user, kinds, d_values, d_d, d_rw, d_rseed, count, req, st["request"])
    user.synchronize()
    plain_out = {k: z(count, 32) for k in ("t", "U", "V", "challenge")}
    plain_out["responses"] = z(N + 5, count, 32)
    blind_out = {k: z(count, 32) for k in ("t", "U", "S1", "S2", "challenge")}
    blind_out["responses"] = z(N + 6, count, 32)
    a_plain = batch._blind_attrs(plain_kinds, d_values, batch._dptr)
    rnd = afx.IssueRandomness(d_tw.data_ptr(), d_uw.data_ptr(), d_seed.data_ptr())
    out = afx.IssuanceSoA(*(plain_out[k].data_ptr() for k in ("t", "U", "V", "challenge", "responses")))
    lib = afx.lib()

    def plain():
        afx.check(lib.afx_issue_dev(issuer.h, C.byref(a_plain), C.byref(rnd), count, C.byref(out), st["plain"].data_ptr()))

    def blind():
        batch.issue_blind_dev(issuer, kinds, d_values, req, 1 + h + hs, d_tw, d_uw, d_rp, d_seed, count, blind_out, st["blind"])
    paths = {"afx_issue_dev": plain, "afx_issue_blind_dev": blind}
    ext = torch.cuda.ExternalStream(issuer.stream)
    for f in paths.values():      # warm-up: workspaces, plan blobs
        f()
    issuer.synchronize()
    # same credential: the user's V of the blind answer is the plain call's V
    V = z(count, 32)
    batch.unblind_issuances_dev(user, kinds, d_values, d_d, req, blind_out, N + 6, count, V, st["unblind"])
    user.synchronize()
    ok = all(not bool(s.any()) for s in st.values()) and bool(torch.equal(V, plain_out["V"])) and bool(torch.equal(blind_out["U"], plain_out["U"]))
    times = {k: [] for k in paths}
    for _ in range(reps):
        for k, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext)
            f()
            e1.record(ext)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    stats = {}
    for k, f in paths.items():
        f()
        issuer.synchronize()
        stats[k] = issuer.plan_stats()
    med = {k: statistics.median(v) for k, v in times.items()}
    say("C5 layout, %d hidden position%s, %d items device-resident; statuses 0 and the unblinded V equal to afx_issue_dev's: %s" % (len(hidden), "" if len(hidden) == 1 else "s", count, ok))
    for k in paths:
        say("  %-20s median %8.2f ms  %6.3f M issuances/s  (runs: %s)" % (k, med[k], count / med[k] / 1e3, " ".join("%.2f" % x for x in times[k])))
    say("  blind against plain: %.2fx the time; spread of the repeats: %.2f ms" % (med["afx_issue_blind_dev"] / med["afx_issue_dev"], max(max(v) - min(v) for v in times.values())))
    for k in paths:
        say("  operation counts per item (%s): %s" % (k, " ".join("%s=%d" % kv for kv in stats[k].items())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("blind against plain issuance (afx_issue_blind_dev, afx_issue_dev), one MI355X, one process, calls alternating, secret-independent addressing 2")
    params, key, ip = bench.load_fixture("c5_16attrs")
    issuer, user = afx.Context(params, key, ip), afx.Context(params, None, ip)
    user.set_secret_independent_addressing(0)      # input generation and the (untimed) requests: synthetic values are no secrets
    for count in (int(x) for x in args.sizes.split(",")):
        d_values = torch.from_numpy(synthetic_values(user, count)).to(torch.device("cuda", 0))
        for nh in sorted(HIDDEN):
            leg(say, torch, issuer, user, d_values, count, HIDDEN[nh], args.reps)
    issuer.close()
    user.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
