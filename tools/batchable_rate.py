"""Batchable against compact presentation proofs on one GPU (include/aeonflux_gpu.h "Batchable presentation proofs").

Issuer::verify of the same presentations in both encodings, device-resident, in ONE process: C2 (readme_4attrs_sSPe, 2^16), C3
(c3 shape S S P P e e e e, 2^20) and the C4-per-rank size (the C3 statement, 2^19).  The two calls alternate; each is timed 5 times
after a warm-up with device events around the whole call on the context's stream (median and all runs reported), with the core
clock the chains of a separate run of each form held - the path is power-bound, so a rate means little without it.  Then the
per-kernel times of one C3 call of each form (afx_ctx_set_timing) and the plan's operation counts (afx_ctx_get_plan_stats).
The baseline is the compact path of the same box and run.  Last, the two AFXB doors against their column forms at the C2 size,
host memory in and out, wall clock (medians of 5 after a warm-up).
    python tools/batchable_rate.py [--reps R] [--out FILE] [--sizes C2,C3,C4]"""
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

KERNELS = ("k_decode", "k_sccheck", "k_scalarop", "k_pointop", "k_negenc", "k_msm", "k_compress2x", "k_pointsum", "k_hash", "k_coef", "k_finish")
# bench.py's workloads; C4 at the size one of eight ranks holds
SIZES = {"C2": bench.WORKLOADS["c2"][:5], "C3": bench.WORKLOADS["c3"][:5], "C4": bench.WORKLOADS["c3"][:3] + (1 << 19, bench.WORKLOADS["c3"][4])}


def generate_both(issuer, user, params, n, layout, hide, count, seed):
    """bench.generate with the show in batchable form: (presentation columns, commitments, shape)"""
    stash, orig = {}, batch.show

    def show2(ctx, *a, **k):
        assert "cm" not in stash, "bench.generate is expected to show once"
        pres, cm, shape, st = batch.show_batchable(ctx, *a, **k)
        stash["cm"] = cm
        return pres, shape, st
    batch.show = show2
    try:
        pres, shape = bench.generate(afx, batch, issuer, user, params, n, layout, hide, count, seed, fast_tables=True)
    finally:
        batch.show = orig
    return pres, stash["cm"], shape


def leg(say, torch, name, reps):
    n, layout, hide, count, fixture = SIZES[name]
    params, key, ip = bench.load_fixture(fixture)
    issuer, user = afx.Context(params, key, ip), afx.Context(params, None, ip)
    pres, cm, shape = generate_both(issuer, user, params, n, layout, hide, count, 777)
    user.close()
    want = bench.corrupt(pres, count, 11)                     # 1 % of the items: both forms must reject exactly these
    issuer.set_secret_independent_addressing(2)
    dev = torch.device("cuda", 0)
    dpres = {f: torch.from_numpy(pres[f]).to(dev) for f in batch.PRES_FIELDS}
    dpres["enc"] = [{f: torch.from_numpy(d[f]).to(dev) for f in batch.ENC_FIELDS} for d in pres["enc"]]
    dcm = {"main": torch.from_numpy(cm["main"]).to(dev), "enc": [torch.from_numpy(a).to(dev) for a in cm["enc"]]}
    soa, keep = batch.presentation_soa(dpres, ptr=lambda t: t.data_ptr())
    csoa, keep2 = batch.commitments_soa(dcm, ptr=lambda t: t.data_ptr())
    st = {k: torch.full((count,), 255, dtype=torch.uint8, device=dev) for k in ("compact", "batchable")}
    seed = bytes(range(32))
    stream_no = [0]
    lib = afx.lib()

    def compact():
        afx.check(lib.afx_verify_presentations_dev(issuer.h, C.byref(shape), C.byref(soa), count, st["compact"].data_ptr()))

    def batchable():
        stream_no[0] += 1
        rng = batch.device_rng(seed, stream_no[0])
        afx.check(lib.afx_verify_presentations_batchable_dev(issuer.h, C.byref(shape), C.byref(soa), C.byref(csoa), C.byref(rng), count, st["batchable"].data_ptr()))
    paths = {"compact": compact, "batchable": batchable}
    ext = torch.cuda.ExternalStream(issuer.stream)
    for f in paths.values():      # warm-up: workspaces, plan blobs, the weight buffer
        f()
    issuer.synchronize()
    same = all(np.array_equal(st[k].cpu().numpy(), want) for k in paths)
    times = {k: [] for k in paths}
    for _ in range(reps):
        for k, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext)
            f()
            e1.record(ext)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    mhz, stats, kt = {}, {}, {}
    for k, f in paths.items():
        issuer.set_timing(True)
        f()
        mhz[k] = issuer.core_clock_mhz()
        kt[k] = {}
        for kn in KERNELS:
            try:
                ms, launches = issuer.get_timing(kn)
            except afx.AfxError:
                continue
            if launches:
                kt[k][kn] = (ms, launches)
        issuer.set_timing(False)
        stats[k] = issuer.plan_stats()
    say("%s: %s, %d presentations device-resident, 1 %% damaged; statuses of both forms equal the expected ones: %s" % (name, layout, count, same))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k in paths:
        # (the clock probe sits in the windowed chain kernel's one-wave form: a plan that runs none of those reports no clock)
        say("  %-9s median %8.2f ms  %6.3f M presentations/s  core clock %s  (runs: %s)"
            % (k, med[k], count / med[k] / 1e3, ("%4.0f MHz" % mhz[k]) if mhz[k] else "not probed", " ".join("%.2f" % t for t in times[k])))
    spread = max(max(v) - min(v) for v in times.values())
    say("  batchable against compact: %+.1f %% time (%.2fx the rate); spread of the repeats: %.2f ms" % (100 * (med["batchable"] / med["compact"] - 1), med["compact"] / med["batchable"], spread))
    if name == "C3":
        for k in paths:
            say("  per-kernel times of one %s call: %s" % (k, "  ".join("%s %.2f ms/%d" % (kn, ms, nl) for kn, (ms, nl) in kt[k].items())))
            say("  operation counts per item (%s): %s" % (k, " ".join("%s=%d" % kv for kv in stats[k].items())))
    issuer.close()


def wire_leg(say, reps):
    """the AFXB doors against the column calls they wrap, C2 size, host memory in and out"""
    import time
    from aeonflux_amd import wire
    n, layout, hide, count, fixture = SIZES["C2"]
    params, key, ip = bench.load_fixture(fixture)
    issuer, user = afx.Context(params, key, ip), afx.Context(params, None, ip)
    captured = {}
    orig = batch.show_batchable

    def keep_args(ctx, *a, **k):
        captured["args"] = a
        return orig(ctx, *a, **k)
    batch.show_batchable = keep_args
    try:
        pres, cm, shape = generate_both(issuer, user, params, n, layout, hide, count, 778)
    finally:
        batch.show_batchable = orig
    a = captured["args"]
    item = dict(kinds=a[0], values=a[1], t=a[2], U=a[3], V=a[4], keypairs=a[5], z_wide=a[6], rng_seed=a[7], enc_seeds=a[8], M2=a[9], m3=a[10])
    blob = wire.pack_batchable(shape, pres, cm)
    seed = bytes(range(32))
    paths = {
        "verify, columns": lambda: batch.verify_presentations_batchable(issuer, shape, pres, cm, seed),
        "verify, AFXB   ": lambda: wire.verify_batchable_wire(issuer, blob, seed),
        "show, columns  ": lambda: batch.show_batchable(user, *a),
        "show, AFXB     ": lambda: wire.show_batchable_wire(user, [item]),
    }
    same = np.array_equal(paths["verify, columns"](), paths["verify, AFXB   "]()) and paths["show, AFXB     "]()[0] == blob
    times = {k: [] for k in paths}
    for _ in range(reps):
        for k, f in paths.items():
            t0 = time.perf_counter()
            f()
            times[k].append(1e3 * (time.perf_counter() - t0))
    say("AFXB doors against the column forms: C2 shape, %d items, host memory in and out (the Python mirror's array handling included); "
        "same statuses and bytes: %s" % (count, same))
    for k, v in times.items():
        say("  %s median %8.2f ms  (runs: %s)" % (k, statistics.median(v), " ".join("%.2f" % t for t in v)))
    issuer.close()
    user.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="C2,C3,C4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("batchable against compact presentation proofs (Issuer::verify), one MI355X, one process, calls alternating")
    for name in args.sizes.split(","):
        leg(say, torch, name, args.reps)
    wire_leg(say, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
