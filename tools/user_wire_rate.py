"""The user side on bytes against the column paths it replaces, on one GPU.

show (AnonymousCredential::show) at bench.py's show shape (readme_4attrs_sSPe: s S P e, attributes 0 and 3 hidden) with 2^16 and 2^20
credentials in host memory:
  (a) afx_show: host columns in, host columns out;
  (b) (a) followed by afx_wire_pack_presentations: the AFXP batch a user has to send today;
  (c) afx_show_wire: the AFXP batch straight from the call.
user-side verify (CredentialIssuance::verify) on the C5 layout (c5_16attrs: S x8 P x4 E x4) with 2^20 issuances:
  (a) afx_verify_issuances on columns;
  (b) afx_verify_issuances_mixed_wire on one AFXI section;
  (c) the same on a stream of 64 sections of 4 layouts (2^18 issuances each), interleaved.
Secret modes 2 and 0; the paths alternate, each timed 5 times (median reported).  Also the core clock of a separate (c) run and
whether the paths wrote the same bytes and statuses.
    python tools/user_wire_rate.py [--reps R] [--out FILE] [--counts 65536,1048576] [--verify-count N]"""
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


def report(say, times, labels, count, unit):
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, label in labels:
        say("  %s median %8.1f ms  %6.3f M %s/s  (runs: %s)" % (label, 1e3 * med[k], count / med[k] / 1e6, unit, " ".join("%.1f" % (1e3 * t) for t in times[k])))
    return med


def clock(ctx, f):
    ctx.set_timing(True)
    f()
    mhz = ctx.core_clock_mhz()
    ctx.set_timing(False)
    return mhz


def show_leg(say, reps, count):
    params, key, ip = bench.load_fixture("readme_4attrs_sSPe")
    issuer, user = afx.Context(params, key, ip), afx.Context(params, None, ip)
    # the bench's credentials (issue + keypairs on the GPU; input generation in the fastest mode)
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
    item = dict(kinds=skinds, values=values, M2=M2, m3=m3, t=iss["t"], U=iss["U"], V=iss["V"], keypairs=dict(zip(("a", "a0", "a1", "pk"), kp)),
                z_wide=rb(count, 64), rng_seed=rb(count, 32), enc_seeds=rb(1, count, 32))
    lib = afx.lib()
    # (a) / (b): columns, allocated and touched once
    cs, kpp, rnd, out, o, cnt, keep = batch._show_args(skinds, values, iss["t"], iss["U"], iss["V"], item["keypairs"], item["z_wide"], item["rng_seed"],
                                                       item["enc_seeds"], M2, m3)
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.fill(1)
    shape = afx.Shape()
    st_a = np.zeros(count, np.uint8)
    soa, keep2 = batch.presentation_soa(o)
    blen = C.c_size_t(0)
    afx.check(lib.afx_show(user.h, C.byref(cs), C.byref(kpp), C.byref(rnd), count, C.byref(out), C.byref(shape), st_a.ctypes.data))
    afx.check(lib.afx_wire_pack_presentations(C.byref(shape), C.byref(soa), count, None, 0, C.byref(blen)))
    blob_b = np.ones(blen.value, np.uint8)
    # (c): one group, the AFXP buffer and statuses allocated and touched once
    grp = (afx.ShowGroup * 1)()
    grp[0].creds, grp[0].rnd, grp[0].count, grp[0].keypairs = cs, rnd, count, C.pointer(kpp)
    olen = C.c_size_t(0)
    afx.check(lib.afx_show_wire(user.h, grp, 1, None, 0, C.byref(olen), None, 0))
    blob_c = np.ones(olen.value, np.uint8)
    st_c = np.zeros(count, np.uint8)

    def path_a():
        afx.check(lib.afx_show(user.h, C.byref(cs), C.byref(kpp), C.byref(rnd), count, C.byref(out), C.byref(shape), st_a.ctypes.data))

    def path_b():
        path_a()
        afx.check(lib.afx_wire_pack_presentations(C.byref(shape), C.byref(soa), count, blob_b.ctypes.data, blob_b.size, C.byref(blen)))

    def path_c():
        afx.check(lib.afx_show_wire(user.h, grp, 1, blob_c.ctypes.data, blob_c.size, C.byref(olen), st_c.ctypes.data, count))
    cells = lib.afx_wire_cells_per_record(C.byref(shape))
    say("show: bench.py's show shape (readme_4attrs_sSPe, s S P e), %d credentials in host memory; %d B AFXP record" % (count, cells * 32))
    for mode in (2, 0):
        user.set_secret_independent_addressing(mode)
        times = timed({"a": path_a, "b": path_b, "c": path_c}, reps)
        same = bytes(blob_b) == bytes(blob_c) and np.array_equal(st_a, st_c) and not st_c.any()
        mhz = clock(user, path_c)
        say("mode %d (%s):" % (mode, "secret-independent prover-side addressing" if mode == 2 else "fastest tables"))
        med = report(say, times, (("a", "(a) afx_show, columns in/out              "), ("b", "(b) afx_show + afx_wire_pack_presentations"),
                                  ("c", "(c) afx_show_wire, AFXP out               ")), count, "presentations")
        say("  (c) against (a): %+.1f %% time; against (b): %+.1f %% time" % (100 * (med["c"] / med["a"] - 1), 100 * (med["c"] / med["b"] - 1)))
        say("  core clock during a (c) run: %.0f MHz;  (b) and (c) byte-equal (AFXP bytes and statuses, all OK): %s" % (mhz, same))
    user.close()


def verify_leg(say, reps, count):
    params, key, ip = bench.load_fixture("c5_16attrs")
    issuer, user = afx.Context(params, key, ip), afx.Context(params, None, ip)
    issuer.set_secret_independent_addressing(0)   # input generation only
    rng = np.random.default_rng(20261017)
    rb = lambda *s: rng.integers(0, 256, size=s, dtype=np.uint8)
    layouts = ["S" * 8 + "P" * 4 + "E" * 4, "P" * 4 + "S" * 8 + "E" * 4, "E" * 4 + "P" * 4 + "S" * 8, "SPE" * 5 + "S"]

    def issued(layout, cnt):
        kinds = [{"S": afx.ATTR_PUBLIC_SCALAR, "P": afx.ATTR_PUBLIC_POINT, "E": afx.ATTR_EITHER_POINT}[c] for c in layout]
        values = np.zeros((16, cnt, 32), np.uint8)
        for i, c in enumerate(layout):
            for o in range(0, cnt, 1 << 18):
                w = rb(min(1 << 18, cnt - o), 64)
                values[i, o:o + w.shape[0]] = batch.scalars_from_wide(issuer, w) if c == "S" else batch.points_from_uniform(issuer, w)
        got, st = wire.issue_wire(issuer, wire.pack_requests(kinds, values), {"t_wide": rb(cnt, 64), "U_wide": rb(cnt, 64), "rng_seed": rb(cnt, 32)})
        assert not st.any()
        return got
    one = issued(layouts[0], count)
    per = count // 4
    parts = [issued(lo, per) for lo in layouts[1:]]
    # 64 sections: 16 slices of each of 4 layouts, interleaved (the first layout's slices from the one-section batch)
    hdr = afx.lib().afx_issuance_wire_header_bytes(16)
    secs = []
    for s in range(16):
        for k in range(4):
            src = one if k == 0 else parts[k - 1]
            cells = 4 + 21 + 16
            lo = s * (per // 16)
            rec = np.frombuffer(src, np.uint8, offset=hdr + lo * cells * 32, count=(per // 16) * cells * 32)
            secs.append(src[:8] + np.uint32(per // 16).tobytes() + src[12:hdr] + rec.tobytes())
    stream = b"".join(secs)
    issuer.close()
    kinds, values, iss = wire.unpack_issuances(one)
    req, s, nr, cnt, keep = batch._issuance_args(kinds, values, iss)
    lib = afx.lib()
    st = {k: np.zeros(count, np.uint8) for k in "abc"}
    n = C.c_size_t(0)

    def path_a():
        afx.check(lib.afx_verify_issuances(user.h, C.byref(req), C.byref(s), nr, count, st["a"].ctypes.data))

    def path_b():
        afx.check(lib.afx_verify_issuances_mixed_wire(user.h, one, len(one), st["b"].ctypes.data, count, C.byref(n)))

    def path_c():
        afx.check(lib.afx_verify_issuances_mixed_wire(user.h, stream, len(stream), st["c"].ctypes.data, count, C.byref(n)))
    say("user-side verify: C5 (c5_16attrs, S x8 P x4 E x4), %d issuances in host memory; (c) = 64 AFXI sections of 4 layouts (%d each)"
        % (count, per // 16))
    for mode in (2, 0):
        user.set_secret_independent_addressing(mode)
        times = timed({"a": path_a, "b": path_b, "c": path_c}, reps)
        same = np.array_equal(st["a"], st["b"]) and not st["b"].any() and not st["c"].any()
        mhz = clock(user, path_c)
        say("mode %d (%s):" % (mode, "secret-independent prover-side addressing" if mode == 2 else "fastest tables"))
        med = report(say, times, (("a", "(a) afx_verify_issuances, columns          "), ("b", "(b) afx_verify_issuances_mixed_wire, 1 sec "),
                                  ("c", "(c) afx_verify_issuances_mixed_wire, 64 sec")), count, "issuances")
        say("  (b) against (a): %+.1f %% time; (c) against (b): %+.1f %% time" % (100 * (med["b"] / med["a"] - 1), 100 * (med["c"] / med["b"] - 1)))
        say("  core clock during a (c) run: %.0f MHz;  (a) and (b) equal statuses, (a), (b), (c) all OK: %s" % (mhz, same))
    user.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--counts", default="65536,1048576")
    ap.add_argument("--verify-count", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("the user side on bytes against the column paths, one MI355X")
    for count in (int(c) for c in args.counts.split(",")):
        show_leg(say, args.reps, count)
    verify_leg(say, args.reps, args.verify_count)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
