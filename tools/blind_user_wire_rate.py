"""The blind user from attribute columns to request bytes (afx_blind_request_wire, afx_blind_request_wire_rng) and from issuance bytes to
the credential (afx_unblind_issuances_wire, afx_unblind_issuances_wire_rng) against the column paths and what a user agent does around
them today, on one GPU.  In the mould of tools/blind_wire_rate.py, whose layout, values and helpers it takes.

C5 layout (16 attributes, S x8 P x4 E x4) with 0, 1 and 4 of its positions hidden, 2^16 and 2^20 items in host memory, secret-independent
addressing 2.  For each door four paths in the same process, alternated, each timed 5 times after a warm-up (median and all runs):
  request   (a) afx_blind_request: host columns in, host columns out;
            (b) (a), then pack_blind_requests: what an agent does today (the packed bytes are made anew every time);
            (c) afx_blind_request_wire: columns in, the AFXQ section out;
            (d) afx_blind_request_wire_rng, against (e): os.urandom draws of d, r_wide and rng_seed, then (c);
  unblind   (a) afx_unblind_issuances on columns;
            (b) numpy unpacking of the AFXJ and AFXQ sections into those columns, then (a);
            (c) afx_unblind_issuances_wire: both sections and d in, t, U, V out;
            (d) afx_unblind_issuances_wire_rng: (c) with d derived again on the device (against (c): there is nothing to draw on the host).
(b) and (c) must give the same bytes.  The first shape is run once in full before anything is reported and that leg is thrown away.
With --tree DIR the two (a) are timed on another checkout's library (the parent commit's, built there) in a child process in the same
run, and on this tree's by the same child program before and after it: the column calls did not move if this tree's medians lie
within that checkout's own run-to-run spread, which is printed.  (The (a) of the legs shares its process with numpy packing and the
doors; it is set against the spread too, for what that says.)
There is no target: nobody has measured these doors before.
    python tools/blind_user_wire_rate.py [--sizes 65536,1048576] [--reps R] [--tree DIR] [--out FILE]"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blind_wire_rate as BW   # noqa: E402  (the layout, the synthetic values, the device's name)

N, HIDDEN = BW.N, BW.HIDDEN


def inputs_of(afx, batch, user, values, count, hidden):
    """(kinds, d, r_wide, rng_seed) of one leg"""
    rng = np.random.default_rng(6160 + count + len(hidden))
    rb = lambda *shape: rng.integers(0, 256, size=shape, dtype=np.uint8)
    kinds = BW.kinds_of(afx, hidden)
    h, _ = batch.blind_layout(kinds)
    return kinds, batch.scalars_from_wide(user, rb(count, 64)), rb(h, count, 64), rb(count, 32)


def request_call(afx, batch, user, kinds, values, d, r_wide, rng_seed, count):
    """afx_blind_request with every array allocated and touched once -> (call, request dict, statuses)"""
    h, hs = batch.blind_layout(kinds)
    o = dict(D=np.ones((count, 32), np.uint8), A=np.ones((h, count, 32), np.uint8), B=np.ones((h, count, 32), np.uint8), challenge=np.ones((count, 32), np.uint8),
             responses=np.ones((1 + h + hs, count, 32), np.uint8))
    st = np.zeros(count, np.uint8)
    a = batch._blind_attrs(kinds, values, batch._hptr)
    rnd = afx.BlindRequestRandomness(batch._hptr(r_wide), batch._hptr(rng_seed))
    out = afx.BlindRequestSoA(*(batch._hptr(o[f]) for f in batch.REQUEST_FIELDS))
    lib = afx.lib()

    def call():
        afx.check(lib.afx_blind_request(user.h, C.byref(a), d.ctypes.data, C.byref(rnd), count, C.byref(out), st.ctypes.data))
    call.keep = (a, rnd, out)
    return call, o, st


def unblind_call(afx, batch, user, kinds, values, d, req, iss, count, outputs=None):
    """afx_unblind_issuances on columns (outputs: (V, statuses) to write into) -> (call, V, statuses)"""
    V, st = outputs or (np.ones((count, 32), np.uint8), np.zeros(count, np.uint8))
    a = batch._blind_attrs(kinds, values, batch._hptr)
    soa = afx.BlindRequestSoA(batch._hptr(req["D"]), batch._hptr(req["A"]), batch._hptr(req["B"]), None, None)
    s = afx.BlindIssuanceSoA(*(batch._hptr(iss[f]) for f in batch.BLIND_ISSUANCE_FIELDS))
    lib = afx.lib()

    def call():
        afx.check(lib.afx_unblind_issuances(user.h, C.byref(a), d.ctypes.data, C.byref(soa), C.byref(s), N + 6, count, V.ctypes.data, st.ctypes.data))
    call.keep = (a, soa, s)
    return call, V, st


def timed(paths, reps):
    times = {k: [] for k, _ in paths}
    for _ in range(reps):
        for k, f in paths:
            t0 = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t0)
    return times


def child(args):
    """the two (a) alone, in a process of its own, on the package and library of the checkout at args.root"""
    sys.path.insert(0, args.root)
    import aeonflux_amd as afx
    import bench
    from aeonflux_amd import batch
    params, key, ip = bench.load_fixture("c5_16attrs")
    issuer, user = afx.Context(params, key, ip), afx.Context(params, None, ip)
    res = {}
    sizes = [int(x) for x in args.sizes.split(",")]
    legs = [(c, nh) for c in sizes for nh in sorted(HIDDEN)]
    values = {}
    for k, (count, nh) in enumerate(legs[:1] + legs):          # (the first leg twice, its first run thrown away, as in the parent process)
        if count not in values:
            user.set_secret_independent_addressing(0)
            values = {count: BW.synthetic_values(batch, user, count)}
            user.set_secret_independent_addressing(2)
        kinds, d, r_wide, rng_seed = inputs_of(afx, batch, user, values[count], count, HIDDEN[nh])
        call_q, req, st_q = request_call(afx, batch, user, kinds, values[count], d, r_wide, rng_seed, count)
        call_q()
        rng = np.random.default_rng(7)
        iss, st_i = batch.issue_blind(issuer, kinds, values[count], req, *(rng.integers(0, 256, size=(count, w), dtype=np.uint8) for w in (64, 64, 64, 32)))
        call_u, V, st_u = unblind_call(afx, batch, user, kinds, values[count], d, req, iss, count)
        call_u()
        times = timed((("request", call_q), ("unblind", call_u)), args.reps)
        assert not st_q.any() and not st_i.any() and not st_u.any()
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
    say("the user's doors of blind issuance against the column paths: C5 (c5_16attrs, S x8 P x4 E x4), arrays in host memory,")
    say("one GPU (%s), one process, calls alternating, secret-independent addressing 2; medians of %d" % (BW.device_name(afx), args.reps))
    lib = afx.lib()
    other, alone = None, []

    def run_child(root):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", os.path.abspath(root), "--sizes", args.sizes, "--reps", str(args.reps)],
                           capture_output=True, text=True, cwd=os.path.abspath(root))
        tail = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
        if r.returncode == 0 and tail:
            return json.loads(tail[-1][6:])
        say("(--tree: the run of the checkout %s failed: %s)" % (os.path.basename(os.path.normpath(root)), (r.stderr or r.stdout)[-300:].replace("\n", " | ")))
        return None
    if args.tree:
        # like for like: the same child program - the two column calls and nothing else in the process - on this tree, on the other
        # checkout and on this tree again (the (a) of the legs below shares its process with numpy packing and the doors)
        alone.append(run_child(ROOT))
        other = run_child(args.tree)
        alone.append(run_child(ROOT))
    sizes = [int(x) for x in args.sizes.split(",")]
    legs = [(c, nh) for c in sizes for nh in sorted(HIDDEN)]
    values = {}
    seed = bytes(range(32, 64))
    for leg, (count, nh) in enumerate(legs[:1] + legs):
        report = say if leg else (lambda s: say("  [first leg of the process, thrown away] " + s.strip()))
        if count not in values:
            user.set_secret_independent_addressing(0)      # input generation: synthetic values are no secrets
            values = {count: BW.synthetic_values(batch, user, count)}
            user.set_secret_independent_addressing(2)
        vals = values[count]
        kinds, d, r_wide, rng_seed = inputs_of(afx, batch, user, vals, count, HIDDEN[nh])
        h, hs = batch.blind_layout(kinds)
        cells_q = 3 + 2 * h + hs + N
        # ---- the request ----
        call_a, req, st_a = request_call(afx, batch, user, kinds, vals, d, r_wide, rng_seed, count)
        group = dict(kinds=kinds, values=vals, d=d, r_wide=r_wide, rng_seed=rng_seed)
        arr, keep = wire._blind_request_groups([group], True)
        olen, ocnt = C.c_size_t(0), C.c_size_t(0)
        afx.check(lib.afx_blind_request_wire(user.h, arr, 1, None, 0, C.byref(olen), None, 0, C.byref(ocnt)))
        out_c, out_d, st_c, d_out = np.ones(olen.value, np.uint8), np.ones(olen.value, np.uint8), np.zeros(count, np.uint8), np.ones((count, 32), np.uint8)
        rng = afx.DeviceRng(seed, 1000 * leg)
        kept = {}

        def req_b():
            call_a()
            kept["b"] = wire.pack_blind_requests(kinds, vals, req)

        def req_c(a=arr):
            afx.check(lib.afx_blind_request_wire(user.h, a, 1, out_c.ctypes.data, out_c.size, C.byref(olen), st_c.ctypes.data, count, C.byref(ocnt)))

        def req_d():
            rng.stream += 1
            afx.check(lib.afx_blind_request_wire_rng(user.h, arr, 1, C.byref(rng), d_out.ctypes.data, out_d.ctypes.data, out_d.size, C.byref(olen), st_c.ctypes.data, count,
                                                     C.byref(ocnt)))

        def req_e():
            fd = np.frombuffer(os.urandom(count * 32), np.uint8).reshape(count, 32).copy()
            fd[:, 31] &= 0x0F          # below 2^252: canonical
            fresh = dict(group, d=fd, r_wide=np.frombuffer(os.urandom(h * count * 64), np.uint8).reshape(h, count, 64), rng_seed=np.frombuffer(os.urandom(count * 32), np.uint8))
            a2, keep2 = wire._blind_request_groups([fresh], True)
            req_c(a2)
        paths = (("a", call_a), ("b", req_b), ("c", req_c), ("d", req_d), ("e", req_e))
        for _, f in paths[:4]:          # warm-up: plans, staging buffers, pinned images
            f()
        req_c()
        same = kept["b"] == bytes(out_c) and not st_a.any() and not st_c.any()
        times = timed(paths, args.reps)
        ok_d = not st_c.any()
        med = {k: statistics.median(v) for k, v in times.items()}
        report("%d hidden position%s, %d items, the request (%d B of values, d and randomness in, AFXQ record %d B out); (b) and (c) byte-equal, statuses 0: %s; (d), (e) statuses 0: %s"
               % (nh, "" if nh == 1 else "s", count, N * 32 + 64 + 64 * h, cells_q * 32, same, ok_d))
        for k, label in (("a", "(a) afx_blind_request, columns in/out       "), ("b", "(b) (a) + pack_blind_requests               "),
                         ("c", "(c) afx_blind_request_wire, AFXQ out        "), ("d", "(d) afx_blind_request_wire_rng              "),
                         ("e", "(e) os.urandom draws + (c)                  ")):
            report("  %s median %8.1f ms  %6.3f M requests/s  (runs: %s)" % (label, 1e3 * med[k], count / med[k] / 1e6, " ".join("%.1f" % (1e3 * t) for t in times[k])))
        report("  (c) against (a): %+.1f %% time; (c) against (b): %+.1f %%; (d) against (e): %+.1f %%; (d) against (c): %+.1f %%"
               % (100 * (med["c"] / med["a"] - 1), 100 * (med["c"] / med["b"] - 1), 100 * (med["d"] / med["e"] - 1), 100 * (med["d"] / med["c"] - 1)))
        med_req_a = med["a"]
        # ---- the unblinding: the requests of the _rng door at one (seed, stream), so that both forms answer one AFXJ section ----
        rng.stream += 1
        stream_u = rng.stream
        req_d_once = lambda: afx.check(lib.afx_blind_request_wire_rng(user.h, arr, 1, C.byref(rng), d_out.ctypes.data, out_d.ctypes.data, out_d.size, C.byref(olen),
                                                                      st_c.ctypes.data, count, C.byref(ocnt)))
        req_d_once()
        afxq, du = bytes(out_d), d_out.copy()
        afxj, st_i = wire.issue_blind_wire_rng(issuer, afxq)
        assert not st_i.any()
        _, _, q_cols = wire.unpack_blind_requests(afxq)
        _, j_cols = wire.unpack_blind_issuances(afxj)
        call_ua, V_a, st_ua = unblind_call(afx, batch, user, kinds, vals, du, q_cols, j_cols, count)
        outputs_b = (np.ones((count, 32), np.uint8), np.zeros(count, np.uint8))
        cols_c = [np.ones((count, 32), np.uint8) for _ in range(3)]
        cols_d = [np.ones((count, 32), np.uint8) for _ in range(3)]
        co_c, co_d = afx.CredentialOut(*(a.ctypes.data for a in cols_c)), afx.CredentialOut(*(a.ctypes.data for a in cols_d))
        st_uc, st_ud = np.zeros(count, np.uint8), np.zeros(count, np.uint8)
        rng_u = afx.DeviceRng(seed, stream_u)

        def unb_b():
            k2, v2, q2 = wire.unpack_blind_requests(afxq)
            _, j2 = wire.unpack_blind_issuances(afxj)
            for i in range(N):          # the agent's own values stand in the rows AFXQ does not carry
                if kinds[i] in (1, 4):
                    v2[i] = vals[i]
            call, V2, st2 = unblind_call(afx, batch, user, k2, v2, du, q2, j2, count, outputs_b)
            call()
            kept["ub"] = (j2["t"], j2["U"], V2)

        def unb_c():
            afx.check(lib.afx_unblind_issuances_wire(user.h, afxj, len(afxj), afxq, len(afxq), du.ctypes.data, C.byref(co_c), st_uc.ctypes.data, count, C.byref(ocnt)))

        def unb_d():
            afx.check(lib.afx_unblind_issuances_wire_rng(user.h, afxj, len(afxj), afxq, len(afxq), C.byref(rng_u), C.byref(co_d), st_ud.ctypes.data, count, C.byref(ocnt)))
        upaths = (("a", call_ua), ("b", unb_b), ("c", unb_c), ("d", unb_d))
        for _, f in upaths:
            f()
        same_u = all(np.array_equal(x, y) for x, y in zip(kept["ub"], cols_c)) and all(np.array_equal(x, y) for x, y in zip(cols_c, cols_d)) \
            and not st_ua.any() and not st_uc.any() and not st_ud.any() and not outputs_b[1].any()
        utimes = timed(upaths, args.reps)
        umed = {k: statistics.median(v) for k, v in utimes.items()}
        report("%d hidden position%s, %d items, the unblinding (AFXJ record %d B + AFXQ record %d B + d in, 96 B out); (b), (c) and (d) equal, statuses 0: %s"
               % (nh, "" if nh == 1 else "s", count, (N + 11) * 32, cells_q * 32, same_u))
        for k, label in (("a", "(a) afx_unblind_issuances, columns          "), ("b", "(b) numpy unpack of AFXJ and AFXQ + (a)     "),
                         ("c", "(c) afx_unblind_issuances_wire, bytes in    "), ("d", "(d) afx_unblind_issuances_wire_rng          ")):
            report("  %s median %8.1f ms  %6.3f M credentials/s  (runs: %s)" % (label, 1e3 * umed[k], count / umed[k] / 1e6, " ".join("%.1f" % (1e3 * t) for t in utimes[k])))
        report("  (c) against (a): %+.1f %% time; (c) against (b): %+.1f %%; (d) against (c): %+.1f %%"
               % (100 * (umed["c"] / umed["a"] - 1), 100 * (umed["c"] / umed["b"] - 1), 100 * (umed["d"] / umed["c"] - 1)))
        if other and leg:
            key = "%d/%d" % (count, nh)
            t = other.get(key)
            for name, mine in (("request", med_req_a), ("unblind", umed["a"])):
                if not t or not t.get(name):
                    continue
                lo, hi, m = min(t[name]), max(t[name]), statistics.median(t[name])
                where = lambda x: "within" if lo <= x <= hi else ("below" if x < lo else "ABOVE")
                report("  (a) %s on the other checkout (%s), alone in its process: median %8.1f ms, runs %.1f .. %.1f ms (%s)"
                       % (name, os.path.basename(os.path.normpath(args.tree)), 1e3 * m, 1e3 * lo, 1e3 * hi, " ".join("%.1f" % (1e3 * x) for x in t[name])))
                for when, a in zip(("before", "after"), alone):
                    if a and a.get(key):
                        ma = statistics.median(a[key][name])
                        report("      this tree alone in its process, %s it: median %8.1f ms (runs: %s), %+.1f %%: %s its spread"
                               % (when, 1e3 * ma, " ".join("%.1f" % (1e3 * x) for x in a[key][name]), 100 * (ma / m - 1), where(ma)))
                report("      this tree's (a) above, beside the other paths: median %8.1f ms, %+.1f %%: %s its spread" % (1e3 * mine, 100 * (mine / m - 1), where(mine)))
    issuer.close()
    user.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
