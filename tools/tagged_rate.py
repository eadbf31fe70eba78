"""Tagged against untagged presentations on one GPU (include/aeonflux_gpu.h "Presentation tags").

In ONE process, device-resident, the calls of a pair alternating, each timed `--reps` times (5) after one discarded leg with device
events around the whole call on its context's stream (median and all runs reported):
    afx_show_dev                  against  afx_show_tagged_dev
    afx_verify_presentations_dev  against  afx_verify_presentations_tagged_dev
and the inversion launch alone (afx_ctx_get_timing "k_sc_invert": device events around that one launch).  There is no target: the
comparison is each tagged call against its untagged twin in the same run.

Shapes.  A tag needs a hidden scalar, which neither the C3 workload of bench.py (S S P P e e e e: its scalars are revealed) nor any
8-attribute show has; so the two shapes are C3's layout with its first scalar hidden as well (s S P P e e e e, p = 0) and bench.py's
show shape (s S P e, p = 0), at 2^16 and 2^20 items.
    python tools/tagged_rate.py [--reps R] [--sizes 65536,1048576] [--out profiles/tagged_rate.txt]"""
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

# name -> (n, layout, hidden positions, p, fixture)
SHAPES = {"C3 layout, s S P P e e e e": (8, "SSPPEEEE", [0, 4, 5, 6, 7], 0, "c3_8attrs_SSPPeeee"),
          "show shape, s S P e": (4, "SSPE", [0, 3], 0, "readme_4attrs_sSPe")}


def credentials(issuer, params, n, layout, hide, count, seed):
    """synthetic credentials of one layout (as bench.generate makes them): dict of host arrays, the show kinds"""
    rng = np.random.default_rng(seed)
    rb = lambda *shape: rng.integers(0, 256, size=shape, dtype=np.uint8)
    values, M2, m3 = (np.zeros((n, count, 32), np.uint8) for _ in range(3))
    kinds = []
    for i, c in enumerate(layout):
        kinds.append({"S": afx.ATTR_PUBLIC_SCALAR, "P": afx.ATTR_PUBLIC_POINT, "E": afx.ATTR_EITHER_POINT}[c])
        values[i] = batch.scalars_from_wide(issuer, rb(count, 64)) if c == "S" else batch.points_from_uniform(issuer, rb(count, 64))
        if c == "E":
            M2[i] = batch.points_from_uniform(issuer, rb(count, 64))
            m3[i] = batch.scalars_from_wide(issuer, rb(count, 64))
    iss, st = batch.issue(issuer, kinds, values, rb(count, 64), rb(count, 64), rb(count, 32))
    assert not st.any(), "issue failed"
    skinds = list(kinds)
    for i in hide:
        skinds[i] = afx.ATTR_SECRET_SCALAR if skinds[i] == afx.ATTR_PUBLIC_SCALAR else afx.ATTR_SECRET_POINT
    nsp = sum(1 for k in skinds if k == afx.ATTR_SECRET_POINT)
    g = max(3, n)
    gen = lambda idx: np.frombuffer(params[4 + 32 * idx:4 + 32 * idx + 32], np.uint8)
    a, a0, a1 = (batch.scalars_from_wide(issuer, rb(count, 64)) for _ in range(3))
    pk, ok = batch.multiscalar_mul(issuer, np.stack([a, a0, a1]), np.stack([np.broadcast_to(gen(5 + g + n + 1 + k), (count, 32)) for k in range(3)]))
    assert ok.all()
    nonce = np.zeros((count, 32), np.uint8)
    nonce[:, :4] = rb(count, 4)
    return dict(values=values, M2=M2, m3=m3, t=iss["t"], U=iss["U"], V=iss["V"], a=a, a0=a0, a1=a1, pk=pk, z_wide=rb(count, 64), rng_seed=rb(count, 32),
                enc_seeds=rb(max(nsp, 1), count, 32), nonce=nonce, tag_seed=rb(count, 32)), skinds, nsp


def timed(torch, ctx, paths, reps):
    """the paths alternating: one discarded leg, then `reps` timed ones; ms per path"""
    ext = torch.cuda.ExternalStream(ctx.stream)
    for f in paths.values():
        f()
    ctx.synchronize()
    times = {k: [] for k in paths}
    for _ in range(reps):
        for k, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext)
            f()
            e1.record(ext)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return times


def leg(say, torch, name, count, reps):
    n, layout, hide, p, fixture = SHAPES[name]
    params, key, ip = bench.load_fixture(fixture)
    issuer, user = afx.Context(params, key, ip), afx.Context(params, None, ip)
    issuer.set_secret_independent_addressing(0)          # the synthetic credentials are no secrets
    host, kinds, nsp = credentials(issuer, params, n, layout, hide, count, 4242)
    issuer.set_secret_independent_addressing(2)
    hs = sum(1 for k in kinds if k == afx.ATTR_SECRET_SCALAR)
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in host.items()}
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)

    def outputs():
        o = {f: zeros(count, 32) for f in ("challenge", "C_x_0", "C_x_1", "C_V")}
        o.update(responses=zeros(3 + hs, count, 32), C_y=zeros(n, count, 32), attr_values=zeros(n, count, 32))
        o["enc"] = [{f: zeros(*((6, count, 32) if f == "responses" else (count, 32))) for f in batch.ENC_FIELDS} for _ in range(nsp)]
        return o
    plain, tagged = outputs(), outputs()
    tags = dict(T=zeros(count, 32), challenge=zeros(count, 32), responses=zeros(2, count, 32))
    st = {k: torch.full((count,), 255, dtype=torch.uint8, device=dev) for k in ("show", "show_tagged", "verify", "verify_tagged")}
    creds = {f: d[f] for f in ("values", "M2", "m3", "t", "U", "V")}
    kp = {f: d[f] for f in ("a", "a0", "a1", "pk")}
    rnd = dict(z_wide=d["z_wide"], rng_seed=d["rng_seed"], enc_seeds=d["enc_seeds"])
    H = batch.tag_scope_generator(user, b"tools/tagged_rate")
    lib = afx.lib()
    cs = afx.CredentialsSoA()
    cs.n_attributes = n
    for i, k in enumerate(kinds):
        cs.kinds[i] = k
    for f in creds:
        setattr(cs, f, creds[f].data_ptr())
    kps = afx.KeypairsSoA(*(kp[f].data_ptr() for f in ("a", "a0", "a1", "pk")))
    rs = afx.ShowRandomness(rnd["z_wide"].data_ptr(), rnd["rng_seed"].data_ptr(), rnd["enc_seeds"].data_ptr())
    eouts = (afx.EncProofOut * max(1, nsp))()
    for e, q in enumerate(plain["enc"]):
        for f in batch.ENC_FIELDS:
            setattr(eouts[e], f, q[f].data_ptr())
    po = afx.PresentationOut()
    for f in batch.PRES_FIELDS:
        setattr(po, f, plain[f].data_ptr())
    po.enc = C.cast(eouts, C.POINTER(afx.EncProofOut))
    shape = afx.Shape()

    def show():
        afx.check(lib.afx_show_dev(user.h, C.byref(cs), C.byref(kps) if nsp else None, C.byref(rs), count, C.byref(po), C.byref(shape), st["show"].data_ptr()))

    def show_tagged():
        batch.show_tagged_dev(user, kinds, creds, kp if nsp else None, rnd, p, H, d["nonce"], d["tag_seed"], count, tagged, tags, st["show_tagged"])
    t_show = timed(torch, user, {"show": show, "show_tagged": show_tagged}, reps)
    user.synchronize()
    same = all(torch.equal(plain[f], tagged[f]) for f in batch.PRES_FIELDS) and not st["show"].any().item() and not st["show_tagged"].any().item()
    soa, keep = batch.presentation_soa(tagged, ptr=lambda t: t.data_ptr())

    def verify():
        afx.check(lib.afx_verify_presentations_dev(issuer.h, C.byref(shape), C.byref(soa), count, st["verify"].data_ptr()))

    def verify_tagged():
        batch.verify_presentations_tagged_dev(issuer, shape, tagged, p, H, d["nonce"], tags, count, st["verify_tagged"])
    t_ver = timed(torch, issuer, {"verify": verify, "verify_tagged": verify_tagged}, reps)
    issuer.synchronize()
    accepted = not st["verify"].any().item() and not st["verify_tagged"].any().item()
    stats = {}
    for k, f, ctx in (("verify", verify, issuer), ("verify_tagged", verify_tagged, issuer), ("show", show, user), ("show_tagged", show_tagged, user)):
        f()
        ctx.synchronize()
        stats[k] = ctx.plan_stats()
    user.set_timing(True)
    inv = []
    for _ in range(reps + 1):
        show_tagged()
        ms, launches = user.get_timing("k_sc_invert")
        inv.append(ms / max(launches, 1))
        user.set_timing(True)          # (resets the sums)
    user.set_timing(False)
    inv = inv[1:]
    say("%s, p = %d, %d items device-resident; tagged show rows equal the untagged ones: %s; both verifiers accept every item: %s" % (name, p, count, same, accepted))
    for pair, times in ((("show", "show_tagged"), t_show), (("verify", "verify_tagged"), t_ver)):
        med = {k: statistics.median(times[k]) for k in pair}
        for k in pair:
            say("  %-13s median %9.2f ms  %6.3f M items/s  (runs: %s)" % (k, med[k], count / med[k] / 1e3, " ".join("%.2f" % t for t in times[k])))
        say("  %s against %s: %+.1f %% time" % (pair[1], pair[0], 100 * (med[pair[1]] / med[pair[0]] - 1)))
    say("  k_sc_invert alone: median %.3f ms  %.1f M inversions/s  (runs: %s)" % (statistics.median(inv), count / statistics.median(inv) / 1e3, " ".join("%.3f" % t for t in inv)))
    for k in ("show", "show_tagged", "verify", "verify_tagged"):
        say("  operation counts per item (%s): %s" % (k, " ".join("%s=%d" % kv for kv in stats[k].items())))
    issuer.close()
    user.close()


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
    say("tagged against untagged presentations, one MI355X, one process, the calls of a pair alternating, secret-independent addressing 2")
    for count in (int(x) for x in args.sizes.split(",")):
        for name in SHAPES:
            leg(say, torch, name, count, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
