"""Plaintexts from bytes, derived keypairs and decryption on one GPU: the three host-pointer calls that hash
(afx_plaintexts_from_bytes, afx_keypairs_derive, afx_decrypt), timed with a host clock around the call, and - where the tree has
them - the *_dev forms, timed with device events, at 2^16 and 2^20 items; every figure the median of --reps runs after a warm-up.
Also how many candidates encode_to_group tried per 64-lane wave (a wave waits for its slowest lane), from the counters the call
returns.

--tree DIR imports the package of another checkout of this repository (with its library built), so that the parent commit's tree
is measured by the same script on the same box, alternated with this one:
    for r in 1 2 3; do python tools/plaintext_rate.py --tree variants/parent_tree; python tools/plaintext_rate.py; done
    python tools/plaintext_rate.py [--tree DIR] [--reps R] [--counts 65536,1048576] [--out FILE]"""
import argparse
import ctypes as C
import hashlib
import os
import statistics
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--counts", default="65536,1048576")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import torch   # (before the library: the HIP runtime inside the torch wheel does not initialise once the system's has)
    torch.cuda.init()
    import aeonflux_amd as afx
    import bench
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    L = afx.lib()
    has_dev = hasattr(L, "afx_decrypt_dev")
    say("plaintext / keypair / decrypt rates, tree %s (%s)" % (os.path.relpath(tree), "with *_dev forms" if has_dev else "host-pointer forms only"))
    params, key, ip = bench.load_fixture("readme_4attrs_sSPe")
    ctx = afx.Context(params, None, ip)
    p = lambda a: a.ctypes.data

    def med(f):
        f()   # warm-up: plans, staging buffers
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), ts

    def line(name, count, m, ts):
        say("  %-34s median %9.2f ms  %8.3f M items/s  (runs: %s)" % (name, 1e3 * m, count / m / 1e6, " ".join("%.2f" % (1e3 * t) for t in ts)))

    for count in (int(c) for c in args.counts.split(",")):
        say("%d items:" % count)
        msgs = np.frombuffer(hashlib.shake_256(b"plaintext-rate/messages").digest(30 * count), np.uint8).reshape(count, 30)
        ms = np.frombuffer(hashlib.shake_256(b"plaintext-rate/master-secrets").digest(64 * count), np.uint8).reshape(count, 64)
        M1, M2, m3, E1, E2, D1, D2, d3 = (np.ones((count, 32), np.uint8) for _ in range(8))
        kp = [np.ones((count, 32), np.uint8) for _ in range(4)]
        ctr, st, out_msgs = np.ones(count, np.uint32), np.ones(count, np.uint8), np.ones((count, 30), np.uint8)
        soa = afx.KeypairsSoA(*(p(x) for x in kp))
        plain = lambda: afx.check(L.afx_plaintexts_from_bytes(ctx.h, p(msgs), count, p(M1), p(M2), p(m3), p(ctr)))
        derive = lambda: afx.check(L.afx_keypairs_derive(ctx.h, p(ms), count, *(p(x) for x in kp)))
        decrypt = lambda: afx.check(L.afx_decrypt(ctx.h, C.byref(soa), p(E1), p(E2), count, p(D1), p(D2), p(d3), p(out_msgs), p(st)))
        m, ts = med(plain)
        line("afx_plaintexts_from_bytes (host)", count, m, ts)
        tries = ctr.astype(np.int64) + 1
        waves = tries[:count - count % 64].reshape(-1, 64).max(axis=1)
        say("    encode_to_group: tries per message mean %.2f max %d; per 64-lane wave (its slowest lane) mean %.2f max %d"
            % (tries.mean(), tries.max(), waves.mean(), waves.max()))
        m, ts = med(derive)
        line("afx_keypairs_derive (host)", count, m, ts)
        afx.check(L.afx_encrypt(ctx.h, C.byref(soa), p(M1), p(M2), p(m3), count, p(E1), p(E2), p(st)))
        assert not st.any()
        m, ts = med(decrypt)
        assert not st.any() and np.array_equal(out_msgs, msgs) and np.array_equal(D1, M1)
        line("afx_decrypt (host)", count, m, ts)
        if not has_dev:
            continue
        dv = lambda a: torch.from_numpy(a).cuda()
        d = {k: dv(v) for k, v in dict(msgs=msgs, ms=ms, M1=M1, M2=M2, m3=m3, E1=E1, E2=E2, D1=D1, D2=D2, d3=d3, st=st, out=out_msgs, a=kp[0], a0=kp[1], a1=kp[2], pk=kp[3]).items()}
        dctr = torch.zeros(count, dtype=torch.int32, device="cuda")
        q = lambda k: d[k].data_ptr()
        dsoa = afx.KeypairsSoA(q("a"), q("a0"), q("a1"), q("pk"))
        stream = torch.cuda.ExternalStream(L.afx_ctx_stream(ctx.h))

        def med_dev(f):
            f()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f()
                e1.record(stream)
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) / 1e3)
            return statistics.median(ts), ts
        m, ts = med_dev(lambda: afx.check(L.afx_plaintexts_from_bytes_dev(ctx.h, q("msgs"), count, q("M1"), q("M2"), q("m3"), dctr.data_ptr(), q("st"))))
        line("afx_plaintexts_from_bytes_dev", count, m, ts)
        m, ts = med_dev(lambda: afx.check(L.afx_keypairs_derive_dev(ctx.h, q("ms"), count, q("a"), q("a0"), q("a1"), q("pk"))))
        line("afx_keypairs_derive_dev", count, m, ts)
        m, ts = med_dev(lambda: afx.check(L.afx_encrypt_dev(ctx.h, C.byref(dsoa), q("M1"), q("M2"), q("m3"), count, q("E1"), q("E2"), q("st"))))
        line("afx_encrypt_dev", count, m, ts)
        m, ts = med_dev(lambda: afx.check(L.afx_decrypt_dev(ctx.h, C.byref(dsoa), q("E1"), q("E2"), count, q("D1"), q("D2"), q("d3"), q("out"), q("st"))))
        line("afx_decrypt_dev", count, m, ts)
        torch.cuda.synchronize()
        assert not d["st"].any() and np.array_equal(d["out"].cpu().numpy(), msgs)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
