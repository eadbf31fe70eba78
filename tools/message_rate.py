"""Whole-message calls against what a caller did before them, on one GPU (include/aeonflux_gpu.h "whole messages").

In ONE process, alternating, each new host-pointer call is timed against the composition it replaces, on the same messages and keys:
  afx_plaintexts_from_messages   vs  numpy chunking and padding + afx_plaintexts_from_bytes
  afx_encrypt_messages           vs  numpy chunking + key replication (one row per chunk) + afx_plaintexts_from_bytes + afx_encrypt
                                     + numpy status reduction and zeroing of failed messages
  afx_decrypt_messages           vs  key replication + afx_decrypt + numpy status reduction and zeroing
  afx_plaintexts_from_bytes_at   vs  afx_plaintexts_from_bytes on the same 30-byte rows (the counters kept from a first call)
Sizes: 2^16 and 2^20 chunks as messages of 30, 200 and 3000 bytes.  Every leg is run once and discarded, then 5 times; medians and all
runs are reported, from a host clock around calls that end synchronised (the host-pointer forms fetch their results).  The two sides'
results are compared before anything is timed, and the first configuration is run once in full, unreported, before any is timed (the
first calls of a process grow the staging buffers and pinned images: legs of ~30 ms among legs of 3 ms).  There is no target: the yardstick is the composition of existing calls in the same
run.
    python tools/message_rate.py [--reps R] [--chunks 65536,1048576] [--lengths 30,200,3000] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aeonflux_amd as afx  # noqa: E402
import bench  # noqa: E402
from aeonflux_amd import batch  # noqa: E402


def chunk_rows(blob, offsets, cf):
    """what a caller does in numpy: [n_chunks, 30] zero-padded rows of the messages"""
    n = int(cf[-1])
    rows = np.zeros((n, 30), np.uint8)
    lens = (offsets[1:] - offsets[:-1]).astype(np.int64)
    if lens.size and (lens == lens[0]).all() and lens[0] % 30 == 0:       # (equal lengths that are whole chunks: a reshape)
        return np.ascontiguousarray(blob[int(offsets[0]):int(offsets[-1])].reshape(n, 30))
    per = (cf[1:] - cf[:-1]).astype(np.int64)
    msg = np.repeat(np.arange(lens.size), per)                             # the message of every chunk
    k = np.arange(n) - np.repeat(cf[:-1].astype(np.int64), per)            # its number inside the message
    start = offsets[:-1].astype(np.int64)[msg] + 30 * k
    take = np.minimum(30, offsets[1:].astype(np.int64)[msg] - start)
    idx = start[:, None] + np.arange(30)[None, :]
    mask = np.arange(30)[None, :] < take[:, None]
    rows[mask] = blob[np.where(mask, idx, 0)][mask]
    return rows


def old_from_messages(ctx, blob, offsets, cf):
    return batch.plaintexts_from_bytes(ctx, chunk_rows(blob, offsets, cf))


def old_encrypt(ctx, kp, blob, offsets, cf):
    per = (cf[1:] - cf[:-1]).astype(np.int64)
    rep = np.repeat(np.arange(per.size), per)
    M1, M2, m3, ctr = batch.plaintexts_from_bytes(ctx, chunk_rows(blob, offsets, cf))
    E1, E2, st = batch.encrypt(ctx, {f: kp[f][rep] for f in ("a", "a0", "a1")}, M1, M2, m3)
    status = np.zeros(per.size, np.uint8)
    status[rep[st != 0]] = afx.ST_VERIFICATION_FAILURE
    dead = status[rep] != 0
    E1[dead] = 0
    E2[dead] = 0
    return E1, E2, ctr, status


def old_decrypt(ctx, kp, E1, E2, cf):
    per = (cf[1:] - cf[:-1]).astype(np.int64)
    rep = np.repeat(np.arange(per.size), per)
    _, _, _, rows, st = batch.decrypt(ctx, {f: kp[f][rep] for f in ("a", "a0", "a1")}, E1, E2)
    status = np.zeros(per.size, np.uint8)
    status[rep[st != 0]] = afx.ST_UNDECRYPTABLE
    rows[status[rep] != 0] = 0
    return rows, status


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def pair(say, what, unit_count, new, old, reps):
    """one discarded leg, then `reps` alternating legs of (new, old)"""
    timed(new), timed(old)
    tn, to = [], []
    for _ in range(reps):
        tn.append(timed(new)[0])
        to.append(timed(old)[0])
    mn, mo = statistics.median(tn), statistics.median(to)
    say("  %-30s new median %9.2f ms  %7.3f M chunks/s  (runs: %s)" % (what, mn, unit_count / mn / 1e3, " ".join("%.2f" % t for t in tn)))
    say("  %-30s old median %9.2f ms  %7.3f M chunks/s  (runs: %s)" % ("", mo, unit_count / mo / 1e3, " ".join("%.2f" % t for t in to)))
    say("  %-30s new against old: %.2fx the time; spread of the repeats: new %.2f ms, old %.2f ms" % ("", mn / mo, max(tn) - min(tn), max(to) - min(to)))


def run_config(say, ctx, n_chunks, length, reps):
    per = (length + 29) // 30
    count = max(1, n_chunks // per)
    rng = np.random.default_rng(7000 + length + n_chunks)
    blob = rng.integers(0, 256, size=count * length, dtype=np.uint8)
    offsets = (np.arange(count + 1, dtype=np.uint64) * np.uint64(length))
    cf = batch.chunk_table(offsets)
    n = int(cf[-1])
    kp = batch.keypairs_derive(ctx, rng.integers(0, 256, size=(count, 64), dtype=np.uint8))
    msgs = (blob, offsets)
    # the two sides agree, before anything is timed
    new_p, old_p = batch.plaintexts_from_messages(ctx, msgs), old_from_messages(ctx, blob, offsets, cf)
    same = all(np.array_equal(x, y) for x, y in zip(new_p[:4], old_p))
    E1, E2, ctr, _, st = batch.encrypt_messages(ctx, kp, msgs)
    o = old_encrypt(ctx, kp, blob, offsets, cf)
    same = same and np.array_equal(E1, o[0]) and np.array_equal(E2, o[1]) and np.array_equal(ctr, o[2]) and np.array_equal(st, o[3]) and not st.any()
    back, dst = batch.decrypt_messages(ctx, kp, E1, E2, cf, as_rows=True)
    rows, ost = old_decrypt(ctx, kp, E1, E2, cf)
    same = same and np.array_equal(back, rows) and np.array_equal(dst, ost) and not dst.any()
    rows30 = chunk_rows(blob, offsets, cf)
    at = batch.plaintexts_from_bytes_at(ctx, rows30, ctr)
    same = same and all(np.array_equal(x, y) for x, y in zip(at[:3], new_p[:3])) and not at[3].any()
    say("%d chunks as %d messages of %d bytes (%d chunks each); new and old results equal: %s" % (n, count, length, per, same))
    pair(say, "afx_plaintexts_from_messages", n, lambda: batch.plaintexts_from_messages(ctx, msgs), lambda: old_from_messages(ctx, blob, offsets, cf), reps)
    pair(say, "afx_encrypt_messages", n, lambda: batch.encrypt_messages(ctx, kp, msgs), lambda: old_encrypt(ctx, kp, blob, offsets, cf), reps)
    pair(say, "afx_decrypt_messages", n, lambda: batch.decrypt_messages(ctx, kp, E1, E2, cf, as_rows=True), lambda: old_decrypt(ctx, kp, E1, E2, cf), reps)
    pair(say, "afx_plaintexts_from_bytes_at", n, lambda: batch.plaintexts_from_bytes_at(ctx, rows30, ctr), lambda: batch.plaintexts_from_bytes(ctx, rows30), reps)
    say("  mean counter of the messages: %.2f (the search tries that many candidates and one more; a wave waits for its slowest lane)" % float(ctr.mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunks", default="65536,1048576")
    ap.add_argument("--lengths", default="30,200,3000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    params, key, ip = bench.load_fixture("readme_4attrs_sSPe")
    ctx = afx.Context(params, None, ip)
    say("whole-message calls against the composition of existing calls they replace, one MI355X, one process, legs alternating,")
    say("host-pointer forms (numpy arrays in and out), host clock around synchronous calls; medians of %d after one discarded leg" % args.reps)
    sizes = [(int(c), int(l)) for c in args.chunks.split(",") for l in args.lengths.split(",")]
    # the first configuration of a process pays for what every later one finds in place - staging buffers grown to size, pinned images,
    # first launches (seen as legs of ~30 ms among legs of 3 ms): it is run once, in full, and not reported
    run_config(lambda s: None, ctx, sizes[0][0], sizes[0][1], 1)
    say("(the first configuration was run once, unreported, to warm the process)")
    for n_chunks, length in sizes:
        run_config(say, ctx, n_chunks, length, args.reps)
    ctx.close()


if __name__ == "__main__":
    main()
