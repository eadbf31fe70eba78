"""The spent-tag set on one GPU (include/aeonflux_gpu.h "The spent-tag set"): afx_tagset_spend_dev on fresh tags and on their replay, and
afx_tagset_contains_dev.

In ONE process, device-resident, `--reps` rounds (5) after one discarded round; a round makes an empty set of capacity 2 * count, then
times, with device events around the whole call on the context's stream,
    spend_dev on `count` distinct random tags (all fresh: every item claims a slot and writes its key),
    spend_dev on the same tags again (all spent: probes and comparisons with kept keys, nothing written but the answers),
    contains_dev on them.
The answers are checked in every round.  There is no target: the figure to hold them against is the tagged verification the calls
follow, 2.6 M presentations/s on C3's layout (profiles/tagged_rate.txt).
    python tools/tagset_rate.py [--reps R] [--sizes 65536,1048576] [--out profiles/tagset_rate.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aeonflux_amd as afx  # noqa: E402
import bench  # noqa: E402
from aeonflux_amd import batch  # noqa: E402


def leg(say, torch, ctx, count, reps):
    dev = torch.device("cuda", 0)
    ext = torch.cuda.ExternalStream(ctx.stream)
    tags = torch.from_numpy(np.random.default_rng(count).integers(0, 256, size=(count, 32), dtype=np.uint8)).to(dev)
    seen = torch.full((count,), 255, dtype=torch.uint8, device=dev)
    times = {"spend_dev, fresh": [], "spend_dev, replay": [], "contains_dev": []}
    ok = True

    def timed(name, f, want):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ext)
        f()
        e1.record(ext)
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1))
        return bool((seen == want).all().item())
    for r in range(reps + 1):
        ts = batch.TagSet(ctx, 2 * count)
        ok &= timed("spend_dev, fresh", lambda: ts.spend_dev(tags, None, count, seen), batch.TAG_FRESH)
        ok &= ts.size() == (count, 2 * count)
        ok &= timed("spend_dev, replay", lambda: ts.spend_dev(tags, None, count, seen), batch.TAG_SPENT)
        ok &= timed("contains_dev", lambda: ts.contains_dev(tags, count, seen), 1)
        ok &= ts.size() == (count, 2 * count)
        ts.close()
    say("%d tags device-resident, capacity %d (%d slots, %.0f MB); every answer as expected: %s" %
        (count, 2 * count, 4 * count, 40 * 4 * count / 1e6, ok))
    for k, t in times.items():
        t = t[1:]
        med = statistics.median(t)
        say("  %-18s median %8.3f ms  %8.1f M tags/s  (runs: %s)" % (k, med, count / med / 1e3, " ".join("%.3f" % x for x in t)))


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
    params, key, ip = bench.load_fixture("readme_4attrs_sSPe")
    ctx = afx.Context(params, None, ip)
    say("the spent-tag set, one MI355X, one process, a fresh set per round, random salt")
    for count in (int(x) for x in args.sizes.split(",")):
        leg(say, torch, ctx, count, args.reps)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
