#!/usr/bin/env python3
"""What one fused_stripe launch costs against the three passes it replaces.

256 objects of 1 MiB, two 512 KiB shards each, all on GPU 0:
  three passes: batched_copy of the shards, checksum_batch over the objects,
                checksum_batch over the shards (the striped put route before
                fused_stripe);
  fused:        one fused_stripe launch (copy + shard digests + object
                digests from a single read).
Both run in this process, alternating, each call timed by the host clock
around an entry point that returns only after its stream has drained.
Prints the medians as one JSON line. Needs a GPU; there is no fallback.

  python scripts/stripe_cost.py [--objects 256] [--size-mib 1] [--reps 50]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import blackbird_amd as bb  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--size-mib", type=int, default=1)
    ap.add_argument("--shards", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()

    g = bb.core.gpu
    if not g.available():
        raise SystemExit("stripe_cost.py needs a GPU")
    n, size = args.objects, args.size_mib << 20
    plan = g.plan_stripe(size, [size // args.shards] * args.shards)
    if plan is None:
        raise SystemExit("shards do not start on tile boundaries")

    src, dst = g.malloc(n * size), g.malloc(n * size)
    g.fill_pattern(src, n * size, seed=17)
    objs = [(src + i * size, size) for i in range(n)]
    segs = [(src + i * size + off, dst + i * size + off, nb, ft, i)
            for i in range(n) for off, nb, ft in plan]
    copies = [(s, d, nb) for s, d, nb, _, _ in segs]
    shards = [(s, nb) for s, _, nb, _, _ in segs]

    def three_passes():
        g.batched_copy(copies)
        obj = g.checksum_device_batch(objs)
        seg = g.checksum_device_batch(shards)
        return seg, obj

    def fused():
        return g.fused_stripe(segs, [size] * n)

    # same answers, same bytes moved — or the timing compares nothing
    want = three_passes()
    got = fused()
    assert (list(got[0]), list(got[1])) == (list(want[0]), list(want[1]))
    assert g.verify_pattern(dst, n * size, seed=17) == 0

    times = {"three_passes": [], "fused_stripe": []}
    for rep in range(args.warmup + args.reps):
        for name, fn in (("three_passes", three_passes), ("fused_stripe", fused)):
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if rep >= args.warmup:
                times[name].append(dt)
    g.free(src)
    g.free(dst)

    out = {"objects": n, "object_bytes": size, "shards": args.shards,
           "reps": args.reps}
    for name, ts in times.items():
        ts.sort()
        out[name + "_median_us"] = round(statistics.median(ts) * 1e6, 1)
        out[name + "_p10_us"] = round(ts[len(ts) // 10] * 1e6, 1)
        out[name + "_p90_us"] = round(ts[len(ts) * 9 // 10] * 1e6, 1)
    out["payload_gb_per_s_fused"] = round(
        n * size / statistics.median(times["fused_stripe"]) / 1e9, 1)
    out["payload_gb_per_s_three_passes"] = round(
        n * size / statistics.median(times["three_passes"]) / 1e9, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
