#!/usr/bin/env python3
"""What a patch session step costs against the one-shot patch step and against
a re-put session step.

patch_cost.py's cluster and shapes: 256 single-shard objects of 1 MiB in one
HBM pool, 64 KiB patched per object, all on GPU 0, one process. Three key
sets, one per contender, and a GpuClient of its own for the re-put session (a
patch erases its keys from its client's placement cache, and any erasure ends
the put sessions bound to that cache):
  one-shot patch:  batch_patch_device — BATCH_PATCH_START, planning, one
                   upload, fused_patch launch, BATCH_PUT_COMPLETE;
  session patch:   batch_patch_prepared after its first call —
                   BATCH_PATCH_START_TOKEN, one FusedPatchPlan replay,
                   BATCH_COMMIT_TOKEN_SHARDS;
  re-put session:  batch_put_prepared(replace=True) after its first call —
                   BATCH_UPSERT_START, one FusedPutPlan replay,
                   BATCH_COMMIT_TOKEN.
and the bare launches over the same shapes, no RPC: gpu.fused_patch and one
replay of a gpu.fused_patch_plan. All five alternate, one of each per
repetition: the plan's before_step hook runs the other four, so a replay is
timed from the hook's return to its next entry (which adds the binding's two
result vectors to it). Every other step is timed by the host clock around a
call that returns only after its stream has drained and its commit was
answered. Prints medians and p10/p90 as one JSON line. Needs a GPU; there is
no fallback.

  python scripts/patch_session_cost.py [--objects 256] [--size-mib 1]
                                       [--patch-kib 64]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import blackbird_amd as bb  # noqa: E402
from patch_cost import _cluster, _stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--size-mib", type=int, default=1)
    ap.add_argument("--patch-kib", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()

    g = bb.core.gpu
    if not g.available():
        raise SystemExit("patch_session_cost.py needs a GPU")
    n, size, plen = args.objects, args.size_mib << 20, args.patch_kib << 10
    poff = size // 4  # tile-aligned, inside the object
    assert poff % 1024 == 0 and plen % 1024 == 0 and poff + plen <= size

    srv, c, stop = _cluster(4 * n * size)
    svc = srv.service()
    gcl = bb.GpuClient(c, 0)
    gcl.init()
    putter = bb.GpuClient(c, 0)
    putter.init()
    putter.set_placement_cache(True)  # put sessions bind to it
    src, new = g.malloc(n * size), g.malloc(n * plen)
    dst, dst2 = g.malloc(n * size), g.malloc(n * size)
    g.fill_pattern(src, n * size, seed=23)
    g.fill_pattern(new, n * plen, seed=29)
    cfg = bb.PlacementConfig()
    cfg.replace = True

    def keyset(prefix):
        keys = ["%s%d" % (prefix, i) for i in range(n)]
        puts = [(k, src + i * size, size) for i, k in enumerate(keys)]
        assert gcl.batch_put_device(puts, cfg) == [0] * n
        return keys, puts, [(k, poff, new + i * plen, plen)
                            for i, k in enumerate(keys)]

    keys_a, _, patches_a = keyset("oa")
    keys_b, _, patches_b = keyset("sb")
    keys_c, puts_c, _ = keyset("rc")
    patch_batch = bb.core.make_patch_batch(patches_b)
    put_batch = bb.core.make_put_batch(puts_c)

    def one_shot():
        assert gcl.batch_patch_device(patches_a) == [0] * n

    def session_patch():
        assert gcl.batch_patch_prepared(patch_batch) == [0] * n

    def session_reput():
        assert putter.batch_put_prepared(put_batch, cfg)

    # both patch steps must leave what a put of the patched bytes leaves, and
    # the session steps must be session steps — or the timing compares nothing
    one_shot()
    session_patch()          # establishes
    assert patch_batch.active and gcl.session_patch_steps == 0
    session_patch()
    session_patch()
    assert gcl.session_patch_steps == 2 and gcl.patched_rewrite_items == 0
    session_reput()          # establishes
    session_reput()
    assert putter.session_put_steps == 1
    def want_of(i):  # object i of every key set after any number of patches
        blob = g.download(src + i * size, size)
        return blob[:poff] + g.download(new + i * plen, plen) + blob[poff + plen:]

    probes = sorted({0, n - 1})
    want = {i: want_of(i) for i in probes}
    want_digest = {i: g.checksum_cpu(w) for i, w in want.items()}
    for keys in (keys_a, keys_b):
        assert gcl.batch_get_device(
            [(k, dst + i * size, size) for i, k in enumerate(keys)],
            verify=True) == [0] * n
        for i in probes:
            assert g.download(dst + i * size, size) == want[i]
            assert svc.get_workers(keys[i]).checksum == want_digest[i]
    assert svc.run_scrub_once() == 0

    # the launches alone, same shapes, plain allocations
    digests = g.fused_put([(src + i * size, dst + i * size, size)
                           for i in range(n)])
    assert g.fused_put([(src + i * size, dst2 + i * size, size)
                        for i in range(n)]) == digests
    sizes = [size] * n

    def runs_into(base):
        return [(new + i * plen, base + i * size + poff, plen, poff // 1024,
                 poff // 1024, i, i) for i in range(n)]

    runs = runs_into(dst)
    launch_digests = [digests]

    def k_patch():  # same bytes every time: the first call's outputs stand
        out = g.fused_patch(runs, sizes, launch_digests[0], sizes,
                            launch_digests[0])
        launch_digests[0] = out[0]

    k_patch()
    for i in probes:
        assert launch_digests[0][i] == want_digest[i]

    steps = {"patch_step": one_shot, "session_patch_step": session_patch,
             "reput_session_step": session_reput, "fused_patch_launch": k_patch}
    times = {name: [] for name in steps}
    times["fused_patch_plan_replay"] = []
    graph0 = gcl.session_graph_steps + putter.session_graph_steps
    patch0, put0 = gcl.session_patch_steps, putter.session_put_steps
    total = args.warmup + args.reps
    mark = [None]

    def before(k):
        now = time.perf_counter()
        if k > args.warmup:  # replay k-1 ran between the hook's calls
            times["fused_patch_plan_replay"].append(now - mark[0])
        if k < total:
            for name, fn in steps.items():
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if k >= args.warmup:
                    times[name].append(dt)
        mark[0] = time.perf_counter()

    # total + 1 replays: the hook of the last one only closes replay total-1
    replays = g.fused_patch_plan(runs_into(dst2), sizes, sizes, digests,
                                 digests, total + 1, before_step=before)
    for i in probes:
        assert replays[0][0][i] == replays[0][1][i] == want_digest[i]
    assert replays[-1] == replays[0]
    assert gcl.session_patch_steps == patch0 + total
    assert putter.session_put_steps == put0 + total
    graphs = gcl.session_graph_steps + putter.session_graph_steps - graph0

    for p in (src, new, dst, dst2):
        g.free(p)
    stop()

    out = {"objects": n, "object_bytes": size, "patch_bytes": plen,
           "patch_offset": poff, "reps": args.reps,
           "session_steps_on_graph": graphs == 2 * total}
    for name, ts in times.items():
        assert len(ts) == args.reps, name
        _stats(out, name, ts)
    out["session_patch_below_patch_p10"] = (
        out["session_patch_step_median_us"] < out["patch_step_p10_us"])
    out["session_patch_below_reput_session_p10"] = (
        out["session_patch_step_median_us"] < out["reput_session_step_p10_us"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
