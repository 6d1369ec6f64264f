#!/usr/bin/env python3
"""What an in-place patch of a range that is not whole tiles costs, against the
rewrite route it replaces and against the tile-aligned session step.

patch_cost.py's cluster and shapes: 256 single-shard objects of 1 MiB in one
HBM pool, 64 KiB patched per object, all on GPU 0, one process. The unaligned
range starts at offset 1000 (a head edge of 24 bytes, 63 whole tiles, a tail
edge of 1000 bytes; the source in phase with the offset), the aligned one at
1024. One key set per contender, two GpuClients:
  edge one-shot:    batch_patch_device, set_patch_edge_tiles(True) — one
                    launch of runs and edges;
  rewrite one-shot: the same call with the option off — per item a verified
                    get, an overlay and a put, in a serial loop;
  edge session:     batch_patch_prepared after its first call, option on,
                    offset 1000 — one replay of runs and edges;
  aligned session:  the same at offset 1024 — one replay of runs alone.
These four alternate, one of each per repetition, each timed by the host
clock around a call that returns only after its stream has drained and its
commit was answered.

And the bare replays over the same shapes, no RPC, gpu.fused_patch_plan: the
runs alone, the runs with their edges, the edges alone. A plan without a tile
and without an edge is refused, so there is no emptier replay to compare
with: what the edge kernel's node adds to a step is read as the median of
runs-with-edges less the median of runs-alone. One plan is replayed at a
time (a replay is timed from its before_step hook's return to the hook's
next entry, which adds the binding's two result vectors to it), so these
three do not alternate step by step: they run in blocks of reps/2 replays,
runs / both / edges, twice over, in the same process right behind the loop
above. The one-shot gpu.fused_patch is not used for this: its binding
converts 512 edge tuples per call, which costs more than the kernel.

Prints medians and p10/p90 as one JSON line. Needs a GPU; there is no
fallback.

  python scripts/patch_edges_cost.py [--objects 256] [--size-mib 1]
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

UNALIGNED, ALIGNED = 1000, 1024


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
        raise SystemExit("patch_edges_cost.py needs a GPU")
    n, size, plen = args.objects, args.size_mib << 20, args.patch_kib << 10
    assert plen % 1024 == 0 and ALIGNED + plen <= size
    phase = UNALIGNED % 16
    stride = plen + 16

    srv, c, stop = _cluster(6 * n * size)
    svc = srv.service()
    on, off = bb.GpuClient(c, 0), bb.GpuClient(c, 0)
    on.init()
    off.init()
    on.set_patch_edge_tiles(True)
    src, new = g.malloc(n * size), g.malloc(n * stride)
    dst = g.malloc(n * size)
    g.fill_pattern(src, n * size, seed=23)
    g.fill_pattern(new, n * stride, seed=29)
    cfg = bb.PlacementConfig()
    cfg.replace = True

    def keyset(prefix, poff):
        keys = ["%s%d" % (prefix, i) for i in range(n)]
        assert on.batch_put_device(
            [(k, src + i * size, size) for i, k in enumerate(keys)],
            cfg) == [0] * n
        at = phase if poff == UNALIGNED else 0
        return keys, [(k, poff, new + i * stride + at, plen)
                      for i, k in enumerate(keys)]

    keys_a, patches_a = keyset("ea", UNALIGNED)
    keys_b, patches_b = keyset("rb", UNALIGNED)
    keys_c, patches_c = keyset("sc", UNALIGNED)
    keys_d, patches_d = keyset("sd", ALIGNED)
    batch_c = bb.core.make_patch_batch(patches_c)
    batch_d = bb.core.make_patch_batch(patches_d)

    def edge_one_shot():
        assert on.batch_patch_device(patches_a) == [0] * n

    def rewrite_one_shot():
        assert off.batch_patch_device(patches_b) == [0] * n

    def edge_session():
        assert on.batch_patch_prepared(batch_c) == [0] * n

    def aligned_session():
        assert on.batch_patch_prepared(batch_d) == [0] * n

    # every step must leave what a put of the patched bytes leaves, and take
    # the route it is named after — or the timing compares nothing
    edge_one_shot()
    assert on.patched_fused_items == n and on.patched_rewrite_items == 0
    rewrite_one_shot()
    assert off.patched_fused_items == 0 and off.patched_rewrite_items == n
    for step, batch in ((edge_session, batch_c), (aligned_session, batch_d)):
        before = on.session_patch_steps
        step()  # establishes
        assert batch.active and on.session_patch_steps == before
        step()
        assert on.session_patch_steps == before + 1
    assert on.patched_rewrite_items == 0

    probes = sorted({0, n - 1})

    def want_of(i, poff):
        blob = g.download(src + i * size, size)
        at = phase if poff == UNALIGNED else 0
        return (blob[:poff] + g.download(new + i * stride + at, plen) +
                blob[poff + plen:])

    for keys, poff in ((keys_a, UNALIGNED), (keys_b, UNALIGNED),
                       (keys_c, UNALIGNED), (keys_d, ALIGNED)):
        assert on.batch_get_device(
            [(k, dst + i * size, size) for i, k in enumerate(keys)],
            verify=True) == [0] * n
        for i in probes:
            w = want_of(i, poff)
            assert g.download(dst + i * size, size) == w
            assert svc.get_workers(keys[i]).checksum == g.checksum_cpu(w)
    assert svc.run_scrub_once() == 0

    # the launches alone, same shapes, into a plain allocation
    digests = g.fused_put([(src + i * size, dst + i * size, size)
                           for i in range(n)])
    sizes = [size] * n
    head = 1024 - UNALIGNED             # bytes of the head edge
    tail = (UNALIGNED + plen) % 1024    # bytes of the tail edge
    inner = plen - head - tail
    last = (UNALIGNED + plen) // 1024   # the tail edge's tile
    runs, edges = [], []
    for i in range(n):
        s, d = new + i * stride + phase, dst + i * size
        runs.append((s + head, d + 1024, inner, 1, 1, i, i))
        edges.append((s, d, UNALIGNED, 1024, 1024, 0, 0, i, i))
        edges.append((s + head + inner, d + last * 1024, 0, tail, 1024, last,
                      last, i, i))
    want_digests = {i: g.checksum_cpu(want_of(i, UNALIGNED)) for i in probes}

    steps = {"edge_patch_step": edge_one_shot,
             "rewrite_patch_step": rewrite_one_shot,
             "edge_session_step": edge_session,
             "aligned_session_step": aligned_session}
    times = {name: [] for name in steps}
    steps0, graphs0 = on.session_patch_steps, on.session_graph_steps
    total = args.warmup + args.reps
    for k in range(total):
        for name, fn in steps.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if k >= args.warmup:
                times[name].append(dt)
    assert on.session_patch_steps == steps0 + 2 * total
    assert on.patched_rewrite_items == 0
    assert off.patched_rewrite_items == n * (total + 1)
    graphs = on.session_graph_steps - graphs0
    assert svc.run_scrub_once() == 0

    # the replays alone: same bytes every time, so every step's outputs are
    # the first one's
    plans = {"replay_runs": (runs, []), "replay_runs_and_edges": (runs, edges),
             "replay_edges": ([], edges)}
    for name in plans:
        times[name] = []
    state = [digests]
    half = (args.reps + 1) // 2
    block = args.warmup + half
    for _ in range(2):
        for name, (segs, eds) in plans.items():
            mark = [None]

            def before(k, name=name):
                now = time.perf_counter()
                if k > args.warmup:  # replay k-1 ran between the hook's calls
                    times[name].append(now - mark[0])
                mark[0] = time.perf_counter()

            # block + 1 replays: the last hook only closes replay block-1
            out = g.fused_patch_plan(segs, sizes, sizes, state[0], state[0],
                                     block + 1, before_step=before, edges=eds)
            assert out[-1] == out[1]
            state[0] = out[-1][0]
    for i in probes:
        assert state[0][i] == want_digests[i]
    for name in plans:
        del times[name][args.reps:]

    for p in (src, new, dst):
        g.free(p)
    stop()

    out = {"objects": n, "object_bytes": size, "patch_bytes": plen,
           "unaligned_offset": UNALIGNED, "aligned_offset": ALIGNED,
           "edges_per_launch": len(edges), "reps": args.reps,
           "session_steps_on_graph": graphs == 2 * total}
    for name, ts in times.items():
        assert len(ts) == args.reps, name
        _stats(out, name, ts)
    extra = round(out["replay_runs_and_edges_median_us"] -
                  out["replay_runs_median_us"], 1)
    out["edge_kernel_extra_us"] = extra
    out["edge_step_below_rewrite_p10"] = (
        out["edge_patch_step_median_us"] < out["rewrite_patch_step_p10_us"])
    out["edge_session_within_aligned_band"] = (
        out["aligned_session_step_p10_us"]
        <= out["edge_session_step_median_us"]
        <= out["aligned_session_step_p90_us"] + max(extra, 0.0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
