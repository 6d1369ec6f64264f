#!/usr/bin/env python3
"""What an in-place range patch costs against re-putting the whole object.

256 single-shard objects of 1 MiB in one HBM pool, all on GPU 0, one process
(coordination, keystone, worker and client embedded):
  re-put: batch_put_device(replace=True) over the same keys — the only way to
          change part of an object before the ranged calls (BATCH_PUT_START,
          one fused copy+digest launch over 2 x 1 MiB per object,
          BATCH_PUT_COMPLETE);
  patch:  batch_patch_device of 64 KiB per object (BATCH_PATCH_START, one
          fused_patch launch over 3 x 64 KiB per object, BATCH_PUT_COMPLETE).
The two alternate; each step is timed by the host clock around a call that
returns only after its stream has drained and its commit was answered. The
launches alone (gpu.fused_patch against gpu.fused_put over the same shapes,
no RPC) are timed the same way. Prints medians and p10/p90 as one JSON line.
Needs a GPU; there is no fallback.

  python scripts/patch_cost.py [--objects 256] [--size-mib 1] [--patch-kib 64]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import blackbird_amd as bb  # noqa: E402


def _cluster(pool_bytes):
    cs = bb.CoordServer()
    cs.start("127.0.0.1", 0)
    ep = "127.0.0.1:%d" % cs.port
    kc = bb.KeystoneConfig()
    kc.listen_address = "127.0.0.1:0"
    kc.coord_endpoint = ep
    srv = bb.create_and_start_keystone(kc)
    wc = bb.WorkerConfig()
    wc.worker_id = "cost-w0"
    wc.coord_endpoint = ep
    wc.data_listen_address = "127.0.0.1:0"
    p = bb.PoolConfig()
    p.pool_id = "hbm0"
    p.storage_class = bb.StorageClass.RAM_GPU
    p.size_bytes = pool_bytes
    p.gpu_device_id = 0
    wc.pools = [p]
    w = bb.WorkerService(wc)
    w.initialize()
    w.start()
    deadline = time.time() + 5
    while time.time() < deadline and not srv.service().get_memory_pools():
        time.sleep(0.05)
    o = bb.ClientOptions()
    o.keystone_endpoint = srv.endpoint
    c = bb.Client(o)
    c.connect()

    def stop():
        c.close()
        w.stop()
        srv.stop()
        srv.service().stop()
        cs.stop()
    return srv, c, stop


def _stats(out, name, ts):
    ts = sorted(ts)
    out[name + "_median_us"] = round(statistics.median(ts) * 1e6, 1)
    out[name + "_p10_us"] = round(ts[len(ts) // 10] * 1e6, 1)
    out[name + "_p90_us"] = round(ts[len(ts) * 9 // 10] * 1e6, 1)


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
        raise SystemExit("patch_cost.py needs a GPU")
    n, size, plen = args.objects, args.size_mib << 20, args.patch_kib << 10
    poff = size // 4  # tile-aligned, inside the object
    assert poff % 1024 == 0 and plen % 1024 == 0 and poff + plen <= size

    srv, c, stop = _cluster(2 * n * size)
    gcl = bb.GpuClient(c, 0)
    gcl.init()
    src, new, dst = g.malloc(n * size), g.malloc(n * plen), g.malloc(n * size)
    g.fill_pattern(src, n * size, seed=23)
    g.fill_pattern(new, n * plen, seed=29)
    keys = ["pc%d" % i for i in range(n)]
    cfg = bb.PlacementConfig()
    cfg.replace = True
    puts = [(k, src + i * size, size) for i, k in enumerate(keys)]
    patches = [(k, poff, new + i * plen, plen) for i, k in enumerate(keys)]

    def reput():
        assert gcl.batch_put_device(puts, cfg) == [0] * n

    def patch():
        assert gcl.batch_patch_device(patches) == [0] * n

    # the patch step must leave what a put of the patched bytes leaves — or
    # the timing compares nothing
    reput()
    patch()
    assert gcl.patched_fused_items == n and gcl.patched_rewrite_items == 0
    assert gcl.batch_get_device(
        [(k, dst + i * size, size) for i, k in enumerate(keys)],
        verify=True) == [0] * n
    host_src = g.download(src, size)
    want = host_src[:poff] + g.download(new, plen) + host_src[poff + plen:]
    assert g.download(dst, size) == want
    assert srv.service().get_workers(keys[0]).checksum == g.checksum_cpu(want)

    times = {"reput_step": [], "patch_step": []}
    for rep in range(args.warmup + args.reps):
        for name, fn in (("reput_step", reput), ("patch_step", patch)):
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if rep >= args.warmup:
                times[name].append(dt)

    # the launches alone, same shapes, plain allocations
    digests = g.fused_put([(src + i * size, dst + i * size, size)
                           for i in range(n)])
    put_descs = [(src + i * size, dst + i * size, size) for i in range(n)]
    runs = [(new + i * plen, dst + i * size + poff, plen, poff // 1024,
             poff // 1024, i, i) for i in range(n)]
    sizes = [size] * n

    def k_put():
        g.fused_put(put_descs)

    def k_patch():  # follows k_put: dst holds src's bytes, `digests` are theirs
        g.fused_patch(runs, sizes, digests, sizes, digests)

    for rep in range(args.warmup + args.reps):
        for name, fn in (("fused_put_launch", k_put),
                         ("fused_patch_launch", k_patch)):
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if rep >= args.warmup:
                times.setdefault(name, []).append(dt)

    for p in (src, new, dst):
        g.free(p)
    stop()

    out = {"objects": n, "object_bytes": size, "patch_bytes": plen,
           "patch_offset": poff, "reps": args.reps}
    for name, ts in times.items():
        _stats(out, name, ts)
    out["patch_step_below_reput_p10"] = (
        out["patch_step_median_us"] < out["reput_step_p10_us"])
    out["model_bytes_moved_patch"] = 3 * plen * n
    out["model_bytes_moved_reput"] = 2 * size * n
    print(json.dumps(out))


if __name__ == "__main__":
    main()
