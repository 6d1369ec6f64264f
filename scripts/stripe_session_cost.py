#!/usr/bin/env python3
"""What a striped batch session step costs against the paths beside it.

One process, one keystone, two RAM_GPU workers on GPU 0; 256 objects of
1 MiB, two shards each; the same source bytes on every path. Alternating in
the same run, for puts and for verified gets:
  one_shot     the striped batch_put_device / batch_get_device without a
               session, from a client whose placement cache is off: the whole
               cold path every step (BATCH_PUT_START with every key, per-object
               placement decoding, one fused_stripe launch,
               BATCH_PUT_COMPLETE with every key; BATCH_GET_WORKERS for gets);
  striped      the striped session step via batch_put_prepared /
               batch_get_prepared (cache on): two tiny RPCs around one captured
               graph launch; zero RPCs for a get;
  single       the single-shard session step over the same bytes
               (max_workers_per_copy = 1), the yardstick.
Every shape is warmed; each call is timed by the host clock around an entry
point that returns only after its stream has drained. Before timing, one_shot
and striped must leave identical digests at the keystone. Prints medians and
p10/p90 as one JSON line. Needs a GPU; there is no fallback.

  python scripts/stripe_session_cost.py [--objects 256] [--size-mib 1] [--reps 50]
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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()

    g = bb.core.gpu
    if not g.available():
        raise SystemExit("stripe_session_cost.py needs a GPU")
    n, size = args.objects, args.size_mib << 20

    cs = bb.CoordServer()
    cs.start("127.0.0.1", 0)
    ep = "127.0.0.1:%d" % cs.port
    kc = bb.KeystoneConfig()
    kc.listen_address = "127.0.0.1:0"
    kc.coord_endpoint = ep
    srv = bb.create_and_start_keystone(kc)
    ks = srv.service()
    workers = []
    for i in range(2):
        wc = bb.WorkerConfig()
        wc.worker_id = "w%d" % i
        wc.coord_endpoint = ep
        wc.data_listen_address = "127.0.0.1:0"
        p = bb.PoolConfig()
        p.pool_id = "hbm%d" % i
        p.storage_class = bb.StorageClass.RAM_GPU
        # three key sets of n objects, and room to spare
        p.size_bytes = 2 * n * size + (64 << 20)
        p.gpu_device_id = 0
        wc.pools = [p]
        w = bb.WorkerService(wc)
        w.initialize()
        w.start()
        workers.append(w)
    deadline = time.time() + 5
    while time.time() < deadline and len(ks.get_memory_pools()) < 2:
        time.sleep(0.05)

    o = bb.ClientOptions()
    o.keystone_endpoint = srv.endpoint
    c = bb.Client(o)
    c.connect()
    cold = bb.GpuClient(c, 0)   # cache off: no sessions, no cached gets
    cold.init()
    warm = bb.GpuClient(c, 0)
    warm.init()
    warm.set_placement_cache(True)

    src, dst = g.malloc(n * size), g.malloc(n * size)
    g.fill_pattern(src, n * size, seed=17)

    striped = bb.PlacementConfig()
    striped.max_workers_per_copy = 2
    striped.replace = True
    striped.checksum = True
    single = bb.PlacementConfig()
    single.replace = True
    single.checksum = True

    def puts(prefix):
        return [("%s%04d" % (prefix, i), src + i * size, size) for i in range(n)]

    def gets(prefix):
        return [("%s%04d" % (prefix, i), dst + i * size, size) for i in range(n)]

    a_put, a_get = puts("a"), gets("a")
    b_put, b_get = bb.make_put_batch(puts("b")), bb.make_get_batch(gets("b"))
    c_put, c_get = bb.make_put_batch(puts("c")), bb.make_get_batch(gets("c"))

    def ok(statuses):
        assert statuses == [0] * n, [s for s in statuses if s][:4]

    def must(done):
        assert done

    put_fns = {
        "one_shot": lambda: ok(cold.batch_put_device(a_put, striped)),
        "striped": lambda: must(warm.batch_put_prepared(b_put, striped)),
        "single": lambda: must(warm.batch_put_prepared(c_put, single)),
    }
    get_fns = {
        "one_shot": lambda: ok(cold.batch_get_device(a_get, verify=True)),
        "striped": lambda: must(warm.batch_get_prepared(b_get, True)),
        "single": lambda: must(warm.batch_get_prepared(c_get, True)),
    }

    # establish every session, then one step of each on it
    for _ in range(2):
        for fn in list(put_fns.values()) + list(get_fns.values()):
            fn()
    # same answers at the keystone — or the timing compares nothing
    for i in range(n):
        a, b = ks.get_workers("a%04d" % i), ks.get_workers("b%04d" % i)
        assert a.checksum == b.checksum != 0, i
        da = [s.digest for s in a.copies[0].shards]
        db = [s.digest for s in b.copies[0].shards]
        assert len(da) == 2 and da == db, i
    assert g.verify_pattern(dst, n * size, seed=17) == 0

    before = (warm.session_put_steps, warm.session_get_steps,
              warm.session_graph_steps)
    times = {k + "_put": [] for k in put_fns}
    times.update({k + "_get": [] for k in get_fns})
    for rep in range(args.warmup + args.reps):
        for kind, fns in (("_put", put_fns), ("_get", get_fns)):
            for name, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if rep >= args.warmup:
                    times[name + kind].append(dt)
    total = args.warmup + args.reps
    # every timed striped and single step was a session step on the graph
    assert warm.session_put_steps - before[0] == 2 * total
    assert warm.session_get_steps - before[1] == 2 * total
    graph = warm.session_graph_steps - before[2]
    assert cold.session_put_steps == 0 and cold.session_get_steps == 0

    out = {"objects": n, "object_bytes": size, "shards": 2, "reps": args.reps,
           "graph_steps": graph, "session_steps": 4 * total}
    for name, ts in times.items():
        ts.sort()
        out[name + "_median_us"] = round(statistics.median(ts) * 1e6, 1)
        out[name + "_p10_us"] = round(ts[len(ts) // 10] * 1e6, 1)
        out[name + "_p90_us"] = round(ts[len(ts) * 9 // 10] * 1e6, 1)
    for kind in ("put", "get"):
        a = "one_shot_" + kind
        out[kind + "_saved_us"] = round(
            out[a + "_median_us"] - out["striped_%s_median_us" % kind], 1)
        out[kind + "_one_shot_spread_us"] = round(
            out[a + "_p90_us"] - out[a + "_p10_us"], 1)
    print(json.dumps(out))

    g.free(src)
    g.free(dst)
    c.close()
    for w in workers:
        w.stop()
    srv.stop()
    ks.stop()
    cs.stop()


if __name__ == "__main__":
    main()
