#!/usr/bin/env python3
"""The GPU client's step counters over one fixed session scenario.

Three session forms, each on a cluster and a client of its own so every
counter starts at zero: plain (one RAM_GPU worker), replicated (replication 2
over two workers) and striped (two shards per object over two workers). Each
runs 6 steps over 4 prepared objects of 256 KiB; a step is a prepared put of
fresh bytes, a prepared get and a byte compare. Before step 4 an "intruder"
object is put and removed at the keystone, which ends the server session.
After every step the counters are recorded:

  session_put_steps, session_get_steps, session_graph_steps,
  striped_fused_items, striped_fused_get_items, ks.token_commits()

Two builds that take the same paths print the same line. Prints one JSON
line. Needs a GPU; there is no fallback.

  python scripts/gpu_client_step_counters.py
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import blackbird_amd as bb  # noqa: E402

N, SIZE, STEPS, INTRUDER_BEFORE = 4, 256 << 10, 6, 4
FORMS = {  # name: (workers, replication, max_workers_per_copy)
    "plain": (1, 1, 1),
    "replicated": (2, 2, 1),
    "striped": (2, 1, 2),
}


def run_form(g, name, n_workers, replication, shards):
    cs = bb.CoordServer()
    cs.start("127.0.0.1", 0)
    ep = "127.0.0.1:%d" % cs.port
    kc = bb.KeystoneConfig()
    kc.listen_address = "127.0.0.1:0"
    kc.coord_endpoint = ep
    srv = bb.create_and_start_keystone(kc)
    ks = srv.service()
    workers = []
    for i in range(n_workers):
        wc = bb.WorkerConfig()
        wc.worker_id = "w%d" % i
        wc.coord_endpoint = ep
        wc.data_listen_address = "127.0.0.1:0"
        p = bb.PoolConfig()
        p.pool_id = "hbm%d" % i
        p.storage_class = bb.StorageClass.RAM_GPU
        p.size_bytes = 64 << 20
        p.gpu_device_id = 0
        wc.pools = [p]
        w = bb.WorkerService(wc)
        w.initialize()
        w.start()
        workers.append(w)
    deadline = time.time() + 5
    while time.time() < deadline and len(ks.get_memory_pools()) < n_workers:
        time.sleep(0.05)

    o = bb.ClientOptions()
    o.keystone_endpoint = srv.endpoint
    c = bb.Client(o)
    c.connect()
    gcl = bb.GpuClient(c, 0)
    gcl.init()
    gcl.set_placement_cache(True)
    cfg = bb.PlacementConfig()
    cfg.replace = True
    cfg.checksum = True
    cfg.replication = replication
    cfg.max_workers_per_copy = shards

    src, dst = g.malloc(N * SIZE), g.malloc(N * SIZE)
    keys = ["%s%02d" % (name, i) for i in range(N)]
    pb = bb.make_put_batch([(k, src + i * SIZE, SIZE)
                            for i, k in enumerate(keys)])
    gb = bb.make_get_batch([(k, dst + i * SIZE, SIZE)
                            for i, k in enumerate(keys)])
    rows = []
    for step in range(1, STEPS + 1):
        if step == INTRUDER_BEFORE:
            ks.put_start("intruder", 4096, bb.PlacementConfig())
            ks.put_complete("intruder", checksum=1)
            ks.remove_object("intruder")
        blob = os.urandom(N * SIZE)
        g.upload(src, blob)
        assert gcl.batch_put_prepared(pb, cfg), (name, step)
        assert gcl.batch_get_prepared(gb), (name, step)
        assert g.download(dst, N * SIZE) == blob, (name, step)
        rows.append({
            "step": step,
            "session_put_steps": gcl.session_put_steps,
            "session_get_steps": gcl.session_get_steps,
            "session_graph_steps": gcl.session_graph_steps,
            "striped_fused_items": gcl.striped_fused_items,
            "striped_fused_get_items": gcl.striped_fused_get_items,
            "token_commits": ks.token_commits(),
        })
    g.free(src)
    g.free(dst)
    c.close()
    for w in workers:
        w.stop()
    srv.stop()
    ks.stop()
    cs.stop()
    return rows


def main():
    g = bb.core.gpu
    if not g.available():
        raise SystemExit("gpu_client_step_counters.py needs a GPU")
    print(json.dumps({name: run_form(g, name, *form)
                      for name, form in FORMS.items()}))


if __name__ == "__main__":
    main()
