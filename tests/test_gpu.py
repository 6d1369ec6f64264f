"""MI355X GPU tests: MFMA fragment-layout probe, bbhash64 kernel vs the CPU
reference (bit-exact), batched scatter/gather copy, HBM backend, and the full
HBM-tier cluster path (BASELINE config #2)."""
import os
import time

import numpy as np
import pytest

import blackbird_amd as bb

from conftest import Cluster

pytestmark = pytest.mark.gpu

MB = 1 << 20
gpu = None  # bound lazily so collection works without GPU


def setup_module():
    global gpu
    gpu = bb.core.gpu


class TestMfmaLayout:
    def test_probe_matches_cpu_matmul(self):
        rng = np.random.default_rng(7)
        # asymmetric matrices (guide: symmetric B can hide transposed layouts)
        a = rng.integers(-128, 128, size=(32, 32), dtype=np.int8)
        b = rng.integers(-128, 128, size=(32, 32), dtype=np.int8)
        want = (a.astype(np.int32) @ b.astype(np.int32)).reshape(-1)
        got = np.array(gpu.mfma_i8_probe(a.tobytes(), b.tobytes()), dtype=np.int32)
        mism = np.nonzero(got != want)[0]
        assert mism.size == 0, f"{mism.size} mismatches, first at {mism[:8]}"

    def test_probe_identity(self):
        a = np.eye(32, dtype=np.int8)
        rng = np.random.default_rng(8)
        b = rng.integers(-128, 128, size=(32, 32), dtype=np.int8)
        got = np.array(gpu.mfma_i8_probe(a.tobytes(), b.tobytes()), dtype=np.int32)
        assert (got.reshape(32, 32) == b.astype(np.int32)).all()


class TestChecksumKernel:
    @pytest.mark.parametrize("size", [1024, 4096, 1 * MB, 1 * MB + 17, 777,
                                      16 * MB])
    def test_matches_cpu_bitexact(self, size):
        data = np.random.default_rng(size).integers(
            0, 256, size=size, dtype=np.uint8).tobytes()
        ptr = gpu.malloc(max(size, 1024))
        try:
            gpu.upload(ptr, data)
            got = gpu.checksum_device(ptr, size)
            want = gpu.checksum_cpu(data)
            assert got == want, f"size={size}: gpu={got:#x} cpu={want:#x}"
        finally:
            gpu.free(ptr)

    def test_batch_matches_cpu(self):
        rng = np.random.default_rng(42)
        sizes = [1024, 65536, 1 * MB, 3333, 100 * 1024]
        ptrs, blobs = [], []
        try:
            for s in sizes:
                blob = rng.integers(0, 256, size=s, dtype=np.uint8).tobytes()
                p = gpu.malloc(s)
                gpu.upload(p, blob)
                ptrs.append(p)
                blobs.append(blob)
            got = gpu.checksum_device_batch(list(zip(ptrs, sizes)))
            want = [gpu.checksum_cpu(b) for b in blobs]
            assert got == want
        finally:
            for p in ptrs:
                gpu.free(p)

    def test_detects_corruption(self):
        data = bytes(1 * MB)
        ptr = gpu.malloc(1 * MB)
        try:
            gpu.upload(ptr, data)
            h0 = gpu.checksum_device(ptr, 1 * MB)
            gpu.upload(ptr + 512 * 1024, b"\x01")
            assert gpu.checksum_device(ptr, 1 * MB) != h0
        finally:
            gpu.free(ptr)


class _PutCase:
    """One size list laid out for the fused-put tests: every object at a
    16-byte-aligned offset of one allocation with a 16-byte gap after it.
    Source gaps hold 0x5A, the destination is pre-filled with 0xA5, so a
    store past an object's end shows up in `dst_image`. Built once per size
    list (CPU digests included) and shared, read-only, by all entry points."""
    PAD = 0xA5

    def __init__(self, sizes):
        rng = np.random.default_rng(1000003 * len(sizes) + sum(sizes))
        self.sizes = list(sizes)
        self.offs = []
        off = 0
        for s in sizes:
            self.offs.append(off)
            off += (s + 15) // 16 * 16 + 16
        self.span = off
        self.blobs = [rng.integers(0, 256, size=s, dtype=np.uint8).tobytes()
                      for s in sizes]
        self.want = [gpu.checksum_cpu(b) for b in self.blobs]
        src = bytearray(b"\x5a" * self.span)
        dst = bytearray(bytes([self.PAD]) * self.span)
        for o, b in zip(self.offs, self.blobs):
            src[o:o + len(b)] = b
            dst[o:o + len(b)] = b
        self.src_image = bytes(src)
        self.dst_image = bytes(dst)


_put_cases = {}


def _put_case(sizes):
    key = tuple(sizes)
    if key not in _put_cases:
        _put_cases[key] = _PutCase(sizes)
    return _put_cases[key]


# name -> size list; what each exercises is spelled out next to it
PUT_SIZE_LISTS = {
    # one guarded tile, and nothing else for the grid to do
    "one_byte": [1],
    # one full tile, no tail, and the prefetch has nothing to fetch
    "one_tile": [1024],
    # tails on either side of a tile edge; an object boundary directly
    # after a prefetched tile
    "tile_edges": [1023, 1025, 16, 17, 2048, 3077],
    # more objects than any wave has tiles: every wave crosses a boundary
    "many_small": [100] * 300,
    # empty objects leading, consecutive and trailing
    "with_empties": [0, 4096, 0, 0, 777, 0],
    # just over 32768 tiles: the 4096-block cap binds, 3 tiles per wave
    "grid_cap": [8 * MB + 1, 3, 12 * MB + 1023, 1 * MB, 12 * MB + 512],
}


class TestFusedPutKernel:
    """fused_put / FusedPutPlan at kernel level, next to the hash-only batch
    kernel they share their tile walk with: digests bit-exact against the
    CPU reference, bytes copied exactly, nothing stored past an object."""

    def _run(self, sizes, entry):
        case = _put_case(sizes)
        src, dst = gpu.malloc(case.span), gpu.malloc(case.span)
        try:
            gpu.upload(src, case.src_image)
            gpu.upload(dst, bytes([case.PAD]) * case.span)
            # an empty object is a non-null pointer with size 0
            descs = [(src + o, dst + o, s)
                     for o, s in zip(case.offs, case.sizes)]
            if entry == "checksum_device_batch":
                steps = [gpu.checksum_device_batch(
                    [(s, n) for s, _, n in descs])]
            elif entry == "fused_put":
                steps = [gpu.fused_put(descs)]
            else:
                steps = gpu.fused_put_plan(descs, 2)
                assert len(steps) == 2
                # accumulators are reset inside the captured graph
                assert steps[1] == steps[0]
            for got in steps:
                bad = [i for i, (g_, w) in enumerate(zip(got, case.want))
                       if g_ != w]
                assert len(got) == len(case.want) and not bad, (entry, bad[:8])
            if entry != "checksum_device_batch":
                # every object's bytes landed; every gap byte and every byte
                # past an object's end still holds the pre-fill
                assert gpu.download(dst, case.span) == case.dst_image, entry
        finally:
            gpu.free(src)
            gpu.free(dst)

    @pytest.mark.parametrize("name", list(PUT_SIZE_LISTS))
    def test_checksum_device_batch(self, name):
        self._run(PUT_SIZE_LISTS[name], "checksum_device_batch")

    @pytest.mark.parametrize("name", list(PUT_SIZE_LISTS))
    def test_fused_put(self, name):
        self._run(PUT_SIZE_LISTS[name], "fused_put")

    @pytest.mark.parametrize("name", list(PUT_SIZE_LISTS))
    def test_fused_put_plan(self, name):
        self._run(PUT_SIZE_LISTS[name], "fused_put_plan")

    def test_all_empty_batch(self):
        """Every object empty: both one-shot entry points return the digest
        of the empty string per object (digest_spec.h); a plan refuses."""
        buf = gpu.malloc(64)
        try:
            want = [gpu.checksum_cpu(b"")] * 2
            assert gpu.checksum_device_batch([(buf, 0), (buf + 16, 0)]) == want
            descs = [(buf, buf + 32, 0), (buf + 16, buf + 48, 0)]
            assert gpu.fused_put(descs) == want
            with pytest.raises(Exception, match="INVALID_ARGUMENT"):
                gpu.fused_put_plan(descs, 2)
        finally:
            gpu.free(buf)


class TestMemops:
    def test_fill_verify(self):
        n = 8 * MB
        ptr = gpu.malloc(n)
        try:
            gpu.fill_pattern(ptr, n, seed=9)
            assert gpu.verify_pattern(ptr, n, seed=9) == 0
            assert gpu.verify_pattern(ptr, n, seed=10) > 0
        finally:
            gpu.free(ptr)

    def test_batched_copy(self):
        rng = np.random.default_rng(3)
        # 0 in the middle: a descriptor that owns no chunk; 4097: one full
        # 4 KiB chunk plus a 1-byte chunk
        sizes = [4096, 1 * MB, 0, 100, 256 * 1024 + 13, 4097, 5000]
        src_skew = [0, 0, 0, 0, 0, 0, 1]  # last one takes the unaligned branch
        bases, srcs, dsts, blobs = [], [], [], []
        try:
            for s, k in zip(sizes, src_skew):
                blob = rng.integers(0, 256, size=s, dtype=np.uint8).tobytes()
                sp, dp = gpu.malloc(s + 16), gpu.malloc(s + 16)
                bases += [sp, dp]
                gpu.upload(sp + k, blob)
                srcs.append(sp + k)
                dsts.append(dp)
                blobs.append(blob)
            gpu.batched_copy([(srcs[i], dsts[i], sizes[i]) for i in range(len(sizes))])
            for i, s in enumerate(sizes):
                assert gpu.download(dsts[i], s) == blobs[i], i
        finally:
            for p in bases:
                gpu.free(p)


class TestHbmBackend:
    def test_reserve_io_checksum(self):
        cfg = bb.PoolConfig()
        cfg.pool_id = "hbm0"
        cfg.storage_class = bb.StorageClass.RAM_GPU
        cfg.size_bytes = 64 * MB
        b = bb.make_backend(cfg, "gputest%d" % os.getpid())
        t = b.reserve(1 * MB)
        b.commit(t.token_id)
        data = os.urandom(1 * MB)
        b.write(t.offset, data)
        assert b.read(t.offset, 1 * MB) == data
        assert b.checksum(t.offset, 1 * MB) == bb.core.gpu.checksum_cpu(data)
        a = b.access_info()
        assert a.kind == bb.AccessKind.HIP_IPC
        assert a.device_id == 0 and len(a.ipc_handle_hex) > 0

    def test_resolver_views_of_in_process_pools(self):
        """The resolver's same-process rung on the GPU: an HBM pool is a
        device view at the backend's base; a PINNED_CPU pool is a host view
        that GpuClient maps for the device with the view's size, and a put
        and a verified get of 12 whole tiles plus a 57-byte partial one at an
        unaligned tail go through that mapping."""
        n = 12345
        cl = Cluster(n_workers=1, pool_bytes=8 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        try:
            v = bb.PoolMapperForTest.local("pool0_0")
            be = cl.workers[0].backend("pool0_0")
            assert v.device and v.size == 8 * MB
            assert v.base != 0 and v.base == be.access_info().base_addr
            assert v.local.storage_class() == bb.StorageClass.RAM_GPU
        finally:
            cl.stop()
        cl = Cluster(n_workers=1, pool_bytes=8 * MB,
                     storage_class=bb.StorageClass.PINNED_CPU)
        src = gpu.malloc(n + 256)
        dst = gpu.malloc(n + 256)
        try:
            v = bb.PoolMapperForTest.local("pool0_0")
            assert not v.device and v.base != 0 and v.size == 8 * MB
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            base = gcl.pool_base_for_test("pool0_0")
            assert base != 0
            data = os.urandom(n)
            gpu.upload(src, data)
            gcl.put_device("pinned-odd", src, n)
            sh = cl.keystone.service().get_workers("pinned-odd") \
                .copies[0].shards[0]
            assert sh.pool_id == "pool0_0" and sh.length == n
            # the pool holds the bytes, seen from the host view and through
            # the device-visible base alike
            assert v.read(sh.offset, n) == data
            assert gpu.download(base + sh.offset, n) == data
            assert gcl.get_device("pinned-odd", dst, n, verify=True) == n
            assert gpu.download(dst, n) == data
            c.close()
        finally:
            gpu.free(src)
            gpu.free(dst)
            cl.stop()

    def test_hbm_cluster_e2e(self):
        cl = Cluster(n_workers=1, pool_bytes=256 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        try:
            c = cl.client(verify_checksum_on_get=True)
            data = os.urandom(1 * MB)
            c.put("gobj", data)
            assert c.get("gobj") == data
            # batched 1 MiB objects — the config #2 shape
            items = [("g%02d" % i, os.urandom(1 * MB)) for i in range(8)]
            assert c.batch_put(items) == [0] * 8
            res = c.batch_get([k for k, _ in items])
            for (k, d), (s, got) in zip(items, res):
                assert s == 0 and got == d
            st = c.cluster_stats()
            assert st.total_used >= 9 * MB
            c.close()
        finally:
            cl.stop()

    def test_scrub_detects_hbm_corruption(self):
        """Digest scrubbing over the HBM tier: bit-rot in device memory is
        caught by the worker's MFMA re-checksum and the object quarantined."""
        cl = Cluster(n_workers=1, pool_bytes=128 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        try:
            c = cl.client()
            data = os.urandom(512 * 1024)
            c.put("hbm-rot", data)
            ks = cl.keystone.service()
            assert ks.run_scrub_once() == 0  # clean pass first
            sh = ks.get_workers("hbm-rot").copies[0].shards[0]
            cl.workers[0].backend(sh.pool_id).write(sh.offset + 4096,
                                                    b"\xff" * 64)
            assert ks.run_scrub_once() == 1
            assert not c.exists("hbm-rot")
            c.close()
        finally:
            cl.stop()


class TestGpuTiering:
    def test_hbm_spill_to_pinned_and_nvme(self, tmp_path):
        """Config #4 on the GPU tier: HBM pool fills past the watermark →
        demotion through PINNED_CPU → NVME via hipMemcpyAsync pulls; data
        stays intact and digest-verified."""
        import time
        cs = bb.CoordServer(); cs.start("127.0.0.1", 0)
        ep = "127.0.0.1:%d" % cs.port
        kc = bb.KeystoneConfig()
        kc.listen_address = "127.0.0.1:0"
        kc.coord_endpoint = ep
        kc.gc_interval_ms = 100000
        kc.tier_high_watermark = 0.6
        srv = bb.create_and_start_keystone(kc)
        wc = bb.WorkerConfig()
        wc.worker_id = "gt0"
        wc.coord_endpoint = ep
        wc.data_listen_address = "127.0.0.1:0"
        hbm = bb.PoolConfig(); hbm.pool_id = "thbm"
        hbm.storage_class = bb.StorageClass.RAM_GPU; hbm.size_bytes = 16 * MB
        pin = bb.PoolConfig(); pin.pool_id = "tpin"
        pin.storage_class = bb.StorageClass.PINNED_CPU; pin.size_bytes = 16 * MB
        nvme = bb.PoolConfig(); nvme.pool_id = "tnvme"
        nvme.storage_class = bb.StorageClass.NVME; nvme.size_bytes = 128 * MB
        nvme.mount_path = str(tmp_path)
        wc.pools = [hbm, pin, nvme]
        w = bb.WorkerService(wc)
        w.initialize(); w.start()
        deadline = time.time() + 5
        while time.time() < deadline and len(srv.service().get_memory_pools()) < 3:
            time.sleep(0.02)
        try:
            o = bb.ClientOptions(); o.keystone_endpoint = srv.endpoint
            o.verify_checksum_on_get = True
            c = bb.Client(o); c.connect()
            cfg = bb.PlacementConfig()
            cfg.preferred_class = bb.StorageClass.RAM_GPU
            ks = srv.service()
            blobs = {}
            for i in range(32):  # 32 MB through a 16 MB HBM pool
                key = "g%d" % i
                blobs[key] = os.urandom(1 * MB)
                c.put(key, blobs[key], cfg)
                if i % 4 == 3:
                    ks.run_tiering_once()
            ks.run_tiering_once()
            classes = {}
            for k in blobs:
                info = ks.get_workers(k)
                classes[k] = info.copies[0].shards[0].storage_class
            spilled = [k for k, cl in classes.items()
                       if cl != bb.StorageClass.RAM_GPU]
            assert spilled, classes
            for k, v in blobs.items():
                assert c.get(k) == v, (k, classes[k])
            # explicit round trip back into HBM
            victim = spilled[0]
            ks.migrate_object(victim, bb.StorageClass.RAM_GPU)
            info = ks.get_workers(victim)
            assert info.copies[0].shards[0].storage_class == bb.StorageClass.RAM_GPU
            assert c.get(victim) == blobs[victim]
            c.close()
        finally:
            w.stop(); srv.stop(); srv.service().stop(); cs.stop()


class TestRcclEngine:
    def test_two_rank_alltoall(self, tmp_path):
        """RCCL grouped send/recv between two ranks (needs ≥2 devices —
        skipped on single-GPU boxes; the 8-GPU driver environment runs it)."""
        if bb.core.gpu.device_count() < 2:
            pytest.skip("needs >=2 GPUs (RCCL: one rank per device)")
        import subprocess, sys, textwrap
        script = tmp_path / "rccl2.py"
        script.write_text(textwrap.dedent(f"""
            import sys, os
            sys.path.insert(0, {repr(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))})
            import blackbird_amd as bb
            rank = int(sys.argv[1]); ep = sys.argv[2]
            g = bb.core.gpu
            MB = 1 << 20
            coord = bb.CoordClient(); coord.connect(ep)
            e = bb.RcclEngine()
            e.init(coord, "rtest", "t1", rank, 2, rank)
            send = g.malloc(2 * MB, rank); recv = g.malloc(2 * MB, rank)
            g.fill_pattern(send, 2 * MB, seed=100 + rank)
            e.alltoallv([send, send + MB][: 2], [MB, MB],
                        [recv, recv + MB][: 2], [MB, MB])
            # slot from peer carries the peer's pattern half
            peer = 1 - rank
            bad_self = g.verify_pattern(recv + rank * MB, MB, seed=100 + rank)
            assert bad_self == 0, bad_self
            e.destroy()
            print("RANK", rank, "OK")
        """))
        cs = bb.CoordServer()
        cs.start("127.0.0.1", 0)
        ep = "127.0.0.1:%d" % cs.port
        try:
            procs = [subprocess.Popen([sys.executable, str(script), str(r), ep],
                                      stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT)
                     for r in (0, 1)]
            for p in procs:
                out, _ = p.communicate(timeout=120)
                assert p.returncode == 0, out.decode()
                assert b"OK" in out
        finally:
            cs.stop()


class TestGpuClientPaths:
    def test_jumbo_object_roundtrip(self):
        """One 200 MiB object through the fused copy+digest path: bytes land
        exactly, the kernel digest matches the bit-exact CPU reference, and
        the verified get passes. (288 GB HBM pools make multi-hundred-MiB
        objects a normal case, not an edge.)"""
        S = 200 * MB
        cl = Cluster(n_workers=1, pool_bytes=512 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        g = bb.core.gpu
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            src = g.malloc(S)
            dst = g.malloc(S)
            g.fill_pattern(src, S, seed=4242)
            g.sync()
            assert gcl.batch_put_device([("jumbo", src, S)]) == [0]
            assert gcl.batch_get_device([("jumbo", dst, S)], verify=True) == [0]
            g.sync()
            assert g.verify_pattern(dst, S, seed=4242) == 0
            blob = g.download(src, S)
            info = cl.keystone.service().get_workers("jumbo")
            assert info.size == S
            assert info.checksum == g.checksum_cpu(blob)
            c.close()
            g.free(src)
            g.free(dst)
        finally:
            cl.stop()

    def test_device_put_get_fused_and_verified(self):
        """GpuClient batch_put_device (fused copy+digest kernel path) and
        get_device: bytes land correctly, digests match the CPU reference,
        verification catches corruption."""
        cl = Cluster(n_workers=1, pool_bytes=512 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        g = bb.core.gpu
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            N, S = 16, 1 * MB
            blobs = [os.urandom(S) for _ in range(N)]
            src = g.malloc(N * S)
            dst = g.malloc(N * S)
            for i, b in enumerate(blobs):
                g.upload(src + i * S, b)
            items = [("dv%02d" % i, src + i * S, S) for i in range(N)]
            st = gcl.batch_put_device(items)
            assert st == [0] * N
            # digests recorded in keystone match the CPU reference
            ks = cl.keystone.service()
            for i, b in enumerate(blobs):
                info = ks.get_workers("dv%02d" % i)
                assert info.checksum == g.checksum_cpu(b), i
            # bytes land correctly (read back through the host client)
            o = bb.ClientOptions()
            o.keystone_endpoint = cl.keystone.endpoint
            o.verify_checksum_on_get = True
            hc = bb.Client(o)
            hc.connect()
            for i, b in enumerate(blobs):
                assert hc.get("dv%02d" % i) == b, i
            # device-side batch get with kernel verification
            get_items = [("dv%02d" % i, dst + i * S, S) for i in range(N)]
            st = gcl.batch_get_device(get_items, verify=True)
            assert st == [0] * N
            for i, b in enumerate(blobs):
                assert g.download(dst + i * S, S) == b, i
            # single-object device path + verify catches corruption
            n = gcl.get_device("dv00", dst, S, verify=True)
            assert n == S
            pool = cl.workers[0].pool_descriptors()[0]
            be = cl.workers[0].backend(pool.pool_id)
            info = ks.get_workers("dv05")
            be.write(info.copies[0].shards[0].offset, b"\x00" * 64)
            with pytest.raises(Exception, match="CHECKSUM_MISMATCH"):
                gcl.get_device("dv05", dst, S, verify=True)
            hc.close()
            c.close()
            g.free(src)
            g.free(dst)
        finally:
            cl.stop()

    def test_verified_placement_cache(self):
        """Opt-in placement cache: gets of this client's own puts skip the
        metadata RPC (one-sided read validated by the in-kernel digest);
        a moved/replaced object falls back to the RPC path transparently."""
        cl = Cluster(n_workers=1, pool_bytes=256 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        g = bb.core.gpu
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            gcl.set_placement_cache(True)
            N, S = 8, 1 * MB
            blobs = [os.urandom(S) for _ in range(N)]
            src = g.malloc(N * S)
            dst = g.malloc(N * S)
            for i, b in enumerate(blobs):
                g.upload(src + i * S, b)
            puts = [("pc%02d" % i, src + i * S, S) for i in range(N)]
            gets = [("pc%02d" % i, dst + i * S, S) for i in range(N)]
            assert gcl.batch_put_device(puts) == [0] * N
            # cached get: correct bytes (the RPC-free leg)
            assert gcl.batch_get_device(gets) == [0] * N
            for i, b in enumerate(blobs):
                assert g.download(dst + i * S, S) == b, i
            # REPLACE one object with different bytes through ANOTHER client
            # (this GpuClient's cache entry goes stale)
            o = bb.ClientOptions()
            o.keystone_endpoint = cl.keystone.endpoint
            hc = bb.Client(o)
            hc.connect()
            cfg = bb.PlacementConfig()
            cfg.replace = True
            new3 = os.urandom(S)
            hc.put("pc03", new3, cfg)
            # stale cached read digest-mismatches → transparent RPC refetch
            assert gcl.batch_get_device(gets) == [0] * N
            assert g.download(dst + 3 * S, S) == new3
            for i, b in enumerate(blobs):
                if i != 3:
                    assert g.download(dst + i * S, S) == b, i
            # removal + explicit invalidate → NOT_FOUND (no ghost reads)
            hc.remove("pc05")
            gcl.invalidate(["pc05"])
            st = gcl.batch_get_device([("pc05", dst, S)])
            assert st[0] != 0
            hc.close()
            c.close()
            g.free(src)
            g.free(dst)
        finally:
            cl.stop()

    def test_async_pipelined_batches(self):
        """batch_put_async/batch_get_async: two batches in flight on one
        GpuClient (metadata RPC of one overlaps GPU work of the other);
        results identical to the synchronous path, bad tokens rejected."""
        cl = Cluster(n_workers=1, pool_bytes=512 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        g = bb.core.gpu
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            N, S = 16, 256 * 1024
            blobs = [os.urandom(S) for _ in range(2 * N)]
            src = g.malloc(2 * N * S)
            dst = g.malloc(2 * N * S)
            for i, b in enumerate(blobs):
                g.upload(src + i * S, b)
            itemsA = [("asyA%02d" % i, src + i * S, S) for i in range(N)]
            itemsB = [("asyB%02d" % i, src + (N + i) * S, S) for i in range(N)]
            tA = gcl.batch_put_async(itemsA)
            tB = gcl.batch_put_async(itemsB)
            assert gcl.async_wait(tA) == [0] * N
            assert gcl.async_wait(tB) == [0] * N
            with pytest.raises(Exception, match="INVALID_ARGUMENT"):
                gcl.async_wait(tA)  # token consumed
            getA = [("asyA%02d" % i, dst + i * S, S) for i in range(N)]
            getB = [("asyB%02d" % i, dst + (N + i) * S, S) for i in range(N)]
            gA = gcl.batch_get_async(getA, verify=True)
            gB = gcl.batch_get_async(getB, verify=True)
            assert gcl.async_wait(gB) == [0] * N  # out-of-order wait
            assert gcl.async_wait(gA) == [0] * N
            for i, b in enumerate(blobs):
                assert g.download(dst + i * S, S) == b, i
            c.close()
            g.free(src)
            g.free(dst)
        finally:
            cl.stop()

    def test_device_put_odd_sizes(self):
        """Tail-tile handling in the fused kernel: non-1KiB-multiple sizes."""
        cl = Cluster(n_workers=1, pool_bytes=128 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        g = bb.core.gpu
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            sizes = [1, 100, 1023, 1025, 65536 + 17, 1 * MB - 1]
            buf = g.malloc(8 * MB)
            blobs = {}
            off = 0
            items = []
            for i, s in enumerate(sizes):
                b = os.urandom(s)
                g.upload(buf + off, b)
                key = "odd%d" % i
                blobs[key] = b
                items.append((key, buf + off, s))
                off += (s + 255) // 256 * 256  # keep 16B alignment
            st = gcl.batch_put_device(items)
            assert st == [0] * len(sizes)
            hc = cl.client(verify_checksum_on_get=True)
            for key, b in blobs.items():
                assert hc.get(key) == b, key
            hc.close()
            c.close()
            g.free(buf)
        finally:
            cl.stop()

    def test_sdma_fallback_roundtrip(self):
        """set_fused_copy(False): every transfer rides hipMemcpyAsync on the
        rotating streams and digests come from the separate batched checksum
        launch. Covers the compact batch path (one worker) and the striped
        multi-shard put/get halves (two workers)."""
        g = bb.core.gpu
        cl = Cluster(n_workers=1, pool_bytes=64 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            gcl.set_fused_copy(False)
            sizes = [1, 1023, 4096, 65536 + 17]
            buf = g.malloc(1 * MB)
            dst = g.malloc(1 * MB)
            blobs, puts, gets = [], [], []
            off = 0
            for i, s in enumerate(sizes):
                b = os.urandom(s)
                g.upload(buf + off, b)
                blobs.append(b)
                puts.append(("sdma%d" % i, buf + off, s))
                gets.append(("sdma%d" % i, dst + off, s))
                off += (s + 255) // 256 * 256  # keep 16B alignment
            assert gcl.batch_put_device(puts) == [0] * len(sizes)
            assert gcl.batch_get_device(gets, verify=True) == [0] * len(sizes)
            ks = cl.keystone.service()
            for (key, ptr, s), b in zip(gets, blobs):
                assert g.download(ptr, s) == b, key
                assert ks.get_workers(key).checksum == g.checksum_cpu(b), key
            c.close()
            g.free(buf)
            g.free(dst)
        finally:
            cl.stop()
        cl = Cluster(n_workers=2, pool_bytes=64 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            gcl.set_fused_copy(False)
            S = 8 * MB
            src = g.malloc(S)
            dst = g.malloc(S)
            blob = os.urandom(S)
            g.upload(src, blob)
            cfg = bb.PlacementConfig()
            cfg.max_workers_per_copy = 2
            assert gcl.batch_put_device([("sdma-striped", src, S)], cfg) == [0]
            info = cl.keystone.service().get_workers("sdma-striped")
            assert len(info.copies[0].shards) == 2
            assert info.checksum == g.checksum_cpu(blob)
            assert gcl.batch_get_device([("sdma-striped", dst, S)],
                                        verify=True) == [0]
            assert g.download(dst, S) == blob
            c.close()
            g.free(src)
            g.free(dst)
        finally:
            cl.stop()

    def test_unaligned_buffers_roundtrip(self):
        """Sources and destinations 8 bytes off 16-byte alignment take the
        copy-only kernel plus a separate digest launch instead of the fused
        copy+digest kernel. Every size stays below one 1 KiB digest tile, so
        only the byte-guarded fragment loads and the byte loop of the copy
        kernel touch the misaligned addresses."""
        cl = Cluster(n_workers=1, pool_bytes=64 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        g = bb.core.gpu
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            sizes = [1, 100, 1023]
            buf = g.malloc(1 * MB)
            dst = g.malloc(1 * MB)
            assert buf % 16 == 0 and dst % 16 == 0
            blobs, puts, gets = [], [], []
            off = 8
            for i, s in enumerate(sizes):
                b = os.urandom(s)
                g.upload(buf + off, b)
                blobs.append(b)
                puts.append(("unal%d" % i, buf + off, s))
                gets.append(("unal%d" % i, dst + off, s))
                off += 4096
            assert gcl.batch_put_device(puts) == [0] * len(sizes)
            hc = cl.client(verify_checksum_on_get=True)
            ks = cl.keystone.service()
            for (key, _, _), b in zip(puts, blobs):
                assert hc.get(key) == b, key
                assert ks.get_workers(key).checksum == g.checksum_cpu(b), key
            assert gcl.batch_get_device(gets, verify=True) == [0, 0, 0]
            for (key, ptr, s), b in zip(gets, blobs):
                assert g.download(ptr, s) == b, key
            hc.close()
            c.close()
            g.free(buf)
            g.free(dst)
        finally:
            cl.stop()


class TestGpuReplication:
    def test_device_put_replicated_single_worker(self):
        """replication=2 on one worker: soft spreading allows same-worker
        copies as last resort; both copies written and readable."""
        cl = Cluster(n_workers=1, pool_bytes=256 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        g = bb.core.gpu
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            S = 1 * MB
            src = g.malloc(S)
            dst = g.malloc(S)
            blob = os.urandom(S)
            g.upload(src, blob)
            cfg = bb.PlacementConfig()
            cfg.replication = 2
            st = gcl.batch_put_device([("rep-obj", src, S)], cfg)
            assert st == [0]
            ks = cl.keystone.service()
            info = ks.get_workers("rep-obj")
            assert len(info.copies) == 2
            # both copies hold the right bytes
            pool = cl.workers[0].pool_descriptors()[0]
            be = cl.workers[0].backend(pool.pool_id)
            for cp in info.copies:
                assert be.read(cp.shards[0].offset, S) == blob
            assert gcl.get_device("rep-obj", dst, S, verify=True) == S
            g.free(src)
            g.free(dst)
            c.close()
        finally:
            cl.stop()


class TestGpuDaemons:
    def test_daemon_cluster_hbm_roundtrip(self, tmp_path):
        """Real daemons (coordd + keystoned + workerd with an HBM pool) and
        the bbctl CLI: put/get/verify through the worker's TCP data plane
        into GPU memory."""
        import json as _json
        import signal
        import socket
        import subprocess
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        bin_dir = os.path.join(repo, "bin")
        if not os.path.exists(os.path.join(bin_dir, "coordd")):
            pytest.skip("daemons not built")

        def free_port():
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            p = s.getsockname()[1]
            s.close()
            return p

        coord_port, ks_port = free_port(), free_port()
        procs = []

        def spawn(args, logname):
            f = open(tmp_path / logname, "w")
            p = subprocess.Popen(args, stdout=f, stderr=subprocess.STDOUT)
            procs.append(p)

        try:
            spawn([f"{bin_dir}/coordd", "--listen-host", "127.0.0.1",
                   "--listen-port", str(coord_port)], "coordd.log")
            import time
            time.sleep(0.3)
            spawn([f"{bin_dir}/keystoned",
                   "--listen-address", f"127.0.0.1:{ks_port}",
                   "--coord-endpoint", f"127.0.0.1:{coord_port}",
                   "--metrics-address", "127.0.0.1:0"], "keystoned.log")
            time.sleep(0.3)
            cfg = {"worker_id": "gdw0",
                   "coord_endpoint": f"127.0.0.1:{coord_port}",
                   "data_listen_address": "127.0.0.1:0",
                   "pools": [{"pool_id": "gd-hbm", "storage_class": "RAM_GPU",
                              "size_bytes": 128 << 20, "gpu_device_id": 0}]}
            (tmp_path / "worker.json").write_text(_json.dumps(cfg))
            spawn([f"{bin_dir}/workerd", "--config",
                   str(tmp_path / "worker.json")], "workerd.log")

            deadline = time.time() + 15
            ok = False
            while time.time() < deadline:
                r = subprocess.run([f"{bin_dir}/bbctl", "--keystone",
                                    f"127.0.0.1:{ks_port}", "pools"],
                                   capture_output=True, text=True)
                if r.returncode == 0 and "RAM_GPU" in r.stdout:
                    ok = True
                    break
                time.sleep(0.3)
            assert ok, (tmp_path / "workerd.log").read_text()[-800:]

            payload = os.urandom(2 * MB + 333)
            r = subprocess.run([f"{bin_dir}/bbctl", "--keystone",
                                f"127.0.0.1:{ks_port}", "--class", "RAM_GPU",
                                "put", "gpu-cli-obj", "-"],
                               input=payload, capture_output=True)
            assert r.returncode == 0, r.stderr
            r = subprocess.run([f"{bin_dir}/bbctl", "--keystone",
                                f"127.0.0.1:{ks_port}", "get", "gpu-cli-obj"],
                               capture_output=True)
            assert r.returncode == 0 and r.stdout == payload
            r = subprocess.run([f"{bin_dir}/bbctl", "--keystone",
                                f"127.0.0.1:{ks_port}", "verify", "gpu-cli-obj"],
                               capture_output=True)
            assert r.returncode == 0, r.stderr
            # native GPU benchmark client: device buffers + fused kernels +
            # placement cache against the daemon cluster, pattern-verified
            r = subprocess.run([f"{bin_dir}/bb_bench", "--keystone",
                                f"127.0.0.1:{ks_port}", "--gpu", "0",
                                "--batch", "16", "--iters", "3"],
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout + r.stderr
            assert "TOTAL" in r.stdout
        finally:
            for p in procs:
                p.send_signal(signal.SIGTERM)
            for p in procs:
                try:
                    p.wait(timeout=5)
                except subprocess.TimeoutExpired:
                    p.kill()



    def test_cross_process_shm_pool_fused(self, tmp_path):
        """GPU client against a RAM_CPU pool owned by a SEPARATE worker
        process: the pool is shm-mapped, GPU-mapped (hipHostRegister), and
        the fused copy+digest kernel writes/reads it directly over PCIe.
        Regression test: the first hipHostGetDevicePointer probe fails by
        design and must not poison later kernel-launch error checks."""
        import json as _json
        import signal
        import socket
        import subprocess
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        bin_dir = os.path.join(repo, "bin")
        if not os.path.exists(os.path.join(bin_dir, "coordd")):
            pytest.skip("daemons not built")
        g = bb.core.gpu

        def free_port():
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            p = s.getsockname()[1]
            s.close()
            return p

        cp, kp = free_port(), free_port()
        procs = []

        def spawn(args, logname):
            f = open(tmp_path / logname, "w")
            procs.append(subprocess.Popen(args, stdout=f,
                                          stderr=subprocess.STDOUT))

        try:
            spawn([f"{bin_dir}/coordd", "--listen-host", "127.0.0.1",
                   "--listen-port", str(cp)], "c.log")
            time.sleep(0.3)
            spawn([f"{bin_dir}/keystoned",
                   "--listen-address", f"127.0.0.1:{kp}",
                   "--coord-endpoint", f"127.0.0.1:{cp}",
                   "--metrics-address", "127.0.0.1:0"], "k.log")
            time.sleep(0.3)
            cfg = {"worker_id": "shmw0",
                   "coord_endpoint": f"127.0.0.1:{cp}",
                   "data_listen_address": "127.0.0.1:0",
                   "pools": [{"pool_id": "shm-pool",
                              "storage_class": "RAM_CPU",
                              "size_bytes": 256 << 20}]}
            (tmp_path / "w.json").write_text(_json.dumps(cfg))
            spawn([f"{bin_dir}/workerd", "--config",
                   str(tmp_path / "w.json")], "w.log")

            o = bb.ClientOptions()
            o.keystone_endpoint = f"127.0.0.1:{kp}"
            c = bb.Client(o)
            deadline = time.time() + 15
            while True:
                try:
                    c.connect()
                    if c.memory_pools():
                        break
                except Exception:
                    pass
                assert time.time() < deadline, "cluster did not assemble"
                time.sleep(0.3)

            gcl = bb.GpuClient(c, 0)
            gcl.init()
            N, S = 8, 1 * MB
            src = g.malloc(N * S)
            dst = g.malloc(N * S)
            g.fill_pattern(src, N * S, seed=3)
            g.sync()
            items = [("shx%d" % i, src + i * S, S) for i in range(N)]
            cfgp = bb.PlacementConfig()
            cfgp.checksum = True
            assert gcl.batch_put_device(items, cfgp) == [0] * N
            assert gcl.batch_get_device(
                [(k, dst + i * S, S) for i, (k, _, _) in enumerate(items)],
                verify=True) == [0] * N
            g.sync()
            assert g.verify_pattern(dst, N * S, seed=3) == 0
            c.batch_remove([k for k, _, _ in items])
            c.close()
            g.free(src)
            g.free(dst)
        finally:
            for p in procs:
                p.send_signal(signal.SIGTERM)
            for p in procs:
                try:
                    p.wait(timeout=5)
                except subprocess.TimeoutExpired:
                    p.kill()


class TestGpuStriping:
    def test_striped_device_put_across_hbm_pools(self):
        """max_workers_per_copy=2 through GpuClient (the v1 multi-shard
        path): one object striped across two workers' HBM pools, written
        and read back from device buffers."""
        cl = Cluster(n_workers=2, pool_bytes=128 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        g = bb.core.gpu
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            S = 8 * MB
            src = g.malloc(S)
            dst = g.malloc(S)
            blob = os.urandom(S)
            g.upload(src, blob)
            cfg = bb.PlacementConfig()
            cfg.max_workers_per_copy = 2
            st = gcl.batch_put_device([("striped-dev", src, S)], cfg)
            assert st == [0]
            info = cl.keystone.service().get_workers("striped-dev")
            assert len(info.copies[0].shards) == 2
            assert len({s.worker_id for s in info.copies[0].shards}) == 2
            assert gcl.get_device("striped-dev", dst, S) == S
            assert g.download(dst, S) == blob
            # host read crosses the same shards
            hc = cl.client(verify_checksum_on_get=True)
            assert hc.get("striped-dev") == blob
            hc.close()
            g.free(src)
            g.free(dst)
            c.close()
        finally:
            cl.stop()


CHECKSUM_MISMATCH = 5003  # ErrorCode::CHECKSUM_MISMATCH (common/error.h)


class _SessionRig:
    """RAM_GPU workers, one client with the placement cache on, and prepared
    put/get batches over back-to-back device buffers."""

    def __init__(self, n_workers, sizes, prefix):
        self.cl = Cluster(n_workers=n_workers, pool_bytes=64 * MB,
                          storage_class=bb.StorageClass.RAM_GPU)
        self.c = self.cl.client()
        self.gcl = bb.GpuClient(self.c, 0)
        self.gcl.init()
        self.gcl.set_placement_cache(True)
        self.ks = self.cl.keystone.service()
        self.sizes = sizes
        self.keys = ["%s%02d" % (prefix, i) for i in range(len(sizes))]
        self.offs = [sum(sizes[:i]) for i in range(len(sizes))]
        self.src, self.dst = gpu.malloc(sum(sizes)), gpu.malloc(sum(sizes))
        self.pb = bb.make_put_batch(
            [(k, self.src + o, n)
             for k, o, n in zip(self.keys, self.offs, sizes)])
        self.gb = bb.make_get_batch(
            [(k, self.dst + o, n)
             for k, o, n in zip(self.keys, self.offs, sizes)])

    @staticmethod
    def cfg(replication=1, max_workers_per_copy=1):
        cfg = bb.PlacementConfig()
        cfg.replace = True
        cfg.checksum = True
        cfg.replication = replication
        cfg.max_workers_per_copy = max_workers_per_copy
        return cfg

    def put(self, cfg):
        """Fresh contents through the prepared put batch."""
        blobs = [os.urandom(n) for n in self.sizes]
        for o, b in zip(self.offs, blobs):
            gpu.upload(self.src + o, b)
        assert self.gcl.batch_put_prepared(self.pb, cfg)
        return blobs

    def step(self, cfg):
        """put, then the prepared get batch, then the bytes compared."""
        blobs = self.put(cfg)
        assert self.gcl.batch_get_prepared(self.gb)
        for o, b in zip(self.offs, blobs):
            assert gpu.download(self.dst + o, len(b)) == b, o
        return blobs

    def check(self, blobs):
        """A verified one-shot get returns `blobs`, and the keystone holds
        their CPU-reference checksums."""
        st = self.gcl.batch_get_device(
            [(k, self.dst + o, n)
             for k, o, n in zip(self.keys, self.offs, self.sizes)],
            verify=True)
        assert st == [0] * len(blobs), st
        for k, o, b in zip(self.keys, self.offs, blobs):
            assert gpu.download(self.dst + o, len(b)) == b, k
            assert self.ks.get_workers(k).checksum == gpu.checksum_cpu(b), k

    def corrupt(self, key, copy):
        """64 zero bytes at offset 4096 of the only shard of `copy`."""
        bad = self.ks.get_workers(key).copies[copy].shards[0]
        victim = next(w for w in self.cl.workers
                      if any(p.pool_id == bad.pool_id
                             for p in w.pool_descriptors()))
        victim.backend(bad.pool_id).write(bad.offset + 4096, b"\x00" * 64)

    def close(self):
        gpu.free(self.src)
        gpu.free(self.dst)
        self.c.close()
        self.cl.stop()


class TestBatchSessions:
    def test_session_fast_path_roundtrip(self):
        """Prepared batches establish a put session on the first step; later
        steps ride the token fast path (two tiny RPCs, one fused kernel) and
        gets go fully RPC-free. Data must stay correct as the source buffer
        changes between steps, and server-side interference must invalidate
        the session transparently."""
        cl = Cluster(n_workers=1, pool_bytes=256 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        g = bb.core.gpu
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            gcl.set_placement_cache(True)
            N, S = 32, 64 * 1024
            src = g.malloc(N * S)
            dst = g.malloc(N * S)
            cfg = bb.PlacementConfig()
            cfg.replace = True
            pb = bb.make_put_batch([("sess%02d" % i, src + i * S, S)
                                    for i in range(N)])
            gb = bb.make_get_batch([("sess%02d" % i, dst + i * S, S)
                                    for i in range(N)])
            ks = cl.keystone.service()

            for step in range(4):
                blobs = [os.urandom(S) for _ in range(N)]
                for i, b in enumerate(blobs):
                    g.upload(src + i * S, b)
                assert gcl.batch_put_prepared(pb, cfg)
                assert gcl.batch_get_prepared(gb)
                for i, b in enumerate(blobs):
                    assert g.download(dst + i * S, S) == b, (step, i)
                # keystone's authoritative digests match the CPU reference
                info = ks.get_workers("sess07")
                assert info.checksum == g.checksum_cpu(blobs[7])
            # steps 2..4 must have used the token fast path and RPC-free gets
            assert gcl.session_put_steps >= 3, gcl.session_put_steps
            assert gcl.session_get_steps >= 2, gcl.session_get_steps
            assert ks.token_commits() >= 3
            # session steps replay the captured hipGraph, not per-op launches
            if not os.environ.get("BB_NO_HIPGRAPH"):
                assert gcl.session_graph_steps >= 3, gcl.session_graph_steps

            # server-side interference: removing ANY object bumps the
            # placement epoch → session falls back transparently, still OK
            ks.put_start("intruder", 4096, bb.PlacementConfig())
            ks.put_complete("intruder", checksum=1)
            ks.remove_object("intruder")
            blobs = [os.urandom(S) for _ in range(N)]
            for i, b in enumerate(blobs):
                g.upload(src + i * S, b)
            fast_before = gcl.session_put_steps
            assert gcl.batch_put_prepared(pb, cfg)   # full path this step
            assert gcl.batch_put_prepared(pb, cfg)   # session re-established
            assert gcl.session_put_steps == fast_before + 1
            assert gcl.batch_get_prepared(gb)
            for i, b in enumerate(blobs):
                assert g.download(dst + i * S, S) == b, i
            c.close()
            g.free(src)
            g.free(dst)
        finally:
            cl.stop()

    def test_plain_get_session_corruption(self):
        """Corruption under a live plain get session is pinned to its item:
        the session step mismatches, counts no step, and the authoritative
        refetch reports it; a fresh put heals the object and the get session
        comes back."""
        rig = _SessionRig(1, [64 * 1024] * 4, prefix="pc")
        try:
            gcl, ks = rig.gcl, rig.ks
            cfg = rig.cfg()
            for _ in range(4):
                rig.step(cfg)
                if gcl.session_get_steps >= 1:
                    break
            assert gcl.session_get_steps >= 1, gcl.session_get_steps
            rig.corrupt(rig.keys[2], copy=0)
            before = gcl.session_get_steps
            st = gcl.batch_get_prepared_statuses(rig.gb, verify=True)
            print("plain corruption statuses:", st)
            assert st == [0, 0, CHECKSUM_MISMATCH, 0]
            assert gcl.session_get_steps == before
            rig.step(cfg)  # fresh bytes: put, get, compare
            for _ in range(2):
                assert gcl.batch_get_prepared(rig.gb)
            assert gcl.session_get_steps > before, gcl.session_get_steps
        finally:
            rig.close()

    def test_replicated_get_session_corruption(self):
        """The same with two replicas on two workers, copy 0 (the one the
        cache and the get session read) of item 1 corrupted. The session step
        mismatches and counts no step. The authoritative refetch is verified
        against the keystone's checksum on the first copy it can reach, which
        is the corrupt one: the item reports CHECKSUM_MISMATCH, the others
        are untouched."""
        rig = _SessionRig(2, [64 * 1024] * 4, prefix="rc")
        try:
            gcl = rig.gcl
            cfg = rig.cfg(replication=2)
            for _ in range(4):
                rig.step(cfg)
                if gcl.session_get_steps >= 1:
                    break
            assert gcl.session_get_steps >= 1, gcl.session_get_steps
            assert len(rig.ks.get_workers(rig.keys[1]).copies) == 2
            rig.corrupt(rig.keys[1], copy=0)
            before = gcl.session_get_steps
            st = gcl.batch_get_prepared_statuses(rig.gb, verify=True)
            print("replicated corruption statuses:", st)
            assert st == [0, CHECKSUM_MISMATCH, 0, 0]
            assert gcl.session_get_steps == before
        finally:
            rig.close()

    def test_put_session_offered_to_the_other_form(self):
        """One BatchPutSession behind one prepared batch, put striped until
        the session steps, then plain, then striped again: the switching call
        takes the full path (no session step, bytes and checksum right) and
        session steps resume in the new form within two further calls.

        The objects are removed at the keystone before each switch. Without
        that the keystone upserts same-size objects IN PLACE whatever shape
        the new config asks for, so the placements would keep their old form:
        a plain put over a striped placement goes through BATCH_PUT_START2,
        which names only shard 0 of a copy, and the verified get that follows
        answers CHECKSUM_MISMATCH for all four items (a keystone/wire defect
        noted in ROADMAP.md, not a session matter); a striped put over a
        plain placement stays single-shard and never forms a striped
        session. The client still holds the session, its token and the cached
        placements of the old form when the switching call arrives."""
        rig = _SessionRig(2, [256 * 1024] * 4, prefix="sw")
        try:
            gcl, ks = rig.gcl, rig.ks
            forms = [rig.cfg(max_workers_per_copy=2), rig.cfg(),
                     rig.cfg(max_workers_per_copy=2)]
            for _ in range(4):
                rig.put(forms[0])
                if gcl.session_put_steps >= 1:
                    break
            assert gcl.session_put_steps >= 1, gcl.session_put_steps
            for cfg in forms[1:]:
                nshards = cfg.max_workers_per_copy
                for k in rig.keys:
                    ks.remove_object(k)
                before = gcl.session_put_steps
                rig.check(rig.put(cfg))  # the switching call
                assert gcl.session_put_steps == before
                for k in rig.keys:
                    assert len(ks.get_workers(k).copies[0].shards) == nshards
                for _ in range(2):
                    blobs = rig.put(cfg)
                assert gcl.session_put_steps > before, gcl.session_put_steps
                rig.check(blobs)
                for k in rig.keys:
                    assert len(ks.get_workers(k).copies[0].shards) == nshards
        finally:
            rig.close()

    def test_session_not_used_when_cache_off(self):
        cl = Cluster(n_workers=1, pool_bytes=256 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        g = bb.core.gpu
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()  # placement cache OFF
            N, S = 4, 4096
            src = g.malloc(N * S)
            cfg = bb.PlacementConfig()
            cfg.replace = True
            pb = bb.make_put_batch([("nc%d" % i, src + i * S, S)
                                    for i in range(N)])
            for _ in range(3):
                assert gcl.batch_put_prepared(pb, cfg)
            assert gcl.session_put_steps == 0
            g.free(src)
            c.close()
        finally:
            cl.stop()

    def test_concurrent_session_clients(self):
        """Two GpuClients (own metadata connections, own key spaces) run
        session-fast-path upsert loops concurrently while a third actor
        creates/removes keys to bump the placement epoch (invalidating the
        others' sessions mid-stream). Every batch must succeed and every
        get must return the bytes that client last put."""
        import threading
        cl = Cluster(n_workers=1, pool_bytes=512 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        g = bb.core.gpu
        errs = []
        quiet = threading.Event()  # set once the intruder stops
        try:
            ks = cl.keystone.service()

            def worker(tag, seed):
                try:
                    c = cl.client()
                    gcl = bb.GpuClient(c, 0)
                    gcl.init()
                    gcl.set_placement_cache(True)
                    N, S = 16, 64 * 1024
                    src = g.malloc(N * S)
                    dst = g.malloc(N * S)
                    cfg = bb.PlacementConfig()
                    cfg.replace = True
                    pb = bb.make_put_batch(
                        [("%s%02d" % (tag, i), src + i * S, S)
                         for i in range(N)])
                    gb = bb.make_get_batch(
                        [("%s%02d" % (tag, i), dst + i * S, S)
                         for i in range(N)])

                    def step_round(step):
                        blobs = [os.urandom(S) for _ in range(N)]
                        for i, b in enumerate(blobs):
                            g.upload(src + i * S, b)
                        assert gcl.batch_put_prepared(pb, cfg), (tag, step)
                        assert gcl.batch_get_prepared(gb), (tag, step)
                        for i, b in enumerate(blobs):
                            got = g.download(dst + i * S, S)
                            assert got == b, (tag, step, i)

                    # phase 1: under continuous epoch interference — every
                    # step must still be correct (sessions may never engage)
                    for step in range(10):
                        step_round(step)
                    quiet.wait(timeout=10)
                    # phase 2: interference gone — the session fast path
                    # must re-engage within a couple of steps
                    before = gcl.session_put_steps
                    for step in range(4):
                        step_round(100 + step)
                    assert gcl.session_put_steps >= before + 2, (
                        tag, before, gcl.session_put_steps)
                    c.close()
                    g.free(src)
                    g.free(dst)
                except Exception as e:  # surfaced after join
                    errs.append((tag, repr(e)))

            def intruder():
                try:
                    for k in range(30):
                        ks.put_start("intr%d" % k, 4096, bb.PlacementConfig())
                        ks.put_complete("intr%d" % k, checksum=k + 1)
                        ks.remove_object("intr%d" % k)  # bumps epoch
                        time.sleep(0.01)
                except Exception as e:
                    errs.append(("intruder", repr(e)))
                finally:
                    quiet.set()

            ts = [threading.Thread(target=worker, args=("cA", 1)),
                  threading.Thread(target=worker, args=("cB", 2)),
                  threading.Thread(target=intruder)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            assert not errs, errs
        finally:
            cl.stop()

    def test_replicated_session_fast_path(self):
        """replication=2 batches ride the session fast path too: one desc
        per copy (same source), both replicas rewritten in place each step,
        the shared digest stamped on both shards. Kill one worker at the
        end: the surviving replica still serves verified gets."""
        cl = Cluster(n_workers=2, pool_bytes=256 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        g = bb.core.gpu
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            gcl.set_placement_cache(True)
            N, S = 8, 256 * 1024
            src = g.malloc(N * S)
            dst = g.malloc(N * S)
            cfg = bb.PlacementConfig()
            cfg.replace = True
            cfg.replication = 2
            pb = bb.make_put_batch([("rs%02d" % i, src + i * S, S)
                                    for i in range(N)])
            gb = bb.make_get_batch([("rs%02d" % i, dst + i * S, S)
                                    for i in range(N)])
            ks = cl.keystone.service()
            for step in range(4):
                blobs = [os.urandom(S) for _ in range(N)]
                for i, b in enumerate(blobs):
                    g.upload(src + i * S, b)
                assert gcl.batch_put_prepared(pb, cfg), step
                assert gcl.batch_get_prepared(gb), step
                for i, b in enumerate(blobs):
                    assert g.download(dst + i * S, S) == b, (step, i)
            assert gcl.session_put_steps >= 2, gcl.session_put_steps
            info = ks.get_workers("rs03")
            assert len(info.copies) == 2
            assert info.checksum == g.checksum_cpu(blobs[3])
            workers = {cp.shards[0].worker_id for cp in info.copies}
            assert workers == {"w0", "w1"}
            for cp in info.copies:
                assert cp.shards[0].digest == info.checksum
            # replica failover: stop the worker holding copy 0, verified
            # gets still succeed from the surviving copy
            victim = info.copies[0].shards[0].worker_id
            cl.workers[int(victim[1])].stop()
            deadline = time.time() + 10
            while time.time() < deadline:
                cps = ks.get_workers("rs03").copies
                if all(cp.shards[0].worker_id != victim for cp in cps):
                    break
                time.sleep(0.1)
            st = gcl.batch_get_device(
                [("rs%02d" % i, dst + i * S, S) for i in range(N)],
                verify=True)
            assert st == [0] * N
            for i, b in enumerate(blobs):
                assert g.download(dst + i * S, S) == b, i
            c.close()
            g.free(src)
            g.free(dst)
        finally:
            cl.stop()

    def test_session_survives_worker_death(self):
        """A session bound to placements on a worker that DIES must degrade
        transparently: the keystone drops the dead worker's copies (epoch
        bump invalidates the session + placement cache), and the next put
        step re-places the whole batch on the surviving worker with zero
        caller-visible errors."""
        cl = Cluster(n_workers=2, pool_bytes=256 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        g = bb.core.gpu
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            gcl.set_placement_cache(True)
            N, S = 8, 256 * 1024
            src = g.malloc(N * S)
            dst = g.malloc(N * S)
            cfg = bb.PlacementConfig()
            cfg.replace = True
            cfg.preferred_worker = "w0"  # pin the session to the victim
            pb = bb.make_put_batch([("wd%02d" % i, src + i * S, S)
                                    for i in range(N)])
            gb = bb.make_get_batch([("wd%02d" % i, dst + i * S, S)
                                    for i in range(N)])
            for step in range(3):  # establish + ride the session
                blobs = [os.urandom(S) for _ in range(N)]
                for i, b in enumerate(blobs):
                    g.upload(src + i * S, b)
                assert gcl.batch_put_prepared(pb, cfg)
                assert gcl.batch_get_prepared(gb)
            assert gcl.session_put_steps >= 1
            ks = cl.keystone.service()
            sh = ks.get_workers("wd00").copies[0].shards[0]
            assert sh.worker_id == "w0"

            cl.workers[0].stop()  # heartbeat TTL 1s → declared dead
            deadline = time.time() + 10
            while time.time() < deadline:
                try:
                    if ks.get_workers("wd00").copies[0].shards[0].worker_id \
                            != "w0":
                        break  # re-replicated to w1 already
                except Exception:
                    break  # or dropped entirely (no surviving replicas)
                time.sleep(0.1)

            cfg2 = bb.PlacementConfig()
            cfg2.replace = True  # no preferred worker: place on survivors
            blobs = [os.urandom(S) for _ in range(N)]
            for i, b in enumerate(blobs):
                g.upload(src + i * S, b)
            assert gcl.batch_put_prepared(pb, cfg2)  # re-places, no error
            assert gcl.batch_get_prepared(gb)
            for i, b in enumerate(blobs):
                assert g.download(dst + i * S, S) == b, i
            assert ks.get_workers("wd00").copies[0].shards[0].worker_id == "w1"
            c.close()
            g.free(src)
            g.free(dst)
        finally:
            cl.stop()

    def test_one_shot_token_commit(self):
        """Even without a reusable session (cache off, replace off), an
        all-fused batch put commits by token + digests — BATCH_PUT_COMPLETE
        never re-sends the keys — and the one-shot token is released at
        commit. Data and digests stay correct."""
        cl = Cluster(n_workers=1, pool_bytes=256 * MB,
                     storage_class=bb.StorageClass.RAM_GPU)
        g = bb.core.gpu
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()  # placement cache OFF
            N, S = 16, 32 * 1024
            src = g.malloc(N * S)
            dst = g.malloc(N * S)
            blobs = [os.urandom(S) for _ in range(N)]
            for i, b in enumerate(blobs):
                g.upload(src + i * S, b)
            cfg = bb.PlacementConfig()
            cfg.replace = False
            cfg.checksum = True
            ks = cl.keystone.service()
            before = ks.token_commits()
            keys = ["ot%02d" % i for i in range(N)]
            assert gcl.batch_put_device(
                [(k, src + i * S, S) for i, k in enumerate(keys)],
                cfg) == [0] * N
            assert ks.token_commits() == before + 1
            assert gcl.batch_get_device(
                [(k, dst + i * S, S) for i, k in enumerate(keys)],
                verify=True) == [0] * N
            for i, b in enumerate(blobs):
                assert g.download(dst + i * S, S) == b, i
            info = ks.get_workers(keys[3])
            assert info.checksum == g.checksum_cpu(blobs[3])
            # replace=False still refuses overwrites after a token commit
            st = gcl.batch_put_device([(keys[0], src, S)], cfg)
            assert st[0] != 0
            c.batch_remove(keys)
            # fresh placements after remove: the one-shot path works again
            assert gcl.batch_put_device(
                [(k, src + i * S, S) for i, k in enumerate(keys)],
                cfg) == [0] * N
            assert ks.token_commits() == before + 2
            g.free(src)
            g.free(dst)
            c.close()
        finally:
            cl.stop()


class TestRcclShuffle:
    def test_two_rank_store_shuffle(self, tmp_path):
        """batch_shuffle_rccl end to end: two ranks put objects into their
        own HBM pools through the store, then exchange them with the RCCL
        all-to-all shuffle (needs >=2 devices; the 8-GPU driver environment
        runs it — the algorithm itself is covered CPU-side in
        test_shuffle.py)."""
        if bb.core.gpu.device_count() < 2:
            pytest.skip("needs >=2 GPUs (RCCL: one rank per device)")
        import subprocess, sys, textwrap
        script = tmp_path / "shuf2.py"
        script.write_text(textwrap.dedent(f"""
            import sys, os, time
            sys.path.insert(0, {repr(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))})
            import blackbird_amd as bb
            rank = int(sys.argv[1]); coord_ep = sys.argv[2]; ks_ep = sys.argv[3]
            g = bb.core.gpu
            S, N = 65536, 32
            coord = bb.CoordClient(); coord.connect(coord_ep)
            wc = bb.WorkerConfig()
            wc.worker_id = "w%d" % rank
            wc.coord_endpoint = coord_ep
            wc.data_listen_address = "127.0.0.1:0"
            pc = bb.PoolConfig(); pc.pool_id = "hbm%d" % rank
            pc.storage_class = bb.StorageClass.RAM_GPU
            pc.size_bytes = 64 << 20; pc.gpu_device_id = rank
            wc.pools = [pc]
            w = bb.WorkerService(wc); w.initialize(); w.start()
            o = bb.ClientOptions(); o.keystone_endpoint = ks_ep
            c = bb.Client(o)
            deadline = time.time() + 20
            while True:
                try:
                    c.connect()
                    if len(c.memory_pools()) >= 2: break
                except Exception: pass
                assert time.time() < deadline, "cluster did not assemble"
                time.sleep(0.05)
            gcl = bb.GpuClient(c, rank); gcl.init()
            gcl.set_placement_cache(True)
            cfg = bb.PlacementConfig()
            cfg.preferred_worker = "w%d" % rank
            src = g.malloc(N * S, rank)
            g.fill_pattern(src, N * S, seed=500 + rank)
            items = [("r%do%02d" % (rank, i), src + i * S, S) for i in range(N)]
            assert gcl.batch_put_device(items, cfg) == [0] * N
            # rendezvous then shuffle: each rank wants ALL peer objects
            e = bb.RcclEngine()
            e.init(coord, "shuftest", "t1", rank, 2, rank)
            peer = 1 - rank
            recv = g.malloc(N * S, rank)
            wants = [([], [], 0), ([], [], 0)]
            wants[peer] = (["r%do%02d" % (peer, i) for i in range(N)],
                           [S] * N, recv)
            bb.core.gpu_batch_shuffle(gcl, e, wants)
            # received bytes are the peer's fill pattern
            bad = g.verify_pattern(recv, N * S, seed=500 + peer)
            assert bad == 0, bad
            e.destroy()
            c.close(); w.stop()
            print("RANK", rank, "OK")
        """))
        cs = bb.CoordServer()
        cs.start("127.0.0.1", 0)
        ep = "127.0.0.1:%d" % cs.port
        kc = bb.KeystoneConfig()
        kc.listen_address = "127.0.0.1:0"
        kc.coord_endpoint = ep
        srv = bb.create_and_start_keystone(kc)
        try:
            procs = [subprocess.Popen(
                         [sys.executable, str(script), str(r), ep, srv.endpoint],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
                     for r in (0, 1)]
            for p in procs:
                out, _ = p.communicate(timeout=180)
                assert p.returncode == 0, out.decode()
                assert b"OK" in out
        finally:
            srv.stop()
            srv.service().stop()
            cs.stop()
