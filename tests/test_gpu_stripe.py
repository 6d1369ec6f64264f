"""fused_stripe on the GPU: the kernel against the CPU reference (segment
digests, object digests, bytes copied, nothing stored past a segment), and
the GpuClient striped put/get paths that ride it."""
import numpy as np
import pytest

import blackbird_amd as bb

from conftest import Cluster

pytestmark = pytest.mark.gpu

MB = 1 << 20
M64 = (1 << 64) - 1
PAD = 0xA5
CHECKSUM_MISMATCH = 5003  # ErrorCode::CHECKSUM_MISMATCH (common/error.h)
gpu = bb.core.gpu


def _rand(rng, n):
    return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()


def _slot(n):
    """Bytes a run of n takes in a gapped layout: 16B-aligned + a 16B gap."""
    return (n + 15) // 16 * 16 + 16


class _Seg:
    def __init__(self, obj, first_tile, data):
        self.obj, self.first_tile, self.data = obj, first_tile, data


def _split(obj, blob, lens):
    """Segments of one object cut at `lens` (tile-aligned but the last)."""
    out, off = [], 0
    for n in lens:
        assert off % 1024 == 0
        out.append(_Seg(obj, off // 1024, blob[off:off + n]))
        off += n
    assert off == len(blob)
    return out


def _expected(segs, obj_sizes):
    """Expected digests from the CPU reference alone."""
    seg_want = [gpu.checksum_cpu(s.data) for s in segs]
    sums = [0] * len(obj_sizes)
    for s in segs:
        sums[s.obj] = (sums[s.obj] +
                       gpu.checksum_cpu_tiles(s.data, s.first_tile)) & M64
    obj_want = [gpu.checksum_cpu_finalize(h, n) for h, n in zip(sums, obj_sizes)]
    return seg_want, obj_want


def _run_scatter(segs, obj_sizes):
    """Every segment's source and destination in its own gapped slot of one
    allocation each (sources 0x5A between them, destinations pre-filled with
    0xA5): digests exact, bytes landed, every other byte untouched."""
    offs, off = [], 0
    for s in segs:
        offs.append(off)
        off += _slot(len(s.data))
    span = max(off, 16)
    src_img = bytearray(b"\x5a" * span)
    dst_img = bytearray(bytes([PAD]) * span)
    for o, s in zip(offs, segs):
        src_img[o:o + len(s.data)] = s.data
        dst_img[o:o + len(s.data)] = s.data
    seg_want, obj_want = _expected(segs, obj_sizes)
    src, dst = gpu.malloc(span), gpu.malloc(span)
    try:
        gpu.upload(src, bytes(src_img))
        gpu.upload(dst, bytes([PAD]) * span)
        seg_got, obj_got = gpu.fused_stripe(
            [(src + o, dst + o, len(s.data), s.first_tile, s.obj)
             for o, s in zip(offs, segs)], obj_sizes)
        bad = [i for i, (g_, w) in enumerate(zip(seg_got, seg_want)) if g_ != w]
        assert len(seg_got) == len(segs) and not bad, ("segments", bad[:8])
        bad = [i for i, (g_, w) in enumerate(zip(obj_got, obj_want)) if g_ != w]
        assert len(obj_got) == len(obj_sizes) and not bad, ("objects", bad[:8])
        assert gpu.download(dst, span) == bytes(dst_img)
        return seg_got, obj_got
    finally:
        gpu.free(src)
        gpu.free(dst)


class TestFusedStripeKernel:
    def test_minimal_two_segment_object(self):
        blob = _rand(np.random.default_rng(1), 4096)
        _, obj = _run_scatter(_split(0, blob, [2048, 2048]), [4096])
        assert obj == [gpu.checksum_cpu(blob)]

    def test_tail_in_last_segment(self):
        blob = _rand(np.random.default_rng(2), 2048 + 1024 + 777)
        _, obj = _run_scatter(_split(0, blob, [2048, 1024, 777]), [len(blob)])
        assert obj == [gpu.checksum_cpu(blob)]

    def test_single_segments_equal_fused_put(self):
        """A segment that is its whole object: both digests are fused_put's."""
        rng = np.random.default_rng(3)
        sizes = [1, 1023, 1024, 1025]
        blobs = [_rand(rng, n) for n in sizes]
        segs = [_Seg(i, 0, b) for i, b in enumerate(blobs)]
        seg, obj = _run_scatter(segs, sizes)
        span = sum(_slot(n) for n in sizes)
        src, dst = gpu.malloc(span), gpu.malloc(span)
        try:
            descs, off = [], 0
            for b in blobs:
                gpu.upload(src + off, b)
                descs.append((src + off, dst + off, len(b)))
                off += _slot(len(b))
            put = gpu.fused_put(descs)
        finally:
            gpu.free(src)
            gpu.free(dst)
        assert seg == put and obj == put
        assert put == [gpu.checksum_cpu(b) for b in blobs]

    def test_many_small(self):
        """300 two-tile objects, all first halves then all second halves:
        every wave crosses segment boundaries, the object index jumps back."""
        rng = np.random.default_rng(4)
        blobs = [_rand(rng, 2048) for _ in range(300)]
        halves = [_split(i, b, [1024, 1024]) for i, b in enumerate(blobs)]
        segs = [h[0] for h in halves] + [h[1] for h in halves]
        _, obj = _run_scatter(segs, [2048] * 300)
        assert obj == [gpu.checksum_cpu(b) for b in blobs]

    def test_odd_lists(self):
        """Zero-length segments leading, in the middle and trailing; object 1
        has no segment at all: its digest is finalize(0, size)."""
        rng = np.random.default_rng(5)
        a, c = _rand(rng, 3072 + 5), _rand(rng, 2048)
        sa, sc = _split(0, a, [1024, 2048 + 5]), _split(2, c, [1024, 1024])
        segs = [_Seg(0, 0, b""), _Seg(2, 2, b""), sa[0], _Seg(0, 1, b""),
                _Seg(1, 0, b""), sc[1], sa[1], sc[0], _Seg(2, 1, b""),
                _Seg(1, 4, b"")]
        seg, obj = _run_scatter(segs, [len(a), 4096, len(c)])
        assert obj == [gpu.checksum_cpu(a),
                       gpu.checksum_cpu_finalize(0, 4096),
                       gpu.checksum_cpu(c)]
        assert seg[0] == gpu.checksum_cpu(b"")
        # nothing but empty segments: no tile at all
        seg, obj = gpu.fused_stripe([(16, 16, 0, 0, 0), (16, 16, 0, 1, 0)],
                                    [1024])
        assert seg == [gpu.checksum_cpu(b"")] * 2
        assert obj == [gpu.checksum_cpu_finalize(0, 1024)]

    def test_partial_coverage_large_first_tile(self):
        """Slot arithmetic is 64-bit: tile 2^40 of a 2^50-byte object."""
        data = _rand(np.random.default_rng(6), 2048)
        size = (1 << 50) + 2048
        _, obj = _run_scatter([_Seg(0, 1 << 40, data)], [size])
        want = gpu.checksum_cpu_finalize(
            gpu.checksum_cpu_tiles(data, 1 << 40), size)
        assert obj == [want]
        # the slots really are the far ones
        assert want != gpu.checksum_cpu_finalize(
            gpu.checksum_cpu_tiles(data, 0), size)

    def test_grid_cap(self):
        """Just over 32768 tiles: the 4096-block cap binds, several tiles per
        wave, segments end inside waves' ranges."""
        rng = np.random.default_rng(7)
        size = 11 * MB + 513
        blobs = [_rand(rng, size) for _ in range(3)]
        segs = []
        for i, b in enumerate(blobs):
            segs += _split(i, b, [3 * MB, 3 * MB, 3 * MB, 2 * MB + 513])
        assert sum((len(s.data) + 1023) // 1024 for s in segs) > 32768
        _, obj = _run_scatter(segs, [size] * 3)
        assert obj == [gpu.checksum_cpu(b) for b in blobs]

    def test_gather(self):
        """The get direction: every source its own allocation, the segments
        of an object land back to back in one buffer."""
        rng = np.random.default_rng(8)
        blobs = [_rand(rng, n) for n in (4096 + 333, 2048, 8192)]
        lens = [[2048, 2048, 333], [1024, 1024], [4096, 4096]]
        segs = []
        for i, (b, ln) in enumerate(zip(blobs, lens)):
            segs += _split(i, b, ln)
        segs = segs[::2] + segs[1::2]  # interleave the objects
        sizes = [len(b) for b in blobs]
        bases, off = [], 0
        for n in sizes:
            bases.append(off)
            off += _slot(n)
        span = off
        dst_img = bytearray(bytes([PAD]) * span)
        for o, b in zip(bases, blobs):
            dst_img[o:o + len(b)] = b
        seg_want, obj_want = _expected(segs, sizes)
        dst = gpu.malloc(span)
        srcs = []
        try:
            gpu.upload(dst, bytes([PAD]) * span)
            descs = []
            for s in segs:
                p = gpu.malloc(len(s.data) + 16)
                srcs.append(p)
                gpu.upload(p, s.data)
                descs.append((p, dst + bases[s.obj] + s.first_tile * 1024,
                              len(s.data), s.first_tile, s.obj))
            seg_got, obj_got = gpu.fused_stripe(descs, sizes)
            assert seg_got == seg_want
            assert obj_got == obj_want == [gpu.checksum_cpu(b) for b in blobs]
            assert gpu.download(dst, span) == bytes(dst_img)
        finally:
            gpu.free(dst)
            for p in srcs:
                gpu.free(p)

    def test_rejects_bad_segments_before_launch(self):
        buf = gpu.malloc(4096)
        try:
            with pytest.raises(Exception, match="INVALID_ARGUMENT"):
                gpu.fused_stripe([(buf, buf + 2048, 777, 0, 0)], [4096])
            assert gpu.fused_stripe([], []) == ([], [])
        finally:
            gpu.free(buf)


class TestGpuClientStripedFused:
    def _cluster(self):
        return Cluster(n_workers=2, pool_bytes=128 * MB,
                       storage_class=bb.StorageClass.RAM_GPU)

    def test_fused_striped_put_get_and_corruption(self):
        """Four 2 MiB objects striped over two HBM pools ride one
        fused_stripe launch each way: object and shard digests match the CPU
        reference, the scrubber agrees, host and device readers get the
        bytes back, and a verified batch get pins corruption to its item."""
        cl = self._cluster()
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            N, S = 4, 2 * MB
            blobs = [_rand(np.random.default_rng(100 + i), S) for i in range(N)]
            src, dst = gpu.malloc(N * S), gpu.malloc(N * S)
            for i, b in enumerate(blobs):
                gpu.upload(src + i * S, b)
            cfg = bb.PlacementConfig()
            cfg.max_workers_per_copy = 2
            cfg.checksum = True
            keys = ["sf%d" % i for i in range(N)]
            st = gcl.batch_put_device(
                [(k, src + i * S, S) for i, k in enumerate(keys)], cfg)
            assert st == [0] * N
            assert gcl.striped_fused_items == N
            ks = cl.keystone.service()
            for k, b in zip(keys, blobs):
                info = ks.get_workers(k)
                assert info.checksum == gpu.checksum_cpu(b), k
                shards = info.copies[0].shards
                assert len(shards) == 2
                off = 0
                for sh in shards:
                    assert sh.digest == gpu.checksum_cpu(
                        b[off:off + sh.length]), (k, off)
                    off += sh.length
                assert off == S
            assert ks.run_scrub_once() == 0
            hc = cl.client(verify_checksum_on_get=True)
            for k, b in zip(keys, blobs):
                assert hc.get(k) == b, k
            hc.close()
            gets = [(k, dst + i * S, S) for i, k in enumerate(keys)]
            assert gcl.batch_get_device(gets, verify=True) == [0] * N
            assert gcl.striped_fused_get_items == N
            for i, b in enumerate(blobs):
                assert gpu.download(dst + i * S, S) == b, i
            assert gcl.striped_fused_items == N  # gets count separately

            # corruption inside shard 1 of one object
            bad = ks.get_workers(keys[2]).copies[0].shards[1]
            victim = next(w for w in cl.workers
                          if any(p.pool_id == bad.pool_id
                                 for p in w.pool_descriptors()))
            victim.backend(bad.pool_id).write(bad.offset + 4096, b"\x00" * 64)
            st = gcl.batch_get_device(gets, verify=True)
            assert st == [0, 0, CHECKSUM_MISMATCH, 0]
            gpu.free(src)
            gpu.free(dst)
            c.close()
        finally:
            cl.stop()

    def test_unaligned_shards_keep_the_old_route(self):
        """2 MiB + 1000 B over two workers: shard 1 does not start on a tile
        boundary, so the item takes the three-pass route, unchanged."""
        cl = self._cluster()
        try:
            c = cl.client()
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            S = 2 * MB + 1000
            blob = _rand(np.random.default_rng(9), S)
            src, dst = gpu.malloc(S), gpu.malloc(S)
            gpu.upload(src, blob)
            cfg = bb.PlacementConfig()
            cfg.max_workers_per_copy = 2
            assert gcl.batch_put_device([("odd", src, S)], cfg) == [0]
            assert gcl.striped_fused_items == 0
            info = cl.keystone.service().get_workers("odd")
            assert len(info.copies[0].shards) == 2
            assert info.checksum == gpu.checksum_cpu(blob)
            assert gcl.batch_get_device([("odd", dst, S)], verify=True) == [0]
            assert gcl.striped_fused_get_items == 0
            assert gpu.download(dst, S) == blob
            gpu.free(src)
            gpu.free(dst)
            c.close()
        finally:
            cl.stop()
