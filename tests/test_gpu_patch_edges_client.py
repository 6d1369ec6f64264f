"""GpuClient.batch_patch_device at byte granularity
(set_patch_edge_tiles(True)) on RAM_GPU clusters: ranges that are not whole
tiles ride the one fused_patch launch, edge tiles composed on the GPU, and
establish and replay patch sessions. Every expected digest is checksum_cpu of
the patched bytes computed from scratch. With the option off the routes are
those of test_gpu_patch.py."""
import os

import numpy as np
import pytest

import blackbird_amd as bb

from conftest import Cluster

pytestmark = pytest.mark.gpu

KB = 1024
N, S = 8, 256 * KB
PATCH = 64 * KB
GRAPHS = "BB_NO_HIPGRAPH" not in os.environ
gpu = bb.core.gpu


def _rand(seed, n):
    return np.random.default_rng(seed).bytes(n)


def _overlay(blob, offset, new):
    return blob[:offset] + new + blob[offset + len(new):]


def _check_keystone(cl, key, want, nshards, ncopies=1):
    """Checksum and every shard digest are the CPU digests of `want`."""
    info = cl.keystone.service().get_workers(key)
    assert info.checksum == gpu.checksum_cpu(want), key
    assert len(info.copies) == ncopies
    for copy in info.copies:
        assert len(copy.shards) == nshards
        off = 0
        for sh in copy.shards:
            assert sh.digest == gpu.checksum_cpu(want[off:off + sh.length]), \
                (key, off)
            off += sh.length
        assert off == len(want)


class _Rig:
    """A RAM_GPU cluster, a GpuClient with the option on, N keys of S bytes
    put through it, and device buffers for new bytes and for reading back."""

    def __init__(self, n_workers, striped=1, replication=1, edge_tiles=True):
        self.cl = Cluster(n_workers=n_workers, pool_bytes=64 << 20,
                          storage_class=bb.StorageClass.RAM_GPU)
        self.c = self.cl.client()
        self.gcl = bb.GpuClient(self.c, 0)
        self.gcl.init()
        assert self.gcl.patch_edge_tiles is False  # the default
        self.gcl.set_patch_edge_tiles(edge_tiles)
        self.svc = self.cl.keystone.service()
        self.cfg = bb.PlacementConfig()
        self.cfg.max_workers_per_copy = striped
        self.cfg.replication = replication
        self.nshards, self.ncopies = striped, replication
        self.bufs = [gpu.malloc(N * S) for _ in range(3)]
        self.src, self.dst, self.new = self.bufs
        self.keys = ["pe%d" % i for i in range(N)]
        self.blobs = [_rand(300 + i, S) for i in range(N)]
        for i, b in enumerate(self.blobs):
            gpu.upload(self.src + i * S, b)
        assert self.gcl.batch_put_device(
            [(k, self.src + i * S, S) for i, k in enumerate(self.keys)],
            self.cfg) == [0] * N

    def close(self):
        for p in self.bufs:
            gpu.free(p)
        self.c.close()
        self.cl.stop()

    def check(self, only=None):
        """Keystone digests from scratch, a clean scrub, a verified get."""
        idx = list(range(N)) if only is None else only
        for i in idx:
            _check_keystone(self.cl, self.keys[i], self.blobs[i], self.nshards,
                            self.ncopies)
        assert self.svc.run_scrub_once() == 0
        assert self.gcl.batch_get_device(
            [(self.keys[i], self.dst + i * S, S) for i in idx],
            verify=True) == [0] * len(idx)
        for i in idx:
            assert gpu.download(self.dst + i * S, S) == self.blobs[i], i

    # 64 KiB from 96 KiB + 40 on: across the shard boundary where striped,
    # an edge at either end, the source in phase with the offset (40 % 16 = 8)
    OFFSET = 96 * KB + 40

    def items(self):
        return [(k, self.OFFSET, self.new + i * S + 8, PATCH)
                for i, k in enumerate(self.keys)]

    def fresh(self, seed):
        for i in range(N):
            data = _rand(seed * 100 + i, PATCH)
            gpu.upload(self.new + i * S + 8, data)
            self.blobs[i] = _overlay(self.blobs[i], self.OFFSET, data)

    def counters(self):
        g = self.gcl
        return (g.session_patch_steps, g.session_graph_steps,
                g.patched_fused_items, g.patched_rewrite_items)


@pytest.fixture(params=[1, 2], ids=["one_worker", "two_workers_striped"])
def rig(request):
    r = _Rig(request.param, striped=request.param)
    try:
        yield r
    finally:
        r.close()


def _three_items(rig):
    """The items of test_gpu_patch.py's rewrite-route test. Item 0: offset
    inside a tile, source in phase with it (1000 % 16 = 8); item 1:
    tile-aligned; item 2: a source that is not 16-byte aligned under a
    whole-tile range."""
    a, b = _rand(700, 3000), _rand(701, 4 * KB)
    gpu.upload(rig.new + 8, a)
    gpu.upload(rig.new + 8 * KB, b)
    items = [(rig.keys[0], 1000, rig.new + 8, len(a)),
             (rig.keys[1], 4 * KB, rig.new + 8 * KB, 4 * KB),
             (rig.keys[2], 4 * KB, rig.new + 8 * KB + 8, KB)]
    rig.blobs[0] = _overlay(rig.blobs[0], 1000, a)
    rig.blobs[1] = _overlay(rig.blobs[1], 4 * KB, b)
    rig.blobs[2] = _overlay(rig.blobs[2], 4 * KB, b[8:8 + KB])
    return items


def test_unaligned_item_rides_the_launch(rig):
    items = _three_items(rig)
    _, _, fused0, rewrite0 = rig.counters()
    assert rig.gcl.batch_patch_device(items) == [0, 0, 0]
    _, _, fused, rewrite = rig.counters()
    assert fused == fused0 + 2          # items 0 and 1
    assert rewrite == rewrite0 + 1      # item 2: its run's source is off by 8
    rig.check(only=[0, 1, 2])


def test_option_off_is_the_rewrite_route():
    """The parent's behaviour: the same items, the option left off."""
    rig = _Rig(1, edge_tiles=False)
    try:
        items = _three_items(rig)
        _, _, fused0, rewrite0 = rig.counters()
        assert rig.gcl.batch_patch_device(items) == [0, 0, 0]
        _, _, fused, rewrite = rig.counters()
        assert fused == fused0 + 1 and rewrite == rewrite0 + 2
        rig.check(only=[0, 1, 2])
        # and a batch of unaligned items alone leaves the launch counter be
        rig.fresh(5)
        _, _, fused0, rewrite0 = rig.counters()
        assert rig.gcl.batch_patch_device(rig.items()) == [0] * N
        _, _, fused, rewrite = rig.counters()
        assert fused == fused0 and rewrite == rewrite0 + N
        rig.check()
    finally:
        rig.close()


def test_small_ranges_and_object_ends(rig):
    """One byte, a row inside a tile, two edges and no run, the last byte,
    an unaligned start through to the object's end — one launch."""
    ranges = [(1, 1), (5000, 384), (1023, 2), (S - 1, 1), (S - 3000, 3000),
              (S // 2 - 7, 14), (0, 1023), (S // 2 - 1024 - 5, 2048 + 10)]
    items = []
    for i, (off, n) in enumerate(ranges):
        data = _rand(800 + i, n)
        at = rig.new + i * S + off % 16
        gpu.upload(at, data)
        items.append((rig.keys[i], off, at, n))
        rig.blobs[i] = _overlay(rig.blobs[i], off, data)
    _, _, fused0, rewrite0 = rig.counters()
    assert rig.gcl.batch_patch_device(items) == [0] * N
    _, _, fused, rewrite = rig.counters()
    assert fused == fused0 + N and rewrite == rewrite0
    rig.check()


def test_eight_keys_across_the_shard_boundary(rig):
    rig.fresh(1)
    _, _, fused0, rewrite0 = rig.counters()
    assert rig.gcl.batch_patch_device(rig.items()) == [0] * N
    _, _, fused, rewrite = rig.counters()
    assert fused == fused0 + N and rewrite == rewrite0
    rig.check()


def test_replicated():
    """replication=2 over two workers: every copy is a kernel object of its
    own with its own edges; both must carry the same digests."""
    rig = _Rig(2, replication=2)
    try:
        rig.fresh(2)
        _, _, fused0, rewrite0 = rig.counters()
        assert rig.gcl.batch_patch_device(rig.items()) == [0] * N
        _, _, fused, rewrite = rig.counters()
        assert fused == fused0 + N and rewrite == rewrite0
        rig.check()   # _check_keystone walks both copies
    finally:
        rig.close()


def test_session_of_unaligned_items(rig):
    """The first prepared call runs the full path and leaves a session; the
    next two replay it with rewritten sources."""
    batch = bb.core.make_patch_batch(rig.items())
    assert not batch.active
    steps0, graphs0, fused0, rewrite0 = rig.counters()
    rig.fresh(1)
    assert rig.gcl.batch_patch_prepared(batch) == [0] * N
    assert batch.active
    rig.check()
    for k, seed in enumerate((2, 3)):
        rig.fresh(seed)
        assert rig.gcl.batch_patch_prepared(batch) == [0] * N
        assert batch.active
        steps, graphs, fused, rewrite = rig.counters()
        assert steps == steps0 + k + 1
        assert graphs == graphs0 + (k + 1 if GRAPHS else 0)
        rig.check()
    steps, graphs, fused, rewrite = rig.counters()
    assert steps == steps0 + 2
    assert fused == fused0 + 3 * N and rewrite == rewrite0
    # the option turned off ends the session: the rewrite route again
    rig.gcl.set_patch_edge_tiles(False)
    rig.fresh(4)
    assert rig.gcl.batch_patch_prepared(batch) == [0] * N
    assert not batch.active
    assert rig.counters()[0] == steps and rig.counters()[3] == rewrite0 + N
    rig.check()
