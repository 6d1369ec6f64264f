"""Striped batch sessions on the GPU: the hipGraph-replayed FusedStripePlan
against the CPU reference, and the GpuClient paths that ride it — striped put
sessions (two tiny RPCs around one replay), RPC-free verified gets of striped
placements from the cache, and striped get sessions."""
import os

import numpy as np
import pytest

import blackbird_amd as bb

from conftest import Cluster

pytestmark = pytest.mark.gpu

MB = 1 << 20
KB = 1 << 10
TILE = 1024
M64 = (1 << 64) - 1
PAD = 0xA5
CHECKSUM_MISMATCH = 5003  # ErrorCode::CHECKSUM_MISMATCH (common/error.h)
gpu = bb.core.gpu


def _rand(rng, n):
    return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()


def _slot(n):
    """Bytes a run of n takes in a gapped layout: 16B-aligned + a 16B gap."""
    return (n + 15) // 16 * 16 + 16


# ------------------------------------------------------------ the plan alone

class _PlanBatch:
    """One batch that meets every boundary of the walk. Segment k is
    (object, first_tile, nbytes); its bytes are object[first_tile * 1024:][:n].

      object 0  three segments: 3*depth + 1 full tiles (the pipelined steady
                loop is entered from 3*depth on), then 1 tile, then 777 B
      object 1  one whole-object segment (first_tile == 0: equal slots)
      object 2  segments listed out of order and interleaved with object 3's
      object 3  two segments, around a zero-length one
      object 4  16 bytes
    """

    def __init__(self):
        depth = gpu.digest_walk_depth()
        lead = 3 * depth + 1
        self.sizes = [(lead + 1) * TILE + 777, 5 * TILE + 333, 4 * TILE,
                      3 * TILE + 1, 16]
        self.segs = [
            (2, 2, 2 * TILE),          # object 2's tail first
            (0, 0, lead * TILE),
            (3, 0, TILE),
            (1, 0, self.sizes[1]),
            (2, 0, 2 * TILE),
            (3, 1, 0),                 # zero-length
            (0, lead + 1, 777),
            (3, 1, 2 * TILE + 1),
            (0, lead, TILE),
            (4, 0, 16),
        ]
        assert sum(self.sizes) < MB
        # below the grid rule's cap every wave owns `per` tiles: object 0's
        # first boundary must fall inside a wave's range, not between two
        total = sum((n + TILE - 1) // TILE for _, _, n in self.segs)
        waves = gpu.digest_grid_waves(total)
        per = (total + waves - 1) // waves
        assert waves > 4  # more than one block's worth of waves
        start = sum((n + TILE - 1) // TILE for o, _, n in self.segs[:1])
        assert (start + lead) % per != 0, (start, lead, per)
        self.obj_off, off = [], 0
        for n in self.sizes:
            self.obj_off.append(off)
            off += _slot(n)
        self.src_span = off
        self.seg_off, off = [], 0
        for _, _, n in self.segs:
            self.seg_off.append(off)
            off += _slot(n)
        self.dst_span = off

    def descs(self, src, dst):
        return [(src + self.obj_off[o] + ft * TILE, dst + so, n, ft, o)
                for (o, ft, n), so in zip(self.segs, self.seg_off)]

    def source(self, blobs):
        img = bytearray(b"\x5a" * self.src_span)
        for o, b in zip(self.obj_off, blobs):
            img[o:o + len(b)] = b
        return bytes(img)

    def expected(self, blobs):
        """(segment digests, object digests, destination image) from the CPU
        reference alone."""
        seg_want, img = [], bytearray(bytes([PAD]) * self.dst_span)
        for (o, ft, n), so in zip(self.segs, self.seg_off):
            data = blobs[o][ft * TILE:ft * TILE + n]
            assert len(data) == n
            seg_want.append(gpu.checksum_cpu(data))
            img[so:so + n] = data
        return seg_want, [gpu.checksum_cpu(b) for b in blobs], bytes(img)


def test_plan_replays_match_cpu_reference():
    """Three replays of one plan, the source rewritten before each: every
    replay gives its own digests bit for bit (a replay that accumulated on the
    previous step's sums would not), the destination holds the step's bytes
    and nothing past a segment; a one-shot fused_stripe agrees with the last
    replay."""
    pb = _PlanBatch()
    rng = np.random.default_rng(2024)
    steps = 3
    blobs = [[_rand(rng, n) for n in pb.sizes] for _ in range(steps)]
    want = [pb.expected(b) for b in blobs]
    assert len({tuple(w[1]) for w in want}) == steps
    src, dst = gpu.malloc(pb.src_span), gpu.malloc(pb.dst_span)
    try:
        seen = []

        def before(k):
            if k > 0:
                seen.append(gpu.download(dst, pb.dst_span))
            gpu.upload(src, pb.source(blobs[k]))
            gpu.upload(dst, bytes([PAD]) * pb.dst_span)

        descs = pb.descs(src, dst)
        got = gpu.fused_stripe_plan(descs, pb.sizes, steps, before_step=before)
        seen.append(gpu.download(dst, pb.dst_span))
        assert len(got) == steps
        for k, ((seg_got, obj_got), (seg_want, obj_want, img)) in enumerate(
                zip(got, want)):
            assert seg_got == seg_want, ("segments", k)
            assert obj_got == obj_want, ("objects", k)
            assert seen[k] == img, ("bytes", k)
        gpu.upload(dst, bytes([PAD]) * pb.dst_span)
        assert gpu.fused_stripe(descs, pb.sizes) == got[-1]
        assert gpu.download(dst, pb.dst_span) == want[-1][2]
    finally:
        gpu.free(src)
        gpu.free(dst)


# ----------------------------------------------------------------- the client

def _striped_cfg(replication=1):
    cfg = bb.PlacementConfig()
    cfg.max_workers_per_copy = 2
    cfg.replication = replication
    cfg.replace = True
    cfg.checksum = True
    return cfg


def _check_keystone(ks, key, blob, ncopies=1):
    """checksum and every shard's own digest equal the CPU reference."""
    info = ks.get_workers(key)
    assert info.checksum == gpu.checksum_cpu(blob), key
    assert len(info.copies) == ncopies
    for copy in info.copies:
        assert len(copy.shards) == 2
        off = 0
        for sh in copy.shards:
            assert sh.digest == gpu.checksum_cpu(blob[off:off + sh.length]), \
                (key, off)
            off += sh.length
        assert off == len(blob)


class _Rig:
    """Cluster of RAM_GPU workers, one client with the cache as asked, and
    prepared put/get batches over back-to-back device buffers."""

    def __init__(self, n_workers, sizes, cache=True, pool_bytes=64 * MB,
                 prefix="ss"):
        self.cl = Cluster(n_workers=n_workers, pool_bytes=pool_bytes,
                          storage_class=bb.StorageClass.RAM_GPU)
        self.c = self.cl.client()
        self.gcl = bb.GpuClient(self.c, 0)
        self.gcl.init()
        self.gcl.set_placement_cache(cache)
        self.ks = self.cl.keystone.service()
        self.sizes = sizes
        self.keys = ["%s%02d" % (prefix, i) for i in range(len(sizes))]
        self.offs, off = [], 0
        for n in sizes:
            self.offs.append(off)
            off += (n + 255) // 256 * 256
        self.src, self.dst = gpu.malloc(off), gpu.malloc(off)
        self.pb = bb.make_put_batch(
            [(k, self.src + o, n)
             for k, o, n in zip(self.keys, self.offs, sizes)])
        self.gb = bb.make_get_batch(
            [(k, self.dst + o, n)
             for k, o, n in zip(self.keys, self.offs, sizes)])

    def step(self, cfg, verify=False):
        """Fresh contents → prepared put → prepared get → bytes back."""
        blobs = [os.urandom(n) for n in self.sizes]
        for o, b in zip(self.offs, blobs):
            gpu.upload(self.src + o, b)
        assert self.gcl.batch_put_prepared(self.pb, cfg)
        assert self.gcl.batch_get_prepared(self.gb, verify)
        for i, (o, b) in enumerate(zip(self.offs, blobs)):
            assert gpu.download(self.dst + o, len(b)) == b, i
        return blobs

    def close(self):
        gpu.free(self.src)
        gpu.free(self.dst)
        self.c.close()
        self.cl.stop()


def test_striped_session_roundtrip_and_corruption():
    """Four 256 KiB objects over two shards: the first step establishes the
    put session (one-shot launch), later steps ride it; gets go RPC-free from
    the cache and then through the get session. Afterwards server-side
    interference ends the session transparently, and corruption inside a
    shard is pinned to its item by a verified get on the live get session."""
    rig = _Rig(2, [256 * KB] * 4)
    try:
        gcl, ks, cfg = rig.gcl, rig.ks, _striped_cfg()
        for _ in range(4):
            blobs = rig.step(cfg)
            for k, b in zip(rig.keys, blobs):
                _check_keystone(ks, k, b)
        assert gcl.session_put_steps >= 3, gcl.session_put_steps
        assert gcl.session_get_steps >= 2, gcl.session_get_steps
        assert ks.token_commits() >= 3
        if not os.environ.get("BB_NO_HIPGRAPH"):
            assert gcl.session_graph_steps >= 3, gcl.session_graph_steps
        assert ks.run_scrub_once() == 0
        # only the establishing step was a one-shot launch
        assert gcl.striped_fused_items == 4

        # server-side interference: removing ANY object bumps the placement
        # epoch → the session falls back transparently, still correct
        ks.put_start("intruder", 4096, bb.PlacementConfig())
        ks.put_complete("intruder", checksum=1)
        ks.remove_object("intruder")
        blobs = [os.urandom(n) for n in rig.sizes]
        for o, b in zip(rig.offs, blobs):
            gpu.upload(rig.src + o, b)
        fast_before = gcl.session_put_steps
        assert gcl.batch_put_prepared(rig.pb, cfg)   # full path this step
        assert gcl.session_put_steps == fast_before
        assert gcl.batch_put_prepared(rig.pb, cfg)   # session re-established
        assert gcl.session_put_steps == fast_before + 1
        gets_before = gcl.session_get_steps
        assert gcl.batch_get_prepared(rig.gb)
        for o, b in zip(rig.offs, blobs):
            assert gpu.download(rig.dst + o, len(b)) == b
        for k, b in zip(rig.keys, blobs):
            _check_keystone(ks, k, b)

        # corruption inside shard 1 of one object, get session live
        assert gcl.session_get_steps == gets_before + 1
        bad = ks.get_workers(rig.keys[2]).copies[0].shards[1]
        victim = next(w for w in rig.cl.workers
                      if any(p.pool_id == bad.pool_id
                             for p in w.pool_descriptors()))
        victim.backend(bad.pool_id).write(bad.offset + 4096, b"\x00" * 64)
        st = gcl.batch_get_prepared_statuses(rig.gb, verify=True)
        assert st == [0, 0, CHECKSUM_MISMATCH, 0]
    finally:
        rig.close()


@pytest.mark.parametrize("sizes,cache", [
    ([2 * MB + 1000], True),                       # shard 1 starts mid-tile
    ([256 * KB, 2 * MB + 1000, 256 * KB], True),   # one item on another route
    ([256 * KB] * 2, False),                       # cache off
])
def test_no_session_where_it_does_not_apply(sizes, cache):
    rig = _Rig(2, sizes, cache=cache, prefix="ns")
    try:
        cfg = _striped_cfg()
        for _ in range(3):
            blobs = rig.step(cfg, verify=True)
            for k, b in zip(rig.keys, blobs):
                info = rig.ks.get_workers(k)
                assert info.checksum == gpu.checksum_cpu(b), k
                assert len(info.copies[0].shards) == 2
        assert rig.gcl.session_put_steps == 0
        assert rig.ks.run_scrub_once() == 0
    finally:
        rig.close()


def test_replicated_and_striped_session():
    """Replication 2 over four workers, two shards per copy: session steps
    are taken, all four shard digests per object are right, and a host client
    that verifies on get reads the bytes back."""
    rig = _Rig(4, [128 * KB] * 2, prefix="rs")
    try:
        cfg = _striped_cfg(replication=2)
        for _ in range(3):
            blobs = rig.step(cfg)
            for k, b in zip(rig.keys, blobs):
                _check_keystone(rig.ks, k, b, ncopies=2)
        assert rig.gcl.session_put_steps >= 2, rig.gcl.session_put_steps
        assert rig.gcl.session_get_steps >= 1, rig.gcl.session_get_steps
        assert rig.ks.run_scrub_once() == 0
        hc = rig.cl.client(verify_checksum_on_get=True)
        try:
            for k, b in zip(rig.keys, blobs):
                assert hc.get(k) == b, k
        finally:
            hc.close()
    finally:
        rig.close()
