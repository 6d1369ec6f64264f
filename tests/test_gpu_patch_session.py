"""Patch sessions on the GPU: gpu.fused_patch_plan, one captured patch step
replayed with other old digests and other bytes every time, against the CPU
reference; and GpuClient.batch_patch_prepared, whose steps after the first
ride a server session (start by token, one replay, commit by token), on
RAM_GPU clusters. Every expected digest is checksum_cpu of the patched bytes
computed from scratch; the pool bytes of the plan cases are compared whole,
gaps included.

The pool is laid out as in test_gpu_patch.py: every shard in a gapped
16-byte-aligned slot of one allocation, the gaps filled with 0xA5; the new
bytes sit in gapped slots of a second allocation, rewritten before every
replay."""
import os

import numpy as np
import pytest

import blackbird_amd as bb

from conftest import Cluster

pytestmark = pytest.mark.gpu

TILE = 1024
KB = 1024
PAD = 0xA5
CHECKSUM_MISMATCH = 5003  # ErrorCode values (common/error.h)
OBJECT_NOT_FOUND = 5000
gpu = bb.core.gpu


def _rand(seed, n):
    return np.random.default_rng(seed).bytes(n)


def _slot(n):
    return (n + 15) // 16 * 16 + 16


def _cut(blob, lens):
    out, off = [], 0
    for n in lens:
        out.append(blob[off:off + n])
        off += n
    assert off == len(blob)
    return out


class _Plan:
    """objs: [(old bytes, shard lengths)]; patches: [(obj, offset, length)],
    the same ranges every step with other bytes. Holds the device pool and
    source, the run list, and the expected state step by step."""

    def __init__(self, objs, patches, front=(), back=()):
        self.lens = [list(lens) for _, lens in objs]
        self.blobs = [blob for blob, _ in objs]
        self.patches = patches
        shard_base, shard_at, off = [], [], 0
        for lens in self.lens:
            shard_base.append(len(shard_at))
            for n in lens:
                shard_at.append(off)
                off += _slot(n)
        self.pool_span = max(off, 16)
        img = bytearray(bytes([PAD]) * self.pool_span)
        for i, blob in enumerate(self.blobs):
            for k, sh in enumerate(_cut(blob, self.lens[i])):
                at = shard_at[shard_base[i] + k]
                img[at:at + len(sh)] = sh
        self.img = img
        # (source offset, pool offset, nbytes, patch index, offset in patch)
        self.runs, self.pieces, soff = [], [], 0
        for j, (i, offset, length) in enumerate(patches):
            pieces = gpu.plan_patch(len(self.blobs[i]), self.lens[i], offset,
                                    length)
            assert pieces is not None, (i, offset, length)
            for k, shard_off, obj_off, n in pieces:
                at = shard_at[shard_base[i] + k] + shard_off
                self.runs.append((soff, at, n, shard_off // TILE,
                                  obj_off // TILE, shard_base[i] + k, i))
                self.pieces.append((soff, at, n, j, obj_off - offset))
                soff += _slot(n)
        self.src_span = max(soff, 16)
        self.front, self.back = list(front), list(back)
        self.shard_lens = [n for lens in self.lens for n in lens]
        self.obj_sizes = [len(b) for b in self.blobs]
        self.src = self.pool = None

    def __enter__(self):
        self.src, self.pool = gpu.malloc(self.src_span), gpu.malloc(self.pool_span)
        gpu.upload(self.src, b"\x5a" * self.src_span)
        gpu.upload(self.pool, bytes(self.img))
        return self

    def __exit__(self, *exc):
        gpu.free(self.src)
        gpu.free(self.pool)

    def segs(self):
        return (self.front +
                [(self.src + s, self.pool + d, n, st, ot, sh, ob)
                 for s, d, n, st, ot, sh, ob in self.runs] + self.back)

    def digests(self):
        """From scratch, of the bytes the objects hold now."""
        return ([gpu.checksum_cpu(sh) for b, lens in zip(self.blobs, self.lens)
                 for sh in _cut(b, lens)],
                [gpu.checksum_cpu(b) for b in self.blobs])

    def fresh_sources(self, seed):
        """New bytes for every patch: uploads them and moves the expected
        objects and pool image on by one step."""
        news = [_rand(seed * 1000 + j, n)
                for j, (_, _, n) in enumerate(self.patches)]
        src_img = bytearray(b"\x5a" * self.src_span)
        for soff, at, n, j, poff in self.pieces:
            src_img[soff:soff + n] = news[j][poff:poff + n]
            self.img[at:at + n] = news[j][poff:poff + n]
        gpu.upload(self.src, bytes(src_img))
        blobs = [bytearray(b) for b in self.blobs]
        for (i, offset, n), new in zip(self.patches, news):
            blobs[i][offset:offset + n] = new
        self.blobs = [bytes(b) for b in blobs]

    def pool_now(self):
        return gpu.download(self.pool, self.pool_span)

    def replay(self, steps, seed):
        """`steps` replays of one plan, fresh bytes before each; checks the
        pool after every replay and every digest of every step."""
        shard_old, obj_old = self.digests()
        want = []

        def before(k):
            if k > 0:  # what replay k-1 left behind
                assert self.pool_now() == bytes(self.img), ("pool", k - 1)
            self.fresh_sources(seed + k)
            want.append(self.digests())

        got = gpu.fused_patch_plan(self.segs(), self.shard_lens,
                                   self.obj_sizes, shard_old, obj_old, steps,
                                   before_step=before)
        assert self.pool_now() == bytes(self.img), ("pool", steps - 1)
        assert len(got) == steps
        for k, ((shard, obj), (shard_want, obj_want)) in enumerate(zip(got, want)):
            bad = [i for i, (g_, w) in enumerate(zip(shard, shard_want)) if g_ != w]
            assert len(shard) == len(shard_want) and not bad, (k, "shards", bad[:8])
            bad = [i for i, (g_, w) in enumerate(zip(obj, obj_want)) if g_ != w]
            assert len(obj) == len(obj_want) and not bad, (k, "objects", bad[:8])
        return got


def _mixed_plan():
    """Every shape of run in one launch (object index: what it is)."""
    objs = [
        (b"\x07", [1]),                                    # 0 one byte, whole
        (_rand(1, TILE), [TILE]),                          # 1 one tile, whole
        (_rand(2, 5 * TILE + 17), [5 * TILE + 17]),        # 2 run to its end
        (_rand(3, 5 * TILE + 1), [3 * TILE, 2 * TILE + 1]),  # 3 across shards
        (_rand(4, 8 * TILE), [8 * TILE]),                  # 4 two disjoint runs
        (_rand(5, 2 * TILE + 5), [2 * TILE + 5]),          # 5 no run names it
        (_rand(6, 4 * TILE), [2 * TILE, 2 * TILE]),        # 6 shard 1 unnamed
    ]
    patches = [(0, 0, 1), (1, 0, TILE), (2, 3 * TILE, 2 * TILE + 17),
               (3, 2 * TILE, 2 * TILE), (4, TILE, TILE), (4, 5 * TILE, 2 * TILE),
               (6, TILE, TILE)]
    # zero-length runs: (16, 16) are never dereferenced
    front = [(16, 16, 0, 0, 0, 0, 0), (16, 16, 0, 1, 4, 4, 3)]
    back = [(16, 16, 0, 2, 2, 7, 5), (0, 0, 0, 0, 0, 1, 1)]
    return _Plan(objs, patches, front, back)


class TestFusedPatchPlan:
    def test_four_replays_against_the_cpu_reference(self):
        with _mixed_plan() as p:
            start_shard, start_obj = p.digests()
            got = p.replay(4, seed=10)
            # the object and the shard no run names: bit for bit, every step
            for shard, obj in got:
                assert obj[5] == start_obj[5]
                assert shard[6] == start_shard[6]   # object 5's only shard
                assert shard[8] == start_shard[8]   # object 6, shard 1
            # and the steps did differ
            assert len({tuple(obj) for _, obj in got}) == 4

    def test_more_accumulators_than_one_finalize_block(self):
        objs = [(_rand(1000 + i, 2 * TILE), [2 * TILE]) for i in range(300)]
        with _Plan(objs, [(i, TILE, TILE) for i in range(300)]) as p:
            assert len(p.shard_lens) + len(p.obj_sizes) == 600
            p.replay(3, seed=20)

    def test_step_one_equals_the_one_shot_launch_bit_for_bit(self):
        with _mixed_plan() as p:
            shard_old, obj_old = p.digests()
            start = bytes(p.img)
            p.fresh_sources(30)
            one_shot = gpu.fused_patch(p.segs(), p.shard_lens, shard_old,
                                       p.obj_sizes, obj_old)
            assert p.pool_now() == bytes(p.img)
            gpu.upload(p.pool, start)
            planned = gpu.fused_patch_plan(p.segs(), p.shard_lens, p.obj_sizes,
                                           shard_old, obj_old, 1)
            assert p.pool_now() == bytes(p.img)
            assert planned == [one_shot]
            assert one_shot == p.digests()

    @pytest.mark.parametrize("which", ["shard", "object"])
    def test_zero_old_digest_at_run_launches_nothing(self, which):
        with _mixed_plan() as p:
            shard_old, obj_old = p.digests()
            start = bytes(p.img)
            p.fresh_sources(40)
            if which == "shard":
                shard_old[3] = 0
            else:
                obj_old[-1] = 0
            with pytest.raises(bb.core.BlackbirdError, match="INVALID_ARGUMENT"):
                gpu.fused_patch_plan(p.segs(), p.shard_lens, p.obj_sizes,
                                     shard_old, obj_old, 1)
            assert p.pool_now() == start


# ---------------------------------------------------------------- GpuClient

N, S = 8, 256 * KB
PATCH = 64 * KB
GRAPHS = "BB_NO_HIPGRAPH" not in os.environ


def _overlay(blob, offset, new):
    return blob[:offset] + new + blob[offset + len(new):]


def _check_keystone(cl, key, want, nshards, ncopies=1):
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


def _backend_of(cl, pool_id):
    w = next(w for w in cl.workers
             if any(p.pool_id == pool_id for p in w.pool_descriptors()))
    return w.backend(pool_id)


class _Rig:
    """A RAM_GPU cluster, a GpuClient, N keys of S bytes put through it, and
    device buffers for the new bytes and for reading back."""

    def __init__(self, n_workers, replication=1, striped=None):
        self.cl = Cluster(n_workers=n_workers, pool_bytes=64 << 20,
                          storage_class=bb.StorageClass.RAM_GPU)
        self.c = self.cl.client()
        self.gcl = bb.GpuClient(self.c, 0)
        self.gcl.init()
        self.svc = self.cl.keystone.service()
        self.cfg = bb.PlacementConfig()
        self.nshards = striped if striped else 1
        self.cfg.max_workers_per_copy = self.nshards
        self.cfg.replication = replication
        self.ncopies = replication
        self.bufs = [gpu.malloc(N * S) for _ in range(3)]
        self.src, self.dst, self.new = self.bufs
        self.keys = ["ps%d" % i for i in range(N)]
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

    def offset(self, i, base=96 * KB):
        """From 96 KiB on — across the shard boundary where striped; the last
        item ends at the object's end."""
        return base if i < N - 1 else S - PATCH

    def items(self, base=96 * KB):
        return [(k, self.offset(i, base), self.new + i * S, PATCH)
                for i, k in enumerate(self.keys)]

    def fresh(self, seed, base=96 * KB, skip=()):
        """Fresh new bytes in the device buffers; the expected blobs move on
        for every item not in `skip`."""
        for i in range(N):
            data = _rand(seed * 100 + i, PATCH)
            gpu.upload(self.new + i * S, data)
            if i not in skip:
                self.blobs[i] = _overlay(self.blobs[i], self.offset(i, base), data)

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

    def counters(self):
        g = self.gcl
        return (g.session_patch_steps, g.session_graph_steps,
                self.svc.token_commits(), g.patched_fused_items,
                g.patched_rewrite_items)

    def establish(self, seed=1):
        """Step one: the full path, which leaves a session."""
        batch = bb.core.make_patch_batch(self.items())
        assert batch.size == N and not batch.active
        before = self.counters()
        self.fresh(seed)
        assert self.gcl.batch_patch_prepared(batch) == [0] * N
        assert batch.active
        after = self.counters()
        assert after[0] == before[0]          # no session step yet
        assert after[3] == before[3] + N and after[4] == before[4]
        return batch

    def session_step(self, batch, seed):
        before = self.counters()
        self.fresh(seed)
        assert self.gcl.batch_patch_prepared(batch) == [0] * N
        after = self.counters()
        assert after[0] == before[0] + 1
        assert after[1] == before[1] + (1 if GRAPHS else 0)
        assert after[2] == before[2] + 1
        assert after[3] == before[3] + N and after[4] == before[4]
        assert batch.active


@pytest.fixture(params=[1, 2], ids=["one_worker", "two_workers_striped"])
def rig(request):
    r = _Rig(request.param, striped=request.param)
    try:
        yield r
    finally:
        r.close()


class TestGpuClientPatchSession:
    def test_three_session_steps_after_the_first(self, rig):
        batch = rig.establish()
        rig.check()
        for seed in (2, 3, 4):
            rig.session_step(batch, seed)
            rig.check()

    def test_another_writer_between_steps(self, rig):
        batch = rig.establish()
        rig.session_step(batch, 2)
        other_c = rig.cl.client()
        try:
            other = bb.GpuClient(other_c, 0)
            other.init()
            fresh = _rand(4242, S)
            gpu.upload(rig.src, fresh)
            cfg = bb.PlacementConfig()
            cfg.max_workers_per_copy = rig.nshards
            cfg.replace = True
            assert other.batch_put_device([(rig.keys[3], rig.src, S)], cfg) == [0]
            rig.blobs[3] = fresh
        finally:
            other_c.close()
        rig.fresh(3)
        assert rig.gcl.batch_patch_prepared(batch) == [0] * N
        rig.check()
        # and the step after, whichever route the last one took
        rig.fresh(4)
        assert rig.gcl.batch_patch_prepared(batch) == [0] * N
        rig.check()

    def test_removed_key_between_steps(self, rig):
        batch = rig.establish()
        rig.session_step(batch, 2)
        other = rig.cl.client()
        try:
            other.remove(rig.keys[2])
        finally:
            other.close()
        rig.fresh(3, skip=(2,))
        st = rig.gcl.batch_patch_prepared(batch)
        assert st == [0, 0, OBJECT_NOT_FOUND] + [0] * (N - 3)
        assert not batch.active
        rig.check(only=[i for i in range(N) if i != 2])

    def test_changed_item_list(self, rig):
        batch = rig.establish()
        rig.session_step(batch, 2)
        # the same batch object, its items now at another offset: the session
        # is bound to the old list, so the full path runs and leaves a
        # session on the new one
        base = 16 * KB
        batch.set_items(rig.items(base))
        before = rig.counters()
        rig.fresh(3, base)
        assert rig.gcl.batch_patch_prepared(batch) == [0] * N
        after = rig.counters()
        assert after[0] == before[0] and after[3] == before[3] + N
        assert batch.active
        rig.check()
        before = rig.counters()
        rig.fresh(4, base)
        assert rig.gcl.batch_patch_prepared(batch) == [0] * N
        assert rig.counters()[0] == before[0] + 1
        rig.check()
        # a new batch over the first list starts from the full path too
        again = bb.core.make_patch_batch(rig.items())
        rig.fresh(5)
        assert rig.gcl.batch_patch_prepared(again) == [0] * N
        assert again.active and rig.counters()[0] == before[0] + 1
        rig.check()

    def test_unaligned_item_leaves_no_session(self, rig):
        items = rig.items()
        k, _, ptr, _ = items[1]
        items[1] = (k, 1000, ptr, 3000)
        batch = bb.core.make_patch_batch(items)
        for seed in (1, 2):
            before = rig.counters()
            for i in range(N):
                data = _rand(seed * 100 + i, PATCH)
                gpu.upload(rig.new + i * S, data)
                if i == 1:
                    rig.blobs[i] = _overlay(rig.blobs[i], 1000, data[:3000])
                else:
                    rig.blobs[i] = _overlay(rig.blobs[i], rig.offset(i), data)
            assert rig.gcl.batch_patch_prepared(batch) == [0] * N
            after = rig.counters()
            assert not batch.active
            assert after[0] == before[0]
            assert after[3] == before[3] + N - 1
            assert after[4] == before[4] + 1
            rig.check()

    def test_corruption_outside_the_range_is_not_laundered(self, rig):
        batch = rig.establish()
        # one byte of key 5, well before the patched range, flipped in the pool
        sh = rig.svc.get_workers(rig.keys[5]).copies[0].shards[0]
        assert sh.length > 5000
        _backend_of(rig.cl, sh.pool_id).write(
            sh.offset + 5000, bytes([rig.blobs[5][5000] ^ 0x20]))
        rig.session_step(batch, 2)
        rig.session_step(batch, 3)
        # the recorded digests are those of the patched CLEAN bytes
        _check_keystone(rig.cl, rig.keys[5], rig.blobs[5], rig.nshards)
        st = rig.gcl.batch_get_device(
            [(k, rig.dst + i * S, S) for i, k in enumerate(rig.keys)],
            verify=True)
        assert st == [0] * 5 + [CHECKSUM_MISMATCH] + [0] * (N - 6)
        assert rig.svc.run_scrub_once() == 1


def test_diverged_replica_in_a_session_step():
    """Replication 2 with an established session; a bit of copy 1 flipped
    inside the patched range: the old terms subtracted differ, so the copies'
    new digests disagree. That key is cancelled, the others commit by key."""
    rig = _Rig(2, replication=2)
    try:
        batch = rig.establish()
        rig.check()
        sh = rig.svc.get_workers(rig.keys[4]).copies[1].shards[0]
        at = rig.offset(4) + 777
        _backend_of(rig.cl, sh.pool_id).write(
            sh.offset + at, bytes([rig.blobs[4][at] ^ 1]))
        rig.fresh(2, skip=(4,))
        st = rig.gcl.batch_patch_prepared(batch)
        assert st == [0] * 4 + [CHECKSUM_MISMATCH] + [0] * (N - 5)
        assert not rig.svc.object_exists(rig.keys[4])
        assert not batch.active
        rig.check(only=[i for i in range(N) if i != 4])
    finally:
        rig.close()
