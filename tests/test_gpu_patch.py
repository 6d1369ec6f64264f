"""fused_patch on the GPU: the kernel against the CPU reference, and the
GpuClient ranged calls that ride it (batch_patch_device,
batch_get_device_range) on RAM_GPU clusters. Every expected digest is
checksum_cpu of the patched bytes computed from scratch; the pool bytes of
the kernel cases are compared whole, gaps included.

Shards sit in gapped 16-byte-aligned slots of one allocation (the "pool"),
pre-filled with their real old content, the gaps with 0xA5; the new bytes sit
in gapped slots of a second allocation. With depth D (gpu.patch_walk_depth) a
run of full tiles inside a wave's range is walked one by one below 2*D tiles
and through prologue, first group and drain from 2*D on; it goes round the
steady loop from 3*D on. The grid rule gives a wave more than two tiles only
once its block cap binds, so the large launches are sized from
gpu.digest_grid_waves and D, as test_gpu_walk_pipeline.py sizes its own."""
import numpy as np
import pytest

import blackbird_amd as bb

pytestmark = pytest.mark.gpu

TILE = 1024
PAD = 0xA5
gpu = bb.core.gpu


def _rand(seed, n):
    return np.random.default_rng(seed).bytes(n)


def _slot(n):
    """Bytes a run of n takes in a gapped layout: 16B-aligned + a 16B gap."""
    return (n + 15) // 16 * 16 + 16


def _tiles(n):
    return (n + TILE - 1) // TILE


class _Obj:
    """An object's old bytes and how its one copy is cut into shards."""

    def __init__(self, blob, lens=None):
        self.blob = blob
        self.lens = [len(blob)] if lens is None else list(lens)
        assert sum(self.lens) == len(blob)

    def shards(self, blob=None):
        blob = self.blob if blob is None else blob
        out, off = [], 0
        for n in self.lens:
            out.append(blob[off:off + n])
            off += n
        return out


def _run_patch(objs, patches, front=(), back=(), in_pool=None, check=True):
    """Patches [(obj index, offset, new bytes)] in one fused_patch launch.
    front/back: raw zero-length runs put before and after the planned ones.
    in_pool: {obj index: bytes actually in the pool}, where they differ from
    the bytes the old digests were taken over. Returns (shard digests, object
    digests, expected patched blobs)."""
    # the pool: every shard in its own slot
    shard_base, shard_at, off = [], [], 0
    for o in objs:
        shard_base.append(len(shard_at))
        for n in o.lens:
            shard_at.append(off)
            off += _slot(n)
    pool_span = max(off, 16)
    pool_img = bytearray(bytes([PAD]) * pool_span)
    for i, o in enumerate(objs):
        held = o.blob if not in_pool or i not in in_pool else in_pool[i]
        for k, sh in enumerate(_Obj(held, o.lens).shards()):
            at = shard_at[shard_base[i] + k]
            pool_img[at:at + len(sh)] = sh
    shard_lens = [n for o in objs for n in o.lens]
    shard_old = [gpu.checksum_cpu(sh) for o in objs for sh in o.shards()]
    obj_sizes = [len(o.blob) for o in objs]
    obj_old = [gpu.checksum_cpu(o.blob) for o in objs]

    # the runs, their sources, and what the pool and the objects become
    want_img = bytearray(pool_img)
    patched = [bytearray(o.blob) for o in objs]
    runs, src_parts, soff = [], [], 0
    for i, offset, new in patches:
        o = objs[i]
        pieces = gpu.plan_patch(len(o.blob), o.lens, offset, len(new))
        assert pieces is not None, (i, offset, len(new))
        patched[i][offset:offset + len(new)] = new
        for k, shard_off, obj_off, n in pieces:
            data = new[obj_off - offset:obj_off - offset + n]
            at = shard_at[shard_base[i] + k] + shard_off
            want_img[at:at + n] = data
            runs.append((soff, at, n, shard_off // TILE, obj_off // TILE,
                         shard_base[i] + k, i))
            src_parts.append((soff, data))
            soff += _slot(n)
    src_span = max(soff, 16)
    src_img = bytearray(b"\x5a" * src_span)
    for at, data in src_parts:
        src_img[at:at + len(data)] = data

    src, pool = gpu.malloc(src_span), gpu.malloc(pool_span)
    try:
        gpu.upload(src, bytes(src_img))
        gpu.upload(pool, bytes(pool_img))
        segs = list(front)
        segs += [(src + s, pool + d, n, st, ot, sh, ob)
                 for s, d, n, st, ot, sh, ob in runs]
        segs += list(back)
        shard_got, obj_got = gpu.fused_patch(segs, shard_lens, shard_old,
                                             obj_sizes, obj_old)
        got_img = gpu.download(pool, pool_span)
    finally:
        gpu.free(src)
        gpu.free(pool)
    assert got_img == bytes(want_img), "pool bytes"
    patched = [bytes(p) for p in patched]
    if check:
        shard_want = [gpu.checksum_cpu(sh) for o, p in zip(objs, patched)
                      for sh in o.shards(p)]
        obj_want = [gpu.checksum_cpu(p) for p in patched]
        bad = [i for i, (g_, w) in enumerate(zip(shard_got, shard_want)) if g_ != w]
        assert len(shard_got) == len(shard_want) and not bad, ("shards", bad[:8])
        bad = [i for i, (g_, w) in enumerate(zip(obj_got, obj_want)) if g_ != w]
        assert len(obj_got) == len(obj_want) and not bad, ("objects", bad[:8])
    return shard_got, obj_got, patched


def _per_wave():
    """Per-wave tile count that takes the steady loop's back edge at least
    twice and leaves a remainder the depth does not divide."""
    depth = gpu.patch_walk_depth()
    per = 4 * depth + max(depth // 2, 1)
    assert per // depth - 2 >= 2
    assert depth == 1 or per % depth
    return per


_long = {}


def _long_blobs():
    """Old and new bytes of three long objects, made once: sized so that every
    wave of the grid as built owns exactly _per_wave() tiles when all of them
    are patched whole, with the inner boundaries inside waves' ranges."""
    if not _long:
        waves = gpu.digest_grid_waves(1 << 40)  # saturated at the grid's cap
        per = _per_wave()
        total = waves * per
        assert waves == gpu.digest_grid_waves(total)
        tiles = [total // 3 + 4, total // 3 + 3]
        tiles.append(total - sum(tiles))
        assert tiles[0] % per and (tiles[0] + tiles[1]) % per
        sizes = [tiles[0] * TILE, (tiles[1] - 1) * TILE + 17,
                 (tiles[2] - 1) * TILE + 1]
        _long["total"] = total
        _long["old"] = [_rand(900 + i, s) for i, s in enumerate(sizes)]
        _long["new"] = [_rand(910 + i, s) for i, s in enumerate(sizes)]
    return _long


class TestFusedPatchKernel:
    def test_one_byte_object(self):
        _run_patch([_Obj(b"\x07")], [(0, 0, b"\xf1")])

    def test_one_tile_object(self):
        _run_patch([_Obj(_rand(1, 1024))], [(0, 0, _rand(2, 1024))])

    @pytest.mark.parametrize("offset,length", [
        (0, 1024), (1024, 1024), (2048, 1024), (3072, 777), (1024, 2825),
        (0, 3849)])
    def test_tailed_object(self, offset, length):
        """3 KiB + 777 B: first tile, middle tiles, the tail alone, the
        middle through to the end, everything."""
        _run_patch([_Obj(_rand(3, 3849))], [(0, offset, _rand(4 + offset, length))])

    def test_two_disjoint_runs_in_one_shard(self):
        old = _rand(5, 8 * 1024 + 5)
        _run_patch([_Obj(old)], [(0, 1024, _rand(6, 2048)),
                                 (0, 6144, _rand(7, 2048 + 5))])

    def test_range_across_two_shards(self):
        """Shards of 4 KiB, 4 KiB and 2 KiB + 100 B; the range covers the end
        of shard 0 and the start of shard 1, where shard_tile != obj_tile.
        Shard 2 and the second object keep their digests."""
        a = _Obj(_rand(8, 10 * 1024 + 100), [4096, 4096, 2148])
        b = _Obj(_rand(9, 2048))
        shard, obj, _ = _run_patch([a, b], [(0, 3072, _rand(10, 3072))])
        assert shard[2] == gpu.checksum_cpu(a.shards()[2])
        assert shard[3] == obj[1] == gpu.checksum_cpu(b.blob)
        # and through to the end of the last shard, mid-tile
        _run_patch([a, b], [(0, 5120, _rand(11, 5120 + 100))])

    def test_whole_object_equals_fused_put(self):
        sizes = [1, 1023, 1024, 1025, 5 * 1024 + 1]
        olds = [_rand(20 + i, n) for i, n in enumerate(sizes)]
        news = [_rand(30 + i, n) for i, n in enumerate(sizes)]
        shard, obj, _ = _run_patch([_Obj(b) for b in olds],
                                   [(i, 0, b) for i, b in enumerate(news)])
        span = sum(_slot(n) for n in sizes)
        src, dst = gpu.malloc(span), gpu.malloc(span)
        try:
            descs, off = [], 0
            for b in news:
                gpu.upload(src + off, b)
                descs.append((src + off, dst + off, len(b)))
                off += _slot(len(b))
            put = gpu.fused_put(descs)
        finally:
            gpu.free(src)
            gpu.free(dst)
        assert shard == put and obj == put

    def test_zero_length_runs(self):
        """Leading, trailing and nothing else: a launch without a tile hands
        the old digests back."""
        o = _Obj(_rand(40, 4096 + 9), [2048, 2057])
        empty = [(16, 16, 0, 0, 0, 0, 0), (16, 16, 0, 1, 3, 1, 0)]
        _run_patch([o], [(0, 1024, _rand(41, 2048))],
                   front=empty, back=empty[::-1] + [(0, 0, 0, 2, 2, 0, 0)])
        shard, obj, _ = _run_patch([o], [], front=empty)
        assert shard == [gpu.checksum_cpu(s) for s in o.shards()]
        assert obj == [gpu.checksum_cpu(o.blob)]

    def test_many_small(self):
        """300 two-tile objects, the second tile of each patched: every wave
        crosses run boundaries and leaves the first tiles alone."""
        objs = [_Obj(_rand(1000 + i, 2048)) for i in range(300)]
        _run_patch(objs, [(i, 1024, _rand(2000 + i, 1024)) for i in range(300)])

    def test_short_runs_around_the_pipeline_depth(self):
        """Runs of 2D-1, 2D, 3D and 3D+1 full tiles (with and without a
        tail) where a wave owns two tiles: the one-by-one path."""
        d = gpu.patch_walk_depth()
        objs, patches = [], []
        for f in (2 * d - 1, 2 * d, 3 * d, 3 * d + 1):
            for tail in (0, 1023):
                n = f * TILE + tail
                objs.append(_Obj(_rand(50 + len(objs), n + 1024)))
                patches.append((len(objs) - 1, 1024, _rand(70 + len(objs), n)))
        _run_patch(objs, patches)

    def test_large_launch(self):
        """Every wave owns 4D tiles plus a remainder that D does not divide:
        steady loop, drain, one-by-one. The first object is striped, so its
        second run mixes twice per tile; the last ends on a 1-byte tail."""
        lb = _long_blobs()
        half = (len(lb["old"][0]) // 2 // TILE + 3) * TILE
        objs = [_Obj(lb["old"][0], [half, len(lb["old"][0]) - half]),
                _Obj(lb["old"][1]), _Obj(lb["old"][2])]
        patches = [(i, 0, b) for i, b in enumerate(lb["new"])]
        assert sum(_tiles(len(b)) for b in lb["new"]) == lb["total"]
        _run_patch(objs, patches)

    def test_large_launch_with_run_lengths_around_the_depth(self):
        """The same long runs with runs of 2D-1, 2D, 3D and 3D+1 full tiles
        between them: where waves own long ranges, these take the pipelined
        path and the switch between runs comes right behind prefetched tiles."""
        lb = _long_blobs()
        d = gpu.patch_walk_depth()
        objs = [_Obj(lb["old"][0])]
        patches = [(0, 0, lb["new"][0])]
        for k, f in enumerate((2 * d - 1, 2 * d, 3 * d, 3 * d + 1) * 2):
            n = f * TILE + (0 if k < 4 else 1)
            # the run starts at tile 2 of a two-shard object's second shard
            objs.append(_Obj(_rand(100 + k, 4096 + n), [2048, 2048 + n]))
            patches.append((len(objs) - 1, 4096, _rand(120 + k, n)))
            if k == 3:
                objs.append(_Obj(lb["old"][1]))
                patches.append((len(objs) - 1, 0, lb["new"][1]))
        objs.append(_Obj(lb["old"][2]))
        patches.append((len(objs) - 1, 0, lb["new"][2]))
        tiles = sum(_tiles(len(b)) for _, _, b in patches)
        waves = gpu.digest_grid_waves(tiles)
        assert (tiles + waves - 1) // waves >= _per_wave()
        _run_patch(objs, patches)

    def test_corruption_outside_the_range_is_not_laundered(self):
        """The patch reads and re-hashes only its own tiles. Old bytes with
        one flipped bit outside the range, digests taken over them: the new
        digest is that of the patched corrupt bytes, not of the patched clean
        ones. And with the digests recorded before the bit flipped in the
        pool, the new digest still is the clean one: it does not match what
        the pool holds, so the corruption stays detectable."""
        clean = _rand(60, 8192)
        corrupt = bytearray(clean)
        corrupt[5000] ^= 0x04
        corrupt = bytes(corrupt)
        new = _rand(61, 2048)
        want_clean = gpu.checksum_cpu(clean[:1024] + new + clean[3072:])
        want_corrupt = gpu.checksum_cpu(corrupt[:1024] + new + corrupt[3072:])
        assert want_clean != want_corrupt
        shard, obj, _ = _run_patch([_Obj(corrupt)], [(0, 1024, new)])
        assert obj == [want_corrupt] and shard == [want_corrupt]
        assert obj != [want_clean]
        shard, obj, _ = _run_patch([_Obj(clean)], [(0, 1024, new)],
                                   in_pool={0: corrupt}, check=False)
        assert obj == [want_clean] and shard == [want_clean]
        assert obj != [want_corrupt]

    def test_rejects_bad_runs_before_launch(self):
        buf = gpu.malloc(8192)
        try:
            with pytest.raises(Exception, match="INVALID_ARGUMENT"):
                # two runs on one shard tile
                gpu.fused_patch([(buf, buf + 4096, 1024, 0, 0, 0, 0),
                                 (buf + 1024, buf + 4096, 1024, 0, 0, 0, 0)],
                                [4096], [1], [4096], [1])
            assert gpu.download(buf, 16) is not None
        finally:
            gpu.free(buf)


# ---------------------------------------------------------------- GpuClient

from conftest import Cluster  # noqa: E402

KB = 1024
CHECKSUM_MISMATCH = 5003  # ErrorCode::CHECKSUM_MISMATCH (common/error.h)
INVALID_ARGUMENT = 6000


def _overlay(blob, offset, new):
    return blob[:offset] + new + blob[offset + len(new):]


def _check_keystone(cl, key, want, nshards):
    """Checksum and every shard digest are the CPU digests of `want`."""
    info = cl.keystone.service().get_workers(key)
    assert info.checksum == gpu.checksum_cpu(want), key
    for copy in info.copies:
        assert len(copy.shards) == nshards
        off = 0
        for sh in copy.shards:
            assert sh.digest == gpu.checksum_cpu(want[off:off + sh.length]), \
                (key, off)
            off += sh.length
        assert off == len(want)


@pytest.fixture(params=[1, 2], ids=["one_worker", "two_workers_striped"])
def gpu_cluster(request):
    """RAM_GPU pools; with two workers every object is striped over both."""
    cl = Cluster(n_workers=request.param, pool_bytes=64 << 20,
                 storage_class=bb.StorageClass.RAM_GPU)
    c = cl.client()
    gcl = bb.GpuClient(c, 0)
    gcl.init()
    cfg = bb.PlacementConfig()
    cfg.max_workers_per_copy = request.param
    try:
        yield cl, gcl, cfg, request.param
    finally:
        c.close()
        cl.stop()


class TestGpuClientRanged:
    N, S = 8, 256 * KB

    def _put(self, gcl, cfg, src, seed):
        blobs = [_rand(seed + i, self.S) for i in range(self.N)]
        keys = ["rk%d" % i for i in range(self.N)]
        for i, b in enumerate(blobs):
            gpu.upload(src + i * self.S, b)
        assert gcl.batch_put_device(
            [(k, src + i * self.S, self.S) for i, k in enumerate(keys)],
            cfg) == [0] * self.N
        return keys, blobs

    def test_batch_patch_device(self, gpu_cluster):
        """8 keys, 64 KiB each from 96 KiB on — across the shard boundary
        where striped — in one launch; the last item ends at the object's
        end."""
        cl, gcl, cfg, nshards = gpu_cluster
        N, S = self.N, self.S
        src, dst, new = gpu.malloc(N * S), gpu.malloc(N * S), gpu.malloc(N * S)
        try:
            keys, blobs = self._put(gcl, cfg, src, 300)
            items, want = [], []
            for i, (k, b) in enumerate(zip(keys, blobs)):
                off = 96 * KB if i < N - 1 else S - 64 * KB
                data = _rand(400 + i, 64 * KB)
                gpu.upload(new + i * S, data)
                items.append((k, off, new + i * S, len(data)))
                want.append(_overlay(b, off, data))
            fused0, rewrite0 = gcl.patched_fused_items, gcl.patched_rewrite_items
            assert gcl.batch_patch_device(items) == [0] * N
            assert gcl.patched_fused_items == fused0 + N
            assert gcl.patched_rewrite_items == rewrite0
            for k, w in zip(keys, want):
                _check_keystone(cl, k, w, nshards)
            assert cl.keystone.service().run_scrub_once() == 0
            assert gcl.batch_get_device(
                [(k, dst + i * S, S) for i, k in enumerate(keys)],
                verify=True) == [0] * N
            for i, w in enumerate(want):
                assert gpu.download(dst + i * S, S) == w, i
            # per-item failures: a missing key and a range past the end
            # change nothing and do not disturb their neighbours
            data = _rand(500, 2 * KB)
            gpu.upload(new, data)
            st = gcl.batch_patch_device([("nope", 0, new, KB),
                                         (keys[0], 0, new, 2 * KB),
                                         (keys[1], S - KB, new, 2 * KB)])
            assert st == [5000, 0, INVALID_ARGUMENT]
            _check_keystone(cl, keys[0], _overlay(want[0], 0, data), nshards)
            _check_keystone(cl, keys[1], want[1], nshards)
        finally:
            for p in (src, dst, new):
                gpu.free(p)

    def test_unaligned_item_rides_the_rewrite_route(self, gpu_cluster):
        cl, gcl, cfg, nshards = gpu_cluster
        N, S = self.N, self.S
        src, dst, new = gpu.malloc(N * S), gpu.malloc(S), gpu.malloc(S)
        try:
            keys, blobs = self._put(gcl, cfg, src, 600)
            a, b = _rand(700, 3000), _rand(701, 4 * KB)
            gpu.upload(new, a)
            gpu.upload(new + 8 * KB, b)
            fused0, rewrite0 = gcl.patched_fused_items, gcl.patched_rewrite_items
            # item 0: offset inside a tile; item 1: tile-aligned, rides the
            # launch; item 2: a source that is not 16-byte aligned
            st = gcl.batch_patch_device([(keys[0], 1000, new, len(a)),
                                         (keys[1], 4 * KB, new + 8 * KB, 4 * KB),
                                         (keys[2], 4 * KB, new + 8 * KB + 8, KB)])
            assert st == [0, 0, 0]
            assert gcl.patched_rewrite_items == rewrite0 + 2
            assert gcl.patched_fused_items == fused0 + 1
            want = [_overlay(blobs[0], 1000, a), _overlay(blobs[1], 4 * KB, b),
                    _overlay(blobs[2], 4 * KB, b[8:8 + KB])]
            for k, w in zip(keys, want):
                _check_keystone(cl, k, w, nshards)
                assert gcl.batch_get_device([(k, dst, S)], verify=True) == [0]
                assert gpu.download(dst, S) == w, k
            assert cl.keystone.service().run_scrub_once() == 0
        finally:
            for p in (src, dst, new):
                gpu.free(p)

    def test_batch_get_device_range(self, gpu_cluster):
        cl, gcl, cfg, nshards = gpu_cluster
        N, S = self.N, self.S
        src, dst = gpu.malloc(N * S), gpu.malloc(N * S)
        try:
            keys, blobs = self._put(gcl, cfg, src, 800)
            half = S // 2
            ranges = [(0, 1), (1, 1023), (1023, 2), (half - 1, 2),
                      (half - 1000, 3001), (S - 1, 1), (3, S - 3), (S, 0)]
            gpu.upload(dst, bytes([PAD]) * (N * S))
            items = [(k, off, dst + i * S, n)
                     for i, (k, (off, n)) in enumerate(zip(keys, ranges))]
            assert gcl.batch_get_device_range(items) == [0] * N
            for i, (b, (off, n)) in enumerate(zip(blobs, ranges)):
                got = gpu.download(dst + i * S, S)
                assert got[:n] == b[off:off + n], i
                assert got[n:] == bytes([PAD]) * (S - n), i  # nothing past it
            st = gcl.batch_get_device_range([(keys[0], S - 1, dst, 2),
                                             ("nope", 0, dst, 1),
                                             (keys[1], 5, dst + 16, 7)])
            assert st == [INVALID_ARGUMENT, 5000, 0]
            assert gpu.download(dst + 16, 7) == blobs[1][5:12]
            gcl.get_device_range(keys[2], half - 3, dst, 6)
            assert gpu.download(dst, 6) == blobs[2][half - 3:half + 3]
        finally:
            gpu.free(src)
            gpu.free(dst)

    def test_cached_verified_get_after_a_patch(self, gpu_cluster):
        """The patching client's own placement cache must not serve the old
        digest: a verified cached get after the patch returns the new bytes."""
        cl, gcl, cfg, nshards = gpu_cluster
        N, S = self.N, self.S
        gcl.set_placement_cache(True)
        src, dst, new = gpu.malloc(N * S), gpu.malloc(N * S), gpu.malloc(4 * KB)
        try:
            keys, blobs = self._put(gcl, cfg, src, 900)
            gets = [(k, dst + i * S, S) for i, k in enumerate(keys)]
            assert gcl.batch_get_device(gets, verify=True) == [0] * N  # cached
            data = _rand(950, 4 * KB)
            gpu.upload(new, data)
            assert gcl.batch_patch_device([(keys[3], 8 * KB, new, 4 * KB)]) == [0]
            assert gcl.batch_get_device(gets, verify=True) == [0] * N
            for i, b in enumerate(blobs):
                w = _overlay(b, 8 * KB, data) if i == 3 else b
                assert gpu.download(dst + i * S, S) == w, i
        finally:
            for p in (src, dst, new):
                gpu.free(p)

    def test_diverged_replica_is_a_checksum_mismatch(self):
        """Two copies, one with a flipped bit inside the patched range: the
        old terms subtracted differ, so the copies' new digests disagree."""
        cl = Cluster(n_workers=2, pool_bytes=64 << 20,
                     storage_class=bb.StorageClass.RAM_GPU)
        c = cl.client()
        try:
            gcl = bb.GpuClient(c, 0)
            gcl.init()
            S = 64 * KB
            blob = _rand(970, S)
            src = gpu.malloc(S)
            gpu.upload(src, blob)
            cfg = bb.PlacementConfig()
            cfg.replication = 2
            assert gcl.batch_put_device([("rep", src, S)], cfg) == [0]
            sh = cl.keystone.service().get_workers("rep").copies[1].shards[0]
            w = next(w for w in cl.workers
                     if any(p.pool_id == sh.pool_id for p in w.pool_descriptors()))
            w.backend(sh.pool_id).write(sh.offset + 5000,
                                        bytes([blob[5000] ^ 1]))
            assert gcl.batch_patch_device([("rep", 4 * KB, src, 4 * KB)]) == \
                [CHECKSUM_MISMATCH]
            assert not cl.keystone.service().object_exists("rep")
            gpu.free(src)
        finally:
            c.close()
            cl.stop()
