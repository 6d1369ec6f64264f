"""Byte-granular in-place patches on the GPU: gpu.fused_patch and
gpu.fused_patch_plan with edge tiles (fused_patch_edge_kernel) against the CPU
reference. Every expected digest is checksum_cpu of the patched bytes computed
from scratch; the pool allocation is compared whole, gaps included.

The pool is laid out as in test_gpu_patch.py: every shard in a gapped
16-byte-aligned slot of one allocation, the gaps filled with 0xA5. A patch's
new bytes sit in a gapped slot of a second allocation at slot + offset % 16,
so that the interior run's source shares its phase with the pool address; the
edges ask for nothing. Ranges are planned with gpu.plan_patch_bytes."""
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
    return (n + 15) // 16 * 16 + 16


def _cut(blob, lens):
    out, off = [], 0
    for n in lens:
        out.append(blob[off:off + n])
        off += n
    assert off == len(blob)
    return out


class _Rig:
    """objs: [(old bytes, shard lengths)]; patches: [(obj, offset, length)],
    the same ranges every step with other bytes. flips: [(obj, byte)], one bit
    flipped in the pool but not in the bytes the old digests are taken over.
    src_phase: where in its slot a patch's source starts, instead of
    offset % 16. Holds the device pool and source, the run and edge lists, and
    the expected pool image and objects step by step."""

    def __init__(self, objs, patches, flips=(), src_phase=None):
        self.lens = [list(lens) for _, lens in objs]
        self.blobs = [blob for blob, _ in objs]
        self.patches = patches
        self.shard_base, self.shard_at, off = [], [], 0
        for lens in self.lens:
            self.shard_base.append(len(self.shard_at))
            for n in lens:
                self.shard_at.append(off)
                off += _slot(n)
        self.pool_span = max(off, 16)
        self.img = bytearray(bytes([PAD]) * self.pool_span)
        for i, blob in enumerate(self.blobs):
            self._write(i, 0, blob)
        for i, at in flips:
            self._write(i, at, bytes([self.blobs[i][at] ^ 0x10]))
        # descriptors with offsets for addresses
        self.runs, self.edges, self.src_at, soff = [], [], [], 0
        for i, offset, length in patches:
            plan = gpu.plan_patch_bytes(len(self.blobs[i]), self.lens[i],
                                        offset, length)
            assert plan is not None, (i, offset, length)
            phase = offset % 16 if src_phase is None else src_phase
            base = soff + phase
            self.src_at.append(base)
            soff += _slot(length + 16)
            for k, shard_off, obj_off, n in plan[0]:
                sh = self.shard_base[i] + k
                self.runs.append((base + obj_off - offset,
                                  self.shard_at[sh] + shard_off, n,
                                  shard_off // TILE, obj_off // TILE, sh, i))
            for k, st, ot, lo, hi, valid, src_off in plan[1]:
                sh = self.shard_base[i] + k
                self.edges.append((base + src_off,
                                   self.shard_at[sh] + st * TILE, lo, hi, valid,
                                   st, ot, sh, i))
        self.src_span = max(soff, 16)
        self.shard_lens = [n for lens in self.lens for n in lens]
        self.obj_sizes = [len(b) for b in self.blobs]
        self.src = self.pool = None

    def _write(self, i, offset, data):
        """data over object i's bytes from offset on, in the pool image."""
        start = 0
        for k, n in enumerate(self.lens[i]):
            lo, hi = max(start, offset), min(start + n, offset + len(data))
            if lo < hi:
                at = self.shard_at[self.shard_base[i] + k] + lo - start
                self.img[at:at + hi - lo] = data[lo - offset:hi - offset]
            start += n

    def __enter__(self):
        self.src, self.pool = gpu.malloc(self.src_span), gpu.malloc(self.pool_span)
        gpu.upload(self.src, b"\x5a" * self.src_span)
        gpu.upload(self.pool, bytes(self.img))
        return self

    def __exit__(self, *exc):
        gpu.free(self.src)
        gpu.free(self.pool)

    def segs(self):
        return [(self.src + s, self.pool + d, n, st, ot, sh, ob)
                for s, d, n, st, ot, sh, ob in self.runs]

    def edge_list(self):
        return [(self.src + s, self.pool + t, lo, hi, valid, st, ot, sh, ob)
                for s, t, lo, hi, valid, st, ot, sh, ob in self.edges]

    def digests(self):
        """From scratch, of the bytes the objects should hold now."""
        return ([gpu.checksum_cpu(sh) for b, lens in zip(self.blobs, self.lens)
                 for sh in _cut(b, lens)],
                [gpu.checksum_cpu(b) for b in self.blobs])

    def pool_digests(self):
        """From scratch, of the objects as the pool image holds them."""
        out = []
        for i, lens in enumerate(self.lens):
            parts = []
            for k, n in enumerate(lens):
                at = self.shard_at[self.shard_base[i] + k]
                parts.append(bytes(self.img[at:at + n]))
            out.append(gpu.checksum_cpu(b"".join(parts)))
        return out

    def fresh_sources(self, seed):
        """New bytes for every patch: uploads them and moves the expected
        objects and pool image on by one step."""
        src_img = bytearray(b"\x5a" * self.src_span)
        blobs = [bytearray(b) for b in self.blobs]
        for j, (i, offset, n) in enumerate(self.patches):
            new = _rand(seed * 1000 + j, n)
            src_img[self.src_at[j]:self.src_at[j] + n] = new
            blobs[i][offset:offset + n] = new
            self._write(i, offset, new)
        gpu.upload(self.src, bytes(src_img))
        self.blobs = [bytes(b) for b in blobs]

    def pool_now(self):
        return gpu.download(self.pool, self.pool_span)

    def _compare(self, got, want, tag=""):
        for name, g, w in zip(("shards", "objects"), got, want):
            bad = [i for i, (a, b) in enumerate(zip(g, w)) if a != b]
            assert len(g) == len(w) and not bad, (tag, name, bad[:8])

    def patch(self, seed=1, check=True):
        """One fused_patch launch with fresh bytes."""
        shard_old, obj_old = self.digests()
        self.fresh_sources(seed)
        got = gpu.fused_patch(self.segs(), self.shard_lens, shard_old,
                              self.obj_sizes, obj_old, edges=self.edge_list())
        assert self.pool_now() == bytes(self.img), "pool bytes"
        if check:
            self._compare(got, self.digests())
        return got

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
                                   before_step=before, edges=self.edge_list())
        assert self.pool_now() == bytes(self.img), ("pool", steps - 1)
        assert len(got) == steps
        for k, (g, w) in enumerate(zip(got, want)):
            self._compare(g, w, k)
        return got


def _one(size, offset, length, lens=None, seed=0):
    objs = [(_rand(100 + seed, size), lens or [size])]
    with _Rig(objs, [(0, offset, length)]) as r:
        got = r.patch(seed + 1)
    return r, got


INSIDE_ONE_TILE = [(1, 1), (1000, 23), (0, 1023), (1, 1023), (2048 + 5, 7)]


class TestEdgeKernel:
    @pytest.mark.parametrize("offset,length", INSIDE_ONE_TILE)
    def test_inside_one_tile(self, offset, length):
        r, _ = _one(4096, offset, length)
        assert r.runs == [] and len(r.edges) == 1

    def test_edges_alone_in_one_launch(self):
        """The same five ranges in five objects, no run in the launch; a
        sixth object is not named and keeps its digests bit for bit."""
        objs = [(_rand(110 + i, 4096), [4096]) for i in range(6)]
        patches = [(i, o, n) for i, (o, n) in enumerate(INSIDE_ONE_TILE)]
        with _Rig(objs, patches) as r:
            assert r.runs == [] and len(r.edges) == 5
            shard, obj = r.patch(2)
            assert shard[5] == obj[5] == gpu.checksum_cpu(objs[5][0])

    @pytest.mark.parametrize("offset,length,nrun", [
        (1023, 2, 0),        # no interior
        (2047, 1026, 1)])    # one byte either side of one whole tile
    def test_two_edges_around_a_boundary(self, offset, length, nrun):
        r, _ = _one(4096, offset, length)
        assert len(r.runs) == nrun and len(r.edges) == 2

    @pytest.mark.parametrize("size,offset,length,nrun,nedge", [
        (4096, 1000, 1048, 1, 1),     # head only
        (4096, 1024, 777, 0, 1),      # tail only, mid-object
        (8192, 1000, 3000, 1, 2)])    # both, with an interior
    def test_head_tail_and_interior(self, size, offset, length, nrun, nedge):
        r, _ = _one(size, offset, length)
        assert (len(r.runs), len(r.edges)) == (nrun, nedge)

    @pytest.mark.parametrize("offset,length", [
        (4999, 1), (4106, 100), (4090, 910), (4095, 2)])
    def test_last_partial_tile(self, offset, length):
        """5000 bytes: the last tile holds 904. Nothing behind the object is
        read into the digest or written: the gap keeps its fill."""
        r, _ = _one(5000, offset, length)
        # the short tile is an edge's, or the tail of the run behind the edge
        assert any(e[4] == 904 for e in r.edges) or \
            any(s[2] % TILE == 904 for s in r.runs)

    @pytest.mark.parametrize("offset,length", [
        (2000, 100),     # across the shard boundary
        (2100, 50),      # inside shard 1
        (1000, 2849)])   # to the end
    def test_striped(self, offset, length):
        """3849 bytes as [2048, 1801]: what lies in shard 1 counts its tiles
        from 0 in the shard and from 2 in the object, the branch with two
        mixes: an edge in the first two cases, the run to the object's end in
        the third. patch() checks both shard digests and the object's."""
        r, (shard, obj) = _one(3849, offset, length, lens=[2048, 1801])
        assert any(e[5] != e[6] for e in r.edges) or \
            any(s[3] != s[4] for s in r.runs)
        assert r.edges
        assert len(shard) == 2 and len(obj) == 1

    def test_odd_source_address(self):
        """Edges alone from a source at an odd address, whatever the offset's
        phase: no alignment is asked of an edge."""
        objs = [(_rand(120, 4096), [4096])]
        for phase in (1, 7):
            with _Rig(objs, [(0, 1016, 16)], src_phase=phase) as r:
                assert r.runs == [] and len(r.edges) == 2
                assert all((r.src + e[0]) % 2 == 1 for e in r.edges[:1])
                r.patch(3)

    def test_both_kernels_on_one_accumulator(self):
        """A run of 4D + D/2 tiles between two edges of one object: the run
        kernel and the edge kernel add into the same two sums. Beside it an
        object patched by a run alone and one by an edge alone."""
        d = gpu.patch_walk_depth()
        per = 4 * d + max(d // 2, 1)
        size = (per + 2) * TILE + 5
        objs = [(_rand(130, size), [size]), (_rand(131, 4096), [4096]),
                (_rand(132, 4096), [4096])]
        patches = [(0, 1000, 24 + per * TILE + 100), (1, 1024, 2048),
                   (2, 5, 7)]
        with _Rig(objs, patches) as r:
            assert [s[2] for s in r.runs] == [per * TILE, 2048]
            assert [e[8] for e in r.edges] == [0, 0, 2]
            r.patch(4)
        # and striped, the run and the tail edge in shard 1
        objs = [(_rand(133, size), [2048, size - 2048])]
        with _Rig(objs, [(0, 1000, size - 1000 - 3)]) as r:
            assert len(r.runs) == 2 and len(r.edges) == 2
            r.patch(5)

    def test_six_hundred_edges(self):
        """More waves than one block holds, more accumulators than the
        256-thread finalize block."""
        objs = [(_rand(1000 + i, 2048), [2048]) for i in range(600)]
        patches = [(i, 1024 * (i % 2) + 3 + i % 1000, 1 + i % 17)
                   for i in range(600)]
        with _Rig(objs, patches) as r:
            assert r.runs == [] and len(r.edges) == 600
            r.patch(6)

    def test_corruption_outside_the_range_is_not_laundered(self):
        """One flipped bit in the pool inside the edge tile but outside
        [lo, hi), and in a second object one in a tile the patch does not
        touch. The patch reads only its tile and writes only [lo, hi): the
        flipped bytes stay (the pool compare) and the new digests are not
        those of what the pool holds, so a scrub still finds both."""
        objs = [(_rand(140, 4096), [4096]), (_rand(141, 4096), [4096])]
        with _Rig(objs, [(0, 1000, 23), (1, 1000, 23)],
                  flips=[(0, 500), (1, 3000)]) as r:
            shard, obj = r.patch(7, check=False)
            held = r.pool_digests()
            clean = r.digests()[1]
            assert held[0] != clean[0] and held[1] != clean[1]
            assert obj[0] != held[0] and obj[1] != held[1]
            assert shard[0] != held[0] and shard[1] != held[1]
            # the untouched tile never entered the sums: the clean digest
            assert obj[1] == clean[1] and shard[1] == clean[1]

    def test_rejects_bad_edges_before_launch(self):
        buf = gpu.malloc(8192)
        try:
            gpu.upload(buf, b"\x11" * 8192)
            with pytest.raises(bb.core.BlackbirdError, match="INVALID_ARGUMENT"):
                # an edge on a tile of the run
                gpu.fused_patch([(buf, buf + 4096, 1024, 0, 0, 0, 0)],
                                [4096], [1], [4096], [1],
                                edges=[(buf + 2048, buf + 4096, 5, 9, 1024,
                                        0, 0, 0, 0)])
            assert gpu.download(buf, 8192) == b"\x11" * 8192
        finally:
            gpu.free(buf)


def _mixed_rig():
    """Runs and edges of every shape in one launch (object: what it is)."""
    objs = [
        (_rand(1, 4096), [4096]),                        # 0 one edge
        (_rand(2, 8192), [8192]),                        # 1 head, run, tail
        (_rand(3, 3849), [2048, 1801]),                  # 2 across shards
        (_rand(4, 5000), [5000]),                        # 3 the last, short tile
        (_rand(5, 5 * TILE + 17), [5 * TILE + 17]),      # 4 a run alone, to the end
        (_rand(6, 2 * TILE + 5), [2 * TILE + 5]),        # 5 nothing names it
        (_rand(7, 4 * TILE), [2 * TILE, 2 * TILE]),      # 6 run in shard 0, edge in 1
    ]
    patches = [(0, 1000, 23), (1, 1000, 3000), (2, 2000, 100), (3, 4090, 910),
               (4, 3 * TILE, 2 * TILE + 17), (6, TILE, TILE), (6, 3 * TILE + 1, 9)]
    return _Rig(objs, patches)


class TestFusedPatchPlanWithEdges:
    def test_four_replays_runs_and_edges_mixed(self):
        with _mixed_rig() as r:
            assert r.runs and r.edges
            start_shard, start_obj = r.digests()
            got = r.replay(4, seed=10)
            for shard, obj in got:
                assert obj[5] == start_obj[5]
                assert shard[6] == start_shard[6]   # object 5's only shard
            assert len({tuple(obj) for _, obj in got}) == 4

    def test_four_replays_edges_alone(self):
        objs = [(_rand(20 + i, 4096), [4096]) for i in range(5)]
        patches = [(i, o, n) for i, (o, n) in enumerate(INSIDE_ONE_TILE)]
        with _Rig(objs, patches) as r:
            assert r.runs == [] and len(r.edges) == 5
            r.replay(4, seed=20)

    def test_step_one_equals_the_one_shot_launch_bit_for_bit(self):
        with _mixed_rig() as r:
            shard_old, obj_old = r.digests()
            start = bytes(r.img)
            one_shot = r.patch(30)
            gpu.upload(r.pool, start)
            planned = gpu.fused_patch_plan(r.segs(), r.shard_lens, r.obj_sizes,
                                           shard_old, obj_old, 1,
                                           edges=r.edge_list())
            assert r.pool_now() == bytes(r.img)
            assert planned == [one_shot]

    def test_empty_plan_is_refused(self):
        with pytest.raises(bb.core.BlackbirdError, match="INVALID_ARGUMENT"):
            gpu.fused_patch_plan([], [4096], [4096], [1], [1], 1, edges=[])
