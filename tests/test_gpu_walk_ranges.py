"""The batched tile walk (digest_device.hip.h) where the ranges of its waves
meet the descriptors in ways test_gpu_walk_pipeline.py does not reach: that
file's small batches stay far below the range rule's cap, and its large ones
hold a few long objects. Here the batches are sized from the rule as built
(gpu.digest_grid_waves gives the ranges it cuts; the trailing ones may be
empty):

  odd_last_range  below the cap, two tiles per range, the last range one tile
  one_object      below the cap: one object across thousands of ranges, one
                  tile off the range grid
  empty_ranges    just past the cap: three tiles per range, and a third of
                  the ranges empty behind the last tile
  small_objects   the same total in objects of 1-3 tiles with 1-byte and
                  1023-byte tails and zero-byte objects between them: every
                  range starts in another descriptor, some in a tail tile,
                  and the last ranges start in the last descriptor

Every case runs through checksum_device_batch, fused_put, fused_put_plan
(three replays), fused_stripe and fused_patch: digests bit-exact against
gpu.checksum_cpu, destination bytes exact including the pre-filled gaps. The
layout is that of test_gpu_walk_pipeline.py: objects at 16-byte-aligned
offsets of one allocation with 16 bytes of gap behind each, 0x5A in the
source gaps, the destination pre-filled with 0xA5, the last object ending
where both allocations end. fused_stripe takes objects of more than 64 tiles as two
segments, the second with first_tile != 0.

fused_patch patches every non-empty object whole, over old random bytes of
the same sizes in the destination (a second seed; the old digests are
checksum_cpu of them). Its runs are the stripe entry's segments, each a shard
of its own: the second run of a long object has shard_tile 0 and obj_tile at
the cut, so both mixes run. A zero-byte object is registered nowhere (a
recorded digest of 0 is refused); its zero-length run names the shard and
the object of a neighbour.
"""
import numpy as np
import pytest

import blackbird_amd as bb

pytestmark = pytest.mark.gpu

TILE = 1024
PAD = 0xA5
gpu = bb.core.gpu

ENTRIES = ["checksum_device_batch", "fused_put", "fused_put_plan",
           "fused_stripe", "fused_patch"]
CASES = ["odd_last_range", "one_object", "empty_ranges", "small_objects"]

# sizes of 1-3 tiles: whole tiles, 1-byte and 1023-byte tails, and nothing;
# 13 entries, so the pattern does not line up with the ranges
SMALL = [TILE, 1, 2 * TILE + 1023, 0, 3 * TILE, TILE + 1, 1023, 2 * TILE,
         2 * TILE + 1, 0, TILE + 1023, 3 * TILE - 1023, 2 * TILE + 1]


def _tiles(size):
    return (size + TILE - 1) // TILE


def _ranges(total_tiles):
    """(tiles per range, ranges that hold a tile, ranges the rule cuts)."""
    cut = gpu.digest_grid_waves(total_tiles)
    per = (total_tiles + cut - 1) // cut
    return per, (total_tiles + per - 1) // per, cut


class _Batch:
    """Objects of the given sizes, filled from one seeded stream."""

    def __init__(self, sizes, seed):
        self.sizes = list(sizes)
        self.offs, off = [], 0
        for s in self.sizes:
            self.offs.append(off)
            off += (s + 15) // 16 * 16 + 16
        self.span = max(self.offs[-1] + self.sizes[-1], 16)
        data = np.random.default_rng(seed).integers(
            0, 256, sum(self.sizes), dtype=np.uint8)
        src = np.full(self.span, 0x5A, dtype=np.uint8)
        dst = np.full(self.span, PAD, dtype=np.uint8)
        self.want, self.segs, at = [], [], 0
        for i, (o, s) in enumerate(zip(self.offs, self.sizes)):
            blob = data[at:at + s]
            at += s
            src[o:o + s] = blob
            dst[o:o + s] = blob
            self.want.append(gpu.checksum_cpu(blob))
            # (obj, offset in the allocation, nbytes, first_tile, digest)
            if _tiles(s) <= 64:
                self.segs.append((i, o, s, 0, self.want[-1]))
            else:
                cut = _tiles(s) // 2 + 3
                self.segs.append((i, o, cut * TILE, 0,
                                  gpu.checksum_cpu(blob[:cut * TILE])))
                self.segs.append((i, o + cut * TILE, s - cut * TILE, cut,
                                  gpu.checksum_cpu(blob[cut * TILE:])))
        self.src_image = src.tobytes()
        self.dst_image = dst.tobytes()
        self.seed = seed
        self._patch = None

    def patch(self):
        """What fused_patch needs on top, made once: (the destination's old
        image, runs as (segment index, shard_tile, obj_tile, shard, obj),
        shard lengths, old shard digests, object sizes, old object digests,
        expected shard digests, expected object digests)."""
        if self._patch is None:
            old = np.random.default_rng(self.seed + 100).integers(
                0, 256, sum(self.sizes), dtype=np.uint8)
            img = np.full(self.span, PAD, dtype=np.uint8)
            start = np.concatenate(([0], np.cumsum(self.sizes)))
            obj_of, sizes, obj_old, obj_want = {}, [], [], []
            for i, (o, s) in enumerate(zip(self.offs, self.sizes)):
                if s:
                    blob = old[start[i]:start[i] + s]
                    img[o:o + s] = blob
                    obj_of[i] = len(sizes)
                    sizes.append(s)
                    obj_old.append(gpu.checksum_cpu(blob))
                    obj_want.append(self.want[i])
            runs, lens, shard_old, shard_want = [], [], [], []
            for k, (i, o, n, first, d) in enumerate(self.segs):
                if n:
                    at = start[i] + first * TILE
                    runs.append((k, 0, first, len(lens), obj_of[i]))
                    lens.append(n)
                    shard_old.append(gpu.checksum_cpu(old[at:at + n]))
                    shard_want.append(d)
                else:
                    runs.append(None)
            # a zero-length run: the nearest run's shard and object
            live = [r for r in runs if r]
            for k, r in enumerate(runs):
                if r is None:
                    near = next((q for q in runs[k::-1] if q), live[0])
                    runs[k] = (k, 0, 0, near[3], near[4])
            self._patch = (img.tobytes(), runs, lens, shard_old, sizes,
                           obj_old, shard_want, obj_want)
        return self._patch

    def tiles(self):
        return sum(_tiles(s) for s in self.sizes)


def _split(total_tiles, parts, tail):
    """Sizes of `parts` objects that hold total_tiles tiles between them;
    none ends on a tile, the last has `tail` bytes in its last tile."""
    tiles = [total_tiles // parts + (3, 1, 4, 2)[i % 4] for i in range(parts - 1)]
    tiles.append(total_tiles - sum(tiles))
    tails = [(1023, 17, 1, 512)[i % 4] for i in range(parts - 1)] + [tail]
    return [(t - 1) * TILE + b for t, b in zip(tiles, tails)]


def _small_sizes(total_tiles):
    """Objects of 0-3 tiles that hold total_tiles tiles, the last of them 7
    tiles with a 1023-byte tail."""
    sizes, left, i = [], total_tiles - 7, 0
    while left > 0:
        s = SMALL[i % len(SMALL)]
        i += 1
        if _tiles(s) > left:
            s = left * TILE
        sizes.append(s)
        left -= _tiles(s)
    return sizes + [6 * TILE + 1023]


_batches = {}


def _batch(name):
    if name not in _batches:
        # the range count saturates at the rule's cap
        cap = gpu.digest_grid_waves(1 << 40)
        if name == "odd_last_range":
            sizes = _split(cap - 1, 3, 1023)
        elif name == "one_object":
            sizes = [TILE, (cap - 1) * TILE + 1]
        elif name == "empty_ranges":
            sizes = _split(2 * cap + 1, 5, 1)
        elif name == "small_objects":
            sizes = _small_sizes(2 * cap + 5)
        _batches[name] = _Batch(sizes, 7000 + CASES.index(name))
    return _batches[name]


def _check(got, want, what):
    bad = [i for i, (g_, w) in enumerate(zip(got, want)) if g_ != w]
    assert len(got) == len(want) and not bad, (what, bad[:8])


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", CASES)
def test_ranges(name, entry):
    b = _batch(name)
    src, dst = gpu.malloc(b.span), gpu.malloc(b.span)
    try:
        gpu.upload(src, b.src_image)
        gpu.upload(dst, b.patch()[0] if entry == "fused_patch"
                   else bytes([PAD]) * b.span)
        descs = [(src + o, dst + o, s) for o, s in zip(b.offs, b.sizes)]
        if entry == "checksum_device_batch":
            _check(gpu.checksum_device_batch([(s, n) for s, _, n in descs]),
                   b.want, entry)
        elif entry == "fused_put":
            _check(gpu.fused_put(descs), b.want, entry)
        elif entry == "fused_put_plan":
            steps = gpu.fused_put_plan(descs, 3)
            assert len(steps) == 3
            assert steps[1] == steps[0] and steps[2] == steps[0]
            _check(steps[0], b.want, entry)
        elif entry == "fused_patch":
            _, runs, lens, shard_old, sizes, obj_old, shard_want, obj_want = \
                b.patch()
            shard, obj = gpu.fused_patch(
                [(src + b.segs[k][1], dst + b.segs[k][1], b.segs[k][2],
                  st, ot, sh, ob) for k, st, ot, sh, ob in runs],
                lens, shard_old, sizes, obj_old)
            _check(shard, shard_want, "shards")
            _check(obj, obj_want, "objects")
        else:
            seg, obj = gpu.fused_stripe(
                [(src + o, dst + o, n, first, i)
                 for i, o, n, first, _ in b.segs], b.sizes)
            _check(seg, [d for *_, d in b.segs], "segments")
            _check(obj, b.want, "objects")
        if entry != "checksum_device_batch":
            assert gpu.download(dst, b.span) == b.dst_image, entry
    finally:
        gpu.free(src)
        gpu.free(dst)


def test_batches_are_what_they_claim():
    """The batches against the range rule as built."""
    cap = gpu.digest_grid_waves(1 << 40)

    def shape(name):
        b = _batch(name)
        return (b,) + _ranges(b.tiles())

    b, per, live, cut = shape("odd_last_range")
    assert per == 2 and cut < cap and b.tiles() % 2 == 1 and live > 1000
    b, per, live, cut = shape("one_object")
    assert per == 2 and cut < cap and len(b.sizes) == 2 and live > 1000
    assert _tiles(b.sizes[0]) % per
    assert any(first for *_, first, _ in b.segs)
    for name in ("empty_ranges", "small_objects"):
        b, per, live, cut = shape(name)
        assert cut == cap and per == 3 and live < cut - cap // 4, name
    # small objects: more than one per range on average, zero-byte ones among
    # them, and the last two ranges start in the last one
    assert len(b.sizes) > live and b.sizes.count(0) > 100
    assert _tiles(b.sizes[-1]) >= 2 * per + 1
