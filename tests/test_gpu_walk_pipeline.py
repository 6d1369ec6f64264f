"""The pipelined tile walk of the batched digest kernels (digest_device.hip.h)
at the places where a software pipeline goes wrong: runs of full tiles
shorter than, equal to and just longer than the pipeline, a descriptor switch
directly behind prefetched tiles, waves that go round the steady loop more
than once and leave it mid-pipeline, and objects that end where their
allocation ends.

Every case runs through checksum_device_batch, fused_put, fused_put_plan
(three replays) and fused_stripe: digests bit-exact against the CPU
reference, destination bytes exact including the pre-filled gaps between
objects. fused_stripe takes small objects as one segment each and cuts long
ones into two segments, so the second runs the pipelined step with
first_tile != 0 (two mixes per tile).

With depth D (gpu.digest_walk_depth) a run of full tiles of one object
inside a wave's range is walked one by one below 2*D tiles, through
prologue, first group and drain from 2*D, and goes round the steady loop
floor(n / D) - 2 times from 3*D on. The grid rule gives a wave more than two
tiles only once its block cap binds. The small batches therefore check the
short-run path and the descriptor switches. The large ones are sized from
the grid rule and the depth as built: every wave owns at least 4*D tiles plus
a remainder that D does not divide, so it takes the loop's back edge at
least twice, drains, and ends on the one-by-one path.
"""
import numpy as np
import pytest

import blackbird_amd as bb

pytestmark = pytest.mark.gpu

TILE = 1024
PAD = 0xA5
gpu = bb.core.gpu

ENTRIES = ["checksum_device_batch", "fused_put", "fused_put_plan",
           "fused_stripe"]

# every full-tile count 0..9 with tails of 0, 1 and 1023 bytes
EDGE_SIZES = [f * TILE + tail for f in range(10) for tail in (0, 1, 1023)]
# where waves own long ranges, also objects around 3 and 4 times the depth
# tried deepest (4): one and two rounds of the loop inside one object
LOOP_EDGE_SIZES = [f * TILE + 1 for f in (11, 12, 13, 16, 17)]

_blobs = {}
_part_digests = {}


def _blob(size, seed):
    """Seeded random bytes and their CPU digest, made once per (size, seed)."""
    key = (size, seed)
    if key not in _blobs:
        data = np.random.default_rng(seed).bytes(size)
        _blobs[key] = (data, gpu.checksum_cpu(data))
    return _blobs[key]


def _tiles(size):
    return (size + TILE - 1) // TILE


def _tiles_per_wave():
    """Smallest per-wave tile count that takes the steady loop's back edge
    twice and leaves a remainder behind the last full group."""
    depth = gpu.digest_walk_depth()
    per = 4 * depth + max(depth // 2, 1)
    assert per // depth - 2 >= 2
    assert depth == 1 or per % depth
    return per


class _Case:
    """Objects laid out as in the fused-put tests: each at a 16-byte-aligned
    offset of one allocation, 16 bytes of gap after it. Source gaps hold
    0x5A, the destination is pre-filled with 0xA5, so a store past an
    object's end shows in `dst_image`. The last object has no gap behind it:
    it ends exactly where both allocations end."""

    def __init__(self, objs):
        self.objs = list(objs)
        self.sizes = [s for s, _ in objs]
        self.offs, off = [], 0
        for s in self.sizes:
            self.offs.append(off)
            off += (s + 15) // 16 * 16 + 16
        self.span = max(self.offs[-1] + self.sizes[-1], 16)
        src = bytearray(b"\x5a" * self.span)
        dst = bytearray(bytes([PAD]) * self.span)
        self.want = []
        for o, (s, seed) in zip(self.offs, objs):
            data, digest = _blob(s, seed)
            src[o:o + s] = data
            dst[o:o + s] = data
            self.want.append(digest)
        self.src_image = bytes(src)
        self.dst_image = bytes(dst)

    def tiles(self):
        return sum(_tiles(s) for s in self.sizes)

    def segments(self):
        """[(obj, offset in the allocation, nbytes, first_tile, digest)]:
        an object of more than 64 tiles is cut in two a little past its
        middle, the others are one segment."""
        out = []
        for i, (o, (s, seed)) in enumerate(zip(self.offs, self.objs)):
            data, digest = _blob(s, seed)
            if _tiles(s) <= 64:
                out.append((i, o, s, 0, digest))
                continue
            cut = _tiles(s) // 2 + 3
            key = (s, seed, cut)
            if key not in _part_digests:
                _part_digests[key] = (gpu.checksum_cpu(data[:cut * TILE]),
                                      gpu.checksum_cpu(data[cut * TILE:]))
            head, tail = _part_digests[key]
            out.append((i, o, cut * TILE, 0, head))
            out.append((i, o + cut * TILE, s - cut * TILE, cut, tail))
        return out


def _long_sizes():
    """Three object sizes, none a tile multiple, that give every wave of the
    grid as built exactly _tiles_per_wave() tiles, with both inner
    boundaries inside a wave's range."""
    # the wave count saturates at the grid rule's cap
    waves = gpu.digest_grid_waves(1 << 40)
    per = _tiles_per_wave()
    total = waves * per
    assert waves == gpu.digest_grid_waves(total)
    tiles = [total // 3 + 4, total // 3 + 3]
    tiles.append(total - sum(tiles))
    sizes = [(t - 1) * TILE + tail for t, tail in zip(tiles, (1023, 17, 1))]
    assert sum(_tiles(s) for s in sizes) == total
    b1 = tiles[0]
    b2 = b1 + tiles[1]
    assert b1 % per and b2 % per, "boundary on a range edge"
    return sizes


_cases = {}


def _case(name):
    if name not in _cases:
        if name == "pipeline_edges":
            objs = [(s, 100 + i) for i, s in enumerate(EDGE_SIZES)]
        elif name == "alloc_end_tile_multiple":
            # the last object: 5 full tiles up to the allocation's last byte
            objs = [(3 * TILE + 5, 201), (5 * TILE, 202)]
        elif name == "alloc_end_one_byte_tail":
            objs = [(3 * TILE + 5, 201), (5 * TILE + 1, 203)]
        elif name == "long_ranges":
            # ends with a 1-byte tail at the allocation's end
            a, b, c = _long_sizes()
            objs = [(a, 301), (b, 302), (c, 303)]
        elif name == "long_ranges_with_edges":
            # the edge objects between long ones, where waves own long
            # ranges and do take the pipelined path for runs of 2 * depth
            # and more; the last object ends on a tile and on the allocation
            a, b, c = _long_sizes()
            objs = ([(a, 301)] +
                    [(s, 100 + i) for i, s in enumerate(EDGE_SIZES)] +
                    [(b, 302)] +
                    [(s, 400 + i) for i, s in enumerate(LOOP_EDGE_SIZES)] +
                    [(c - 1, 304)])
        _cases[name] = _Case(objs)
    return _cases[name]


CASES = ["pipeline_edges", "alloc_end_tile_multiple",
         "alloc_end_one_byte_tail", "long_ranges", "long_ranges_with_edges"]


def _check(got, want, what):
    bad = [i for i, (g_, w) in enumerate(zip(got, want)) if g_ != w]
    assert len(got) == len(want) and not bad, (what, bad[:8])


def _run(case, entry):
    src, dst = gpu.malloc(case.span), gpu.malloc(case.span)
    try:
        gpu.upload(src, case.src_image)
        gpu.upload(dst, bytes([PAD]) * case.span)
        descs = [(src + o, dst + o, s) for o, s in zip(case.offs, case.sizes)]
        if entry == "checksum_device_batch":
            _check(gpu.checksum_device_batch([(s, n) for s, _, n in descs]),
                   case.want, entry)
        elif entry == "fused_put":
            _check(gpu.fused_put(descs), case.want, entry)
        elif entry == "fused_put_plan":
            steps = gpu.fused_put_plan(descs, 3)
            assert len(steps) == 3
            assert steps[1] == steps[0] and steps[2] == steps[0]
            _check(steps[0], case.want, entry)
        else:
            segs = case.segments()
            seg, obj = gpu.fused_stripe(
                [(src + o, dst + o, n, first, i) for i, o, n, first, _ in segs],
                case.sizes)
            _check(seg, [d for *_, d in segs], "segments")
            _check(obj, case.want, "objects")
        if entry != "checksum_device_batch":
            assert gpu.download(dst, case.span) == case.dst_image, entry
    finally:
        gpu.free(src)
        gpu.free(dst)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", CASES)
def test_walk(name, entry):
    _run(_case(name), entry)


def test_long_cases_reach_every_wave():
    """In the large batches a wave's range takes the steady loop's back edge
    at least twice and ends behind a full group; they are as large as that
    needs and no larger than a few hundred tiles more; the striped form of
    them has segments that do not start at their object's tile 0."""
    waves = gpu.digest_grid_waves(1 << 40)
    depth = gpu.digest_walk_depth()
    want = _tiles_per_wave()
    for name in ("long_ranges", "long_ranges_with_edges"):
        case = _case(name)
        tiles = case.tiles()
        per = (tiles + gpu.digest_grid_waves(tiles) - 1) // \
            gpu.digest_grid_waves(tiles)
        assert waves * want <= tiles < waves * want + 512, (name, tiles)
        assert per // depth - 2 >= 2, (name, per)
        assert depth == 1 or per % depth, (name, per)
        assert any(first for *_, first, _ in case.segments()), name
