"""Byte-granular patch planning, host only: gpu.plan_patch_bytes against a
brute-force byte map, and gpu.check_patch_edges, one rejection per rule.

A plan is (runs, edges): runs are plan_patch's pieces (shard, shard_off,
obj_off, nbytes); edges are (shard, shard_tile, obj_tile, lo, hi, valid,
src_off). Edge descriptors for the check are (src, tile, lo, hi, valid,
shard_tile, obj_tile, shard, obj)."""
import pytest

import blackbird_amd as bb

gpu = bb.core.gpu
TILE = 1024

SIZES = [1, 1024, 3849, 4096]
LENS = {"whole": lambda size: [size],
        "two": lambda size: [2048, 1801],
        "three": lambda size: [1024, 1024, 1801]}


def _points(size):
    pts = {0, 1, 15, 16, 1023, 1024, 1025, 2047, 2048, 2049, size - 1, size}
    return sorted(p for p in pts if 0 <= p <= size)


def _cases():
    for size in SIZES:
        for name, make in LENS.items():
            lens = make(size)
            if sum(lens) != size:
                continue
            yield pytest.param(size, lens, id="%d-%s" % (size, name))


def _shard_starts(lens):
    out, off = [], 0
    for n in lens:
        out.append(off)
        off += n
    return out


@pytest.mark.parametrize("size,lens", list(_cases()))
def test_plan_against_a_byte_map(size, lens):
    starts = _shard_starts(lens)
    checked = 0
    for offset in _points(size):
        for length in _points(size):
            if offset + length > size:
                continue
            plan = gpu.plan_patch_bytes(size, lens, offset, length)
            assert plan is not None, (offset, length)
            runs, edges = plan
            # every byte of the range once, none outside: (object byte ->
            # byte of the caller's new bytes)
            seen = {}
            for shard, shard_off, obj_off, n in runs:
                assert starts[shard] + shard_off == obj_off
                assert shard_off + n <= lens[shard]
                # whole tiles, or to the object's end
                assert shard_off % TILE == 0 and obj_off % TILE == 0
                assert n > 0
                assert n % TILE == 0 or obj_off + n == size, (offset, length)
                for b in range(n):
                    assert obj_off + b not in seen
                    seen[obj_off + b] = obj_off + b - offset
            assert len(edges) <= 2, (offset, length)
            for shard, st, ot, lo, hi, valid, src_off in edges:
                assert starts[shard] + st * TILE == ot * TILE
                assert valid == min(TILE, lens[shard] - st * TILE)
                assert valid == min(TILE, size - ot * TILE)
                assert 0 <= lo < hi <= valid
                assert (lo, hi) != (0, TILE)
                for p in range(lo, hi):
                    at = ot * TILE + p
                    assert at not in seen
                    seen[at] = src_off + p - lo
            assert seen == {offset + b: b for b in range(length)}, \
                (offset, length)
            # no edge on a tile a run covers
            covered = {(s, t) for s, so, _, n in runs
                       for t in range(so // TILE, (so + n + TILE - 1) // TILE)}
            assert not covered & {(s, st) for s, st, *_ in edges}
            # the whole-tile planner's answer wherever it has one
            aligned = gpu.plan_patch(size, lens, offset, length)
            if aligned is not None:
                assert runs == aligned and edges == [], (offset, length)
            else:
                # refused there for its edges, or an empty range off a tile
                assert edges or length == 0, (offset, length)
            checked += 1
    assert checked >= 3


def test_shapes_of_small_ranges():
    # inside one tile: one edge
    assert gpu.plan_patch_bytes(4096, [4096], 1, 1) == \
        ([], [(0, 0, 0, 1, 2, 1024, 0)])
    assert gpu.plan_patch_bytes(4096, [4096], 2053, 7) == \
        ([], [(0, 2, 2, 5, 12, 1024, 0)])
    # across a boundary, no whole tile: two edges and no run
    assert gpu.plan_patch_bytes(4096, [4096], 1023, 2) == \
        ([], [(0, 0, 0, 1023, 1024, 1024, 0), (0, 1, 1, 0, 1, 1024, 1)])
    # head, interior, tail
    assert gpu.plan_patch_bytes(8192, [8192], 1000, 3000) == \
        ([(0, 1024, 1024, 2048)],
         [(0, 0, 0, 1000, 1024, 1024, 0), (0, 3, 3, 0, 928, 1024, 2072)])
    # from a tile boundary to the object's end, mid-tile: a run, no edge
    assert gpu.plan_patch_bytes(5000, [5000], 4096, 904) == \
        ([(0, 4096, 4096, 904)], [])
    # the last partial tile entered inside: an edge with valid < 1024
    assert gpu.plan_patch_bytes(5000, [5000], 4106, 100) == \
        ([], [(0, 4, 4, 10, 110, 904, 0)])
    # striped: the edge of shard 1 counts its tile in shard and in object
    assert gpu.plan_patch_bytes(3849, [2048, 1801], 2000, 100) == \
        ([], [(0, 1, 1, 976, 1024, 1024, 0), (1, 0, 2, 0, 52, 1024, 48)])
    # an empty range
    assert gpu.plan_patch_bytes(4096, [4096], 7, 0) == ([], [])


def test_refusals():
    for offset, length in [(0, 3850), (3849, 1), (3850, 0), (1 << 63, 1 << 63)]:
        assert gpu.plan_patch_bytes(3849, [3849], offset, length) is None
    # shards off tile boundaries, lengths that do not add up
    assert gpu.plan_patch_bytes(3849, [2000, 1849], 0, 1) is None
    assert gpu.plan_patch_bytes(3849, [2048, 1800], 0, 1) is None


# ------------------------------------------------------- check_patch_edges

SRC, POOL = 1 << 20, 2 << 20
# object 0: 3849 bytes as [2048, 1801] at POOL and POOL + 4096;
# object 1: 8192 bytes, one shard at POOL + 8192
SHARD_LENS = [2048, 1801, 8192]
OBJ_SIZES = [3849, 8192]
SHARD_AT = [POOL, POOL + 4096, POOL + 8192]


def _edge(shard, shard_tile, obj_tile, lo, hi, valid, obj, src=SRC + 3):
    return (src, SHARD_AT[shard] + shard_tile * TILE, lo, hi, valid,
            shard_tile, obj_tile, shard, obj)


RUN = (SRC + 4096, SHARD_AT[2] + 2048, 2048, 2, 2, 2, 1)  # tiles 2, 3 of shard 2
GOOD = [_edge(0, 1, 1, 976, 1024, 1024, 0),           # head, shard 0
        _edge(1, 0, 2, 0, 52, 1024, 0, SRC + 51),     # tail, shard 1, odd src
        _edge(1, 1, 3, 700, 777, 777, 0, SRC + 200),  # the object's last tile
        _edge(2, 1, 1, 1, 1024, 1024, 1, SRC + 2048),  # next to the run
        _edge(2, 4, 4, 0, 1, 1024, 1, SRC + 8000)]


def _check(edges, segs=(RUN,)):
    gpu.check_patch_edges(edges, list(segs), SHARD_LENS, OBJ_SIZES)


def test_a_legal_mixed_list_passes():
    _check(GOOD)
    _check([])
    _check(GOOD, segs=())
    # and through the launch's own check, old digests included
    gpu.check_patch_segs([RUN], SHARD_LENS, [1, 2, 3], OBJ_SIZES, [4, 5],
                         edges=GOOD)


@pytest.mark.parametrize("edge,what", [
    (_edge(0, 0, 0, 0, 1, 1024, 0)[:7] + (3, 0), "shard index"),
    (_edge(0, 0, 0, 0, 1, 1024, 0)[:8] + (2,), "object index"),
    (_edge(0, 0, 0, 5, 5, 1024, 0), "lo < hi"),
    (_edge(0, 0, 0, 6, 5, 1024, 0), "lo < hi"),
    (_edge(1, 1, 3, 700, 778, 777, 0), "hi <= valid"),
    (_edge(1, 1, 3, 700, 777, 1024, 0), "valid"),       # the tile has 777
    (_edge(0, 1, 1, 0, 5, 777, 0), "valid"),            # the tile has 1024
    (_edge(0, 2, 2, 0, 1, 1024, 0), "past its shard"),
    (_edge(1, 2, 4, 0, 1, 1024, 0), "past its shard"),
    (_edge(1, 0, 3, 0, 5, 1024, 0), "valid"),  # 1024 in the shard, 777 in the object
    (_edge(1, 0, 4, 0, 5, 1024, 0), "past its object"),
    ((SRC, POOL, 0, 5, 1024, 1 << 60, 1 << 60, 2, 1), "past its shard"),
    (_edge(0, 0, 0, 10, 20, 1024, 0, src=POOL + 1023), "overlaps"),
    (_edge(0, 0, 0, 10, 20, 1024, 0, src=POOL - 5), "overlaps"),
    (_edge(2, 2, 2, 0, 5, 1024, 1), "tile of a run"),
    (_edge(2, 3, 3, 1000, 1024, 1024, 1), "tile of a run"),
    (_edge(2, 1, 1, 0, 1, 1024, 1, SRC + 9000), "another edge"),
])
def test_one_rejection_per_rule(edge, what):
    with pytest.raises(bb.core.BlackbirdError, match="INVALID_ARGUMENT") as e:
        _check(GOOD + [edge])
    assert "patch edge" in str(e.value), what
    # the launch refuses it before any HIP call, with or without a GPU
    with pytest.raises(bb.core.BlackbirdError, match="INVALID_ARGUMENT"):
        gpu.fused_patch([RUN], SHARD_LENS, [1, 2, 3], OBJ_SIZES, [4, 5],
                        edges=GOOD + [edge])


def test_source_next_to_its_tile_is_no_overlap():
    # [src, src + hi - lo) ends where the tile begins; begins where valid ends
    _check([_edge(0, 0, 0, 10, 20, 1024, 0, src=POOL - 10)], segs=())
    _check([_edge(1, 1, 3, 0, 5, 777, 0, src=SHARD_AT[1] + 1024 + 777)],
           segs=())


def test_existing_entry_points_take_no_edges():
    """The calls of before: same arguments, same answers."""
    gpu.check_patch_segs([RUN], SHARD_LENS, [1, 2, 3], OBJ_SIZES, [4, 5])
    assert gpu.plan_patch(4096, [4096], 1, 1) is None
