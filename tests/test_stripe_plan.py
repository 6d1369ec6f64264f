"""Host side of the fused striped copy+digest launch (no GPU): the planner
that turns one copy's shard lengths into segments, the argument check of
gpu.fused_stripe, and the identity that lets one pass over the shards yield
the object's digest."""
import numpy as np
import pytest

import blackbird_amd as bb

MB = 1 << 20
gpu = bb.core.gpu


def _even_shards(size, n):
    """Shard lengths as the allocator cuts them: ceil(size/n), last shorter."""
    shard = (size + n - 1) // n
    lens = []
    left = size
    while left > 0:
        lens.append(min(shard, left))
        left -= lens[-1]
    return lens


class TestPlanner:
    @pytest.mark.parametrize("n", [2, 4, 8])
    def test_power_of_two_stripes(self, n):
        plan = gpu.plan_stripe(1 * MB, _even_shards(1 * MB, n))
        each = MB // n
        assert plan == [(k * each, each, k * each // 1024) for k in range(n)]
        for off, nbytes, first_tile in plan:
            assert off % 1024 == 0 and first_tile * 1024 == off

    def test_three_way_is_not_fusable(self):
        lens = _even_shards(1 * MB, 3)
        assert lens[0] == 349526
        assert gpu.plan_stripe(1 * MB, lens) is None

    def test_odd_size_two_way_is_not_fusable(self):
        size = 2 * MB + 1000
        assert gpu.plan_stripe(size, _even_shards(size, 2)) is None

    def test_final_short_shard_is_accepted(self):
        size = 2 * MB + 777
        plan = gpu.plan_stripe(size, [1 * MB, 1 * MB, 777])
        assert plan == [(0, MB, 0), (MB, MB, 1024), (2 * MB, 777, 2048)]
        # a single shard is its whole object
        assert gpu.plan_stripe(1000, [1000]) == [(0, 1000, 0)]

    def test_lengths_must_add_up(self):
        assert gpu.plan_stripe(4096, [2048, 1024]) is None
        assert gpu.plan_stripe(4096, [2048, 4096]) is None


class TestChecker:
    """Segments are (src, dst, nbytes, first_tile, obj); the check never
    looks at the addresses."""

    def _ok(self, segs, sizes):
        gpu.check_stripe_segs(segs, sizes)

    def _rejected(self, segs, sizes):
        with pytest.raises(Exception, match="INVALID_ARGUMENT"):
            gpu.check_stripe_segs(segs, sizes)

    def test_object_index_in_range(self):
        self._ok([(0, 0, 1024, 0, 1)], [4096, 4096])
        self._rejected([(0, 0, 1024, 0, 2)], [4096, 4096])
        self._rejected([(0, 0, 0, 0, 0)], [])

    def test_segment_inside_object(self):
        self._ok([(0, 0, 2048, 2, 0)], [4096])
        self._rejected([(0, 0, 3072, 2, 0)], [4096])
        self._rejected([(0, 0, 0, 5, 0)], [4096])
        # first_tile * 1024 must not wrap
        self._rejected([(0, 0, 1024, 1 << 54, 0)], [4096])
        self._ok([(0, 0, 2048, 1 << 40, 0)], [(1 << 50) + 2048])

    def test_partial_tile_only_at_object_end(self):
        self._ok([(0, 0, 1024 + 777, 2, 0)], [3072 + 777])
        self._ok([(0, 0, 777, 3, 0)], [3072 + 777])
        self._rejected([(0, 0, 777, 0, 0)], [4096])
        self._rejected([(0, 0, 1025, 1, 0)], [3072 + 777])

    def test_zero_length_and_whole_object(self):
        self._ok([(0, 0, 0, 0, 0), (0, 0, 0, 4, 0), (0, 0, 0, 2, 0)], [4096])
        self._ok([(0, 0, 4096, 0, 0)], [4096])
        self._ok([(0, 0, 1, 0, 0)], [1])
        self._ok([(0, 0, 1025, 0, 0)], [1025])
        self._ok([], [])
        self._ok([], [4096])


    def test_fused_stripe_checks_before_any_device_call(self):
        """The launch entry runs the same check first, so a bad list is
        INVALID_ARGUMENT with or without a GPU; an empty list returns at
        once."""
        with pytest.raises(Exception, match="INVALID_ARGUMENT"):
            gpu.fused_stripe([(4096, 8192, 777, 0, 0)], [4096])
        assert gpu.fused_stripe([], []) == ([], [])


class TestCombinationIdentity:
    @pytest.mark.parametrize("size,lens", [
        (1 * MB, _even_shards(1 * MB, 2)),
        (1 * MB, _even_shards(1 * MB, 8)),
        (2 * MB + 777, [1 * MB, 1 * MB, 777]),
        (3072 + 1, [1024, 2048, 1]),
        (1000, [1000]),
    ])
    def test_shard_partials_sum_to_object_digest(self, size, lens):
        blob = np.random.default_rng(size).integers(
            0, 256, size=size, dtype=np.uint8).tobytes()
        plan = gpu.plan_stripe(size, lens)
        assert plan is not None
        h = 0
        for off, nbytes, first_tile in plan:
            h = (h + gpu.checksum_cpu_tiles(blob[off:off + nbytes],
                                            first_tile)) % (1 << 64)
        assert gpu.checksum_cpu_finalize(h, size) == gpu.checksum_cpu(blob)
