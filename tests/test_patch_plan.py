"""Host side of the in-place range patch (no GPU): the inverse of the digest's
finalize, the identity that moves a recorded digest by the patched tiles'
terms alone, the planners that cut a byte range into per-shard pieces, and
the argument check of gpu.fused_patch."""
import numpy as np
import pytest

import blackbird_amd as bb

M64 = (1 << 64) - 1
gpu = bb.core.gpu

# (size, offset, length): a middle tile, the tail alone, the middle through
# to the end, a 1-byte object, a whole object, a last short tile
SHAPES = [(4096, 1024, 1024), (3849, 3072, 777), (3849, 1024, 2825),
          (1, 0, 1), (5000, 0, 5000), (5000, 4096, 904)]


def _rand(seed, n):
    return np.random.default_rng(seed).integers(
        0, 256, size=n, dtype=np.uint8).tobytes()


class TestUnfinalize:
    @pytest.mark.parametrize("h", [0, 1, 0xB1ACB19D, 1 << 63, M64,
                                   0x0123456789ABCDEF])
    @pytest.mark.parametrize("n", [0, 1, 1024, 3849, (1 << 50) + 7])
    def test_round_trip(self, h, n):
        d = gpu.checksum_cpu_finalize(h, n)
        assert gpu.checksum_cpu_unfinalize(d, n) == h
        # and the other way round: finalize is onto
        assert gpu.checksum_cpu_finalize(gpu.checksum_cpu_unfinalize(h, n), n) == h

    def test_recovers_the_tile_sum_of_a_digest(self):
        blob = _rand(1, 3849)
        assert gpu.checksum_cpu_unfinalize(gpu.checksum_cpu(blob), len(blob)) == \
            gpu.checksum_cpu_tiles(blob, 0)


class TestPatchIdentity:
    @pytest.mark.parametrize("size,offset,length", SHAPES)
    def test_patched_digest_from_the_patched_tiles_alone(self, size, offset, length):
        old = _rand(size, size)
        new = _rand(size + 1, length)
        patched = old[:offset] + new + old[offset + length:]
        assert len(patched) == size and patched != old
        first = offset // 1024
        h = gpu.checksum_cpu_unfinalize(gpu.checksum_cpu(old), size)
        h = (h + gpu.checksum_cpu_tiles(new, first)
             - gpu.checksum_cpu_tiles(old[offset:offset + length], first)) & M64
        assert gpu.checksum_cpu_finalize(h, size) == gpu.checksum_cpu(patched)

    def test_corruption_outside_the_range_stays_visible(self):
        """The patch never re-hashes what it did not touch: with a byte
        flipped outside the range, the patched digest is not the digest of
        the patched corrupt bytes."""
        size, offset, length = 4096, 1024, 1024
        old, new = _rand(7, size), _rand(8, length)
        corrupt = bytearray(old)
        corrupt[3000] ^= 0x10
        h = gpu.checksum_cpu_unfinalize(gpu.checksum_cpu(old), size)
        h = (h + gpu.checksum_cpu_tiles(new, 1)
             - gpu.checksum_cpu_tiles(old[offset:offset + length], 1)) & M64
        got = gpu.checksum_cpu_finalize(h, size)
        corrupt[offset:offset + length] = new
        assert got != gpu.checksum_cpu(bytes(corrupt))


class TestPlanners:
    """Pieces are (shard, shard_off, obj_off, nbytes)."""

    def test_one_shard(self):
        assert gpu.plan_patch(3849, [3849], 1024, 1024) == [(0, 1024, 1024, 1024)]
        assert gpu.plan_patch(3849, [3849], 3072, 777) == [(0, 3072, 3072, 777)]
        assert gpu.plan_patch(3849, [3849], 0, 3849) == [(0, 0, 0, 3849)]
        assert gpu.plan_patch(1, [1], 0, 1) == [(0, 0, 0, 1)]
        assert gpu.plan_patch(4096, [4096], 2048, 0) == []
        assert gpu.range_pieces(3849, [3849], 1, 1023) == [(0, 1, 1, 1023)]

    def test_two_shards(self):
        lens = [2048, 1801]
        # inside one shard
        assert gpu.plan_patch(3849, lens, 1024, 1024) == [(0, 1024, 1024, 1024)]
        assert gpu.plan_patch(3849, lens, 2048, 1024) == [(1, 0, 2048, 1024)]
        # across the boundary
        assert gpu.plan_patch(3849, lens, 1024, 2048) == \
            [(0, 1024, 1024, 1024), (1, 0, 2048, 1024)]
        # to the object's end, mid-tile
        assert gpu.plan_patch(3849, lens, 1024, 2825) == \
            [(0, 1024, 1024, 1024), (1, 0, 2048, 1801)]
        assert gpu.plan_patch(3849, lens, 3072, 777) == [(1, 1024, 3072, 777)]
        # a ranged get takes any bytes
        assert gpu.range_pieces(3849, lens, 2047, 2) == \
            [(0, 2047, 2047, 1), (1, 0, 2048, 1)]
        assert gpu.range_pieces(3849, lens, 3848, 1) == [(1, 1800, 3848, 1)]

    def test_three_shards(self):
        lens = [2048, 2048, 1000]
        size = sum(lens)
        assert gpu.plan_patch(size, lens, 2048, 1024) == [(1, 0, 2048, 1024)]
        assert gpu.plan_patch(size, lens, 1024, 3072 + 1000) == \
            [(0, 1024, 1024, 1024), (1, 0, 2048, 2048), (2, 0, 4096, 1000)]
        assert gpu.plan_patch(size, lens, 3072, 1024) == [(1, 1024, 3072, 1024)]
        assert gpu.range_pieces(size, lens, 1, size - 1) == \
            [(0, 1, 1, 2047), (1, 0, 2048, 2048), (2, 0, 4096, 1000)]
        # every piece of a patch plan starts on a tile of shard and object
        for shard, shard_off, obj_off, n in gpu.plan_patch(size, lens, 0, size):
            assert shard_off % 1024 == 0 and obj_off % 1024 == 0

    def test_refusals(self):
        lens = [2048, 1801]
        assert gpu.plan_patch(3849, lens, 1, 1024) is None       # offset
        assert gpu.plan_patch(3849, lens, 1023, 1) is None
        assert gpu.plan_patch(3849, lens, 1024, 777) is None     # interior length
        assert gpu.plan_patch(3849, lens, 0, 3848) is None
        assert gpu.plan_patch(3849, lens, 3072, 778) is None     # past the end
        assert gpu.plan_patch(3849, lens, 4096, 0) is None
        # a copy plan_stripe refuses: shard 1 starts inside a tile
        assert gpu.plan_stripe(3849, [2000, 1849]) is None
        assert gpu.plan_patch(3849, [2000, 1849], 0, 1024) is None
        assert gpu.plan_patch(4096, [2048, 1024], 0, 1024) is None
        # the ranged get only needs the lengths to add up and the range inside
        assert gpu.range_pieces(3849, [2000, 1849], 1999, 2) == \
            [(0, 1999, 1999, 1), (1, 0, 2000, 1)]
        assert gpu.range_pieces(3849, lens, 3849, 0) == []
        assert gpu.range_pieces(3849, lens, 3849, 1) is None
        assert gpu.range_pieces(3849, lens, 0, 3850) is None
        assert gpu.range_pieces(3849, lens, 1 << 63, 1 << 63) is None
        assert gpu.range_pieces(4096, [2048, 1024], 0, 1) is None


A, B = 1 << 20, 2 << 20  # two 16-byte-aligned addresses far apart


class TestChecker:
    """Runs are (src, dst, nbytes, shard_tile, obj_tile, shard, obj); the
    object is 3 KiB + 777 B over shards of 2048 and 1801 bytes."""
    LENS, OLD_S = [2048, 1801], [11, 12]
    SIZES, OLD_O = [3849], [13]

    def _check(self, segs, lens=None, old_s=None, sizes=None, old_o=None):
        gpu.check_patch_segs(segs, self.LENS if lens is None else lens,
                             self.OLD_S if old_s is None else old_s,
                             self.SIZES if sizes is None else sizes,
                             self.OLD_O if old_o is None else old_o)

    def _rejected(self, segs, **kw):
        with pytest.raises(Exception, match="INVALID_ARGUMENT"):
            self._check(segs, **kw)

    def test_accepts_legal_runs(self):
        self._check([(A, B, 1024, 1, 1, 0, 0)])
        self._check([(A, B, 1801, 0, 2, 1, 0)])             # to the end, mid-tile
        self._check([(A, B, 777, 1, 3, 1, 0)])              # the tail alone
        self._check([(A, B, 1024, 0, 0, 0, 0), (A + 1024, B + 1024, 1024, 1, 1, 0, 0),
                     (A + 2048, B + 2048, 1024, 0, 2, 1, 0)])
        self._check([])

    def test_shard_index_out_of_range(self):
        self._rejected([(A, B, 1024, 0, 0, 2, 0)])

    def test_object_index_out_of_range(self):
        self._rejected([(A, B, 1024, 0, 0, 0, 1)])

    def test_run_outside_its_shard(self):
        self._rejected([(A, B, 2048, 1, 1, 0, 0)])
        self._rejected([(A, B, 0, 3, 0, 0, 0)])
        self._rejected([(A, B, 1024, 1 << 54, 0, 0, 0)])    # tile * 1024 wraps

    def test_run_outside_its_object(self):
        self._rejected([(A, B, 1024, 0, 3, 1, 0)])
        self._rejected([(A, B, 0, 0, 4, 0, 0)])
        self._rejected([(A, B, 1024, 0, 1 << 54, 0, 0)])

    def test_partial_tile_only_at_the_end_of_object_and_shard(self):
        self._rejected([(A, B, 777, 0, 0, 0, 0)])
        self._rejected([(A, B, 1025, 0, 2, 1, 0)])
        # ends at the object's end but not at its shard's
        self._rejected([(A, B, 777, 0, 3, 1, 0)])
        # ends at its shard's end but not at the object's
        self._rejected([(A, B, 1801, 0, 1, 1, 0)])

    def test_alignment(self):
        self._rejected([(A + 8, B, 1024, 0, 0, 0, 0)])
        self._rejected([(A, B + 4, 1024, 0, 0, 0, 0)])

    def test_source_overlaps_destination(self):
        self._rejected([(A, A, 1024, 0, 0, 0, 0)])
        self._rejected([(A, A + 1008, 1024, 0, 0, 0, 0)])
        self._rejected([(A + 16, A, 1024, 0, 0, 0, 0)])
        self._check([(A, A + 1024, 1024, 0, 0, 0, 0)])      # back to back

    def test_two_runs_on_one_shard_tile(self):
        self._rejected([(A, B, 1024, 1, 1, 0, 0), (A + 4096, B, 1024, 1, 1, 0, 0)])
        self._rejected([(A, B, 2048, 0, 0, 0, 0),
                        (A + 4096, B + 1024, 1024, 1, 1, 0, 0)])
        # the same tile index of another shard is another tile
        self._check([(A, B, 1024, 0, 0, 0, 0), (A + 4096, B + 2048, 1024, 0, 2, 1, 0)])

    def test_unrecorded_old_digest(self):
        run = [(A, B, 1024, 0, 0, 0, 0)]
        self._rejected(run, old_s=[0, 12])
        self._rejected(run, old_s=[11, 0])   # even of a shard no run names
        self._rejected(run, old_o=[0])
        self._rejected([], old_o=[0])

    def test_zero_length_runs(self):
        # any address, any tile up to the end, as often as wanted
        self._check([(0, 0, 0, 0, 0, 0, 0), (8, 8, 0, 2, 2, 0, 0),
                     (8, 8, 0, 2, 2, 0, 0), (A, A, 0, 1, 3, 1, 0)])

    def test_fused_patch_checks_before_any_device_call(self):
        """The launch entry runs the same check first, so a bad list is
        INVALID_ARGUMENT with or without a GPU; a list with no tile returns
        the digests it was given."""
        with pytest.raises(Exception, match="INVALID_ARGUMENT"):
            gpu.fused_patch([(A, B, 777, 0, 0, 0, 0)], self.LENS, self.OLD_S,
                            self.SIZES, self.OLD_O)
        assert gpu.fused_patch([(0, 0, 0, 0, 0, 0, 0)], self.LENS, self.OLD_S,
                               self.SIZES, self.OLD_O) == (self.OLD_S, self.OLD_O)
        assert gpu.fused_patch([], [], [], [], []) == ([], [])
