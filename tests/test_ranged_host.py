"""Byte-range get and in-place range patch through the host client and the
keystone (no GPU): RAM_CPU clusters. After every patch the expected digests
are checksum_cpu of the patched bytes computed from scratch."""
import numpy as np
import pytest

import blackbird_amd as bb

from conftest import Cluster

gpu = bb.core.gpu
INVALID_STATE = 1004         # ErrorCode values (common/error.h)
OBJECT_NOT_FOUND = 5000
OBJECT_NOT_COMMITTED = 5004
KB = 1024


def _rand(seed, n):
    return np.random.default_rng(seed).bytes(n)


def _cfg(replication=1, max_workers_per_copy=1):
    cfg = bb.PlacementConfig()
    cfg.replication = replication
    cfg.max_workers_per_copy = max_workers_per_copy
    return cfg


def _overlay(blob, offset, new):
    return blob[:offset] + new + blob[offset + len(new):]


def _check_object(cl, c, key, want, ncopies=1, nshards=1):
    """A full get returns `want`; the keystone's checksum and every shard
    digest are the CPU digests of `want`; the scrubber agrees."""
    assert c.get(key) == want
    ks = cl.keystone.service()
    info = ks.get_workers(key)
    assert info.size == len(want)
    assert info.checksum == gpu.checksum_cpu(want)
    assert len(info.copies) == ncopies
    for copy in info.copies:
        assert len(copy.shards) == nshards
        off = 0
        for sh in copy.shards:
            assert sh.digest == gpu.checksum_cpu(want[off:off + sh.length]), off
            off += sh.length
        assert off == len(want)
    assert ks.run_scrub_once() == 0
    vc = cl.client(verify_checksum_on_get=True)
    try:
        assert vc.get(key) == want
    finally:
        vc.close()


def _backend_of(cl, pool_id):
    w = next(w for w in cl.workers
             if any(p.pool_id == pool_id for p in w.pool_descriptors()))
    return w.backend(pool_id)


class TestGetRange:
    def test_offsets_and_ends(self, cluster):
        c = cluster.client()
        blob = _rand(1, 5 * KB + 123)
        c.put("k", blob)
        for off, n in [(0, 1), (0, 1024), (1, 1023), (1, 2048), (1023, 2),
                       (1023, 3000), (0, len(blob)), (len(blob) - 1, 1),
                       (4096, len(blob) - 4096), (len(blob), 0), (7, 0)]:
            assert c.get_range("k", off, n) == blob[off:off + n], (off, n)
        c.close()

    def test_one_byte_past_the_end(self, cluster):
        c = cluster.client()
        blob = _rand(2, 3000)
        c.put("k", blob)
        for off, n in [(0, 3001), (2999, 2), (3000, 1), (3001, 0),
                       (1 << 63, 1 << 63)]:
            with pytest.raises(Exception, match="INVALID_ARGUMENT"):
                c.get_range("k", off, n)
        with pytest.raises(Exception, match="OBJECT_NOT_FOUND"):
            c.get_range("missing", 0, 1)
        c.close()

    @pytest.mark.parametrize("force_tcp", [False, True])
    def test_across_shard_boundaries_of_a_striped_object(self, cluster3,
                                                         force_tcp):
        c = cluster3.client(force_tcp=force_tcp)
        blob = _rand(3, 3 * 8 * KB)
        c.put("tri", blob, _cfg(max_workers_per_copy=3))
        shards = cluster3.keystone.service().get_workers("tri").copies[0].shards
        assert [s.length for s in shards] == [8 * KB] * 3
        for off, n in [(8 * KB - 1, 2), (8 * KB - 100, 8 * KB + 200),
                       (1, len(blob) - 1), (16 * KB, 8 * KB), (16 * KB - 1, 1),
                       (len(blob) - 1, 1), (0, len(blob))]:
            assert c.get_range("tri", off, n) == blob[off:off + n], (off, n)
        c.close()


class TestPatch:
    def test_single_shard(self, cluster):
        c = cluster.client()
        blob = _rand(10, 3 * KB + 777)
        c.put("k", blob)
        for seed, (off, n) in enumerate([(1024, 1024), (0, 1024), (3072, 777),
                                         (1024, 2825), (0, len(blob))]):
            blob = _overlay(blob, off, _rand(20 + seed, n))
            c.patch("k", off, blob[off:off + n])
            _check_object(cluster, c, "k", blob)
        # a 1-byte object, whole
        c.put("one", b"\x01")
        c.patch("one", 0, b"\xfe")
        _check_object(cluster, c, "one", b"\xfe")
        c.close()

    def test_striped(self, cluster3):
        c = cluster3.client()
        blob = _rand(11, 3 * 8 * KB)
        c.put("tri", blob, _cfg(max_workers_per_copy=3))
        for seed, (off, n) in enumerate([(2 * KB, KB), (7 * KB, 2 * KB),
                                         (4 * KB, 16 * KB), (23 * KB, KB)]):
            blob = _overlay(blob, off, _rand(30 + seed, n))
            c.patch("tri", off, blob[off:off + n])
            _check_object(cluster3, c, "tri", blob, nshards=3)
        c.close()

    def test_replicated(self, cluster3):
        c = cluster3.client()
        blob = _rand(12, 16 * KB + 5)
        c.put("rep", blob, _cfg(replication=2))
        for seed, (off, n) in enumerate([(3 * KB, 2 * KB), (16 * KB, 5)]):
            blob = _overlay(blob, off, _rand(40 + seed, n))
            c.patch("rep", off, blob[off:off + n])
            _check_object(cluster3, c, "rep", blob, ncopies=2)
        c.close()

    def test_in_place_patch_reads_only_its_range(self, cluster):
        """A byte corrupted outside the range: the in-place patch goes
        through, the digest it records is that of the patched CLEAN bytes,
        so the corruption stays detectable — a re-hash of the pool would have
        laundered it."""
        c = cluster.client()
        blob = _rand(13, 8 * KB)
        c.put("k", blob)
        sh = cluster.keystone.service().get_workers("k").copies[0].shards[0]
        _backend_of(cluster, sh.pool_id).write(sh.offset + 5000,
                                               bytes([blob[5000] ^ 0x20]))
        new = _rand(14, 2 * KB)
        c.patch("k", KB, new)
        want = _overlay(blob, KB, new)
        ks = cluster.keystone.service()
        assert ks.get_workers("k").checksum == gpu.checksum_cpu(want)
        assert c.get_range("k", KB, 2 * KB) == new
        vc = cluster.client(verify_checksum_on_get=True)
        with pytest.raises(Exception, match="CHECKSUM_MISMATCH"):
            vc.get("k")
        vc.close()
        assert ks.run_scrub_once() == 1
        c.close()

    def test_unaligned_patch_takes_the_rewrite_route(self, cluster3):
        c = cluster3.client()
        blob = _rand(15, 3 * 8 * KB)
        c.put("tri", blob, _cfg(max_workers_per_copy=3))
        c.put("k", blob[:5000])
        for key, nshards, cases in [
                ("tri", 3, [(1, 1024), (1024, 100), (8 * KB - 3, 7)]),
                ("k", 1, [(1023, 2), (4096, 903), (4999, 1)])]:
            want = blob if key == "tri" else blob[:5000]
            for seed, (off, n) in enumerate(cases):
                want = _overlay(want, off, _rand(50 + seed, n))
                c.patch(key, off, want[off:off + n])
                _check_object(cluster3, c, key, want, nshards=nshards)
        # shards that do not start on tiles: plan_stripe refuses the copy
        odd = _rand(16, 3 * 8 * KB - 100)
        c.put("odd", odd, _cfg(max_workers_per_copy=3))
        lens = [s.length for s in
                cluster3.keystone.service().get_workers("odd").copies[0].shards]
        assert gpu.plan_stripe(len(odd), lens) is None
        odd = _overlay(odd, 2048, _rand(17, 1024))
        c.patch("odd", 2048, odd[2048:3072])
        _check_object(cluster3, c, "odd", odd, nshards=3)
        c.close()

    def test_rewrite_route_verifies_what_it_reads(self, cluster):
        """The rewrite route does re-hash the whole object, so it must not
        put corrupt bytes back under a fresh digest."""
        c = cluster.client()
        blob = _rand(18, 8 * KB)
        c.put("k", blob)
        sh = cluster.keystone.service().get_workers("k").copies[0].shards[0]
        _backend_of(cluster, sh.pool_id).write(sh.offset + 5000,
                                               bytes([blob[5000] ^ 0x20]))
        with pytest.raises(Exception, match="CHECKSUM_MISMATCH"):
            c.patch("k", 1, b"xyz")
        # still committed, still the old digest
        assert cluster.keystone.service().get_workers("k").checksum == \
            gpu.checksum_cpu(blob)
        c.close()

    def test_object_without_a_recorded_checksum(self, cluster):
        c = cluster.client()
        blob = _rand(19, 4 * KB)
        cfg = _cfg()
        cfg.checksum = False
        c.put("nock", blob, cfg)
        ks = cluster.keystone.service()
        assert ks.get_workers("nock").checksum == 0
        assert [st for st, _ in ks.batch_patch_start(["nock"])] == [INVALID_STATE]
        assert c.get("nock") == blob  # state unchanged
        new = _rand(20, KB)
        c.patch("nock", KB, new)
        _check_object(cluster, c, "nock", _overlay(blob, KB, new))
        c.close()

    def test_range_past_the_end_changes_nothing(self, cluster):
        c = cluster.client()
        blob = _rand(21, 4 * KB)
        c.put("k", blob)
        for off, n in [(4 * KB, 1), (3 * KB, KB + 1), (5 * KB, 0)]:
            with pytest.raises(Exception, match="INVALID_ARGUMENT"):
                c.patch("k", off, b"\x00" * n)
        _check_object(cluster, c, "k", blob)
        c.close()

    def test_missing_key(self, cluster):
        c = cluster.client()
        with pytest.raises(Exception, match="OBJECT_NOT_FOUND"):
            c.patch("missing", 0, b"\x00" * 1024)
        ks = cluster.keystone.service()
        assert [st for st, _ in ks.batch_patch_start(["missing"])] == \
            [OBJECT_NOT_FOUND]
        c.close()

    def test_pending_key(self, cluster):
        c = cluster.client()
        ks = cluster.keystone.service()
        ks.put_start("pend", 4 * KB, _cfg())
        with pytest.raises(Exception, match="OBJECT_NOT_COMMITTED"):
            c.patch("pend", 0, b"\x00" * 1024)
        # a key already being patched is PENDING too
        c.put("k", _rand(22, 4 * KB))
        assert [st for st, _ in ks.batch_patch_start(["k"])] == [0]
        assert [st for st, _ in ks.batch_patch_start(["k", "pend"])] == \
            [OBJECT_NOT_COMMITTED] * 2
        with pytest.raises(Exception, match="OBJECT_NOT_COMMITTED"):
            c.patch("k", 0, b"\x00" * 1024)
        c.close()


class TestPatchStartAndAbort:
    def test_start_pins_and_abort_restores(self, cluster3):
        c = cluster3.client()
        ks = cluster3.keystone.service()
        blob = _rand(23, 3 * 8 * KB)
        c.put("tri", blob, _cfg(max_workers_per_copy=3))
        before = ks.get_workers("tri")
        (st, info), = ks.batch_patch_start(["tri"])
        assert st == 0
        # the answer carries what the patch moves: size, checksum, digests
        assert info.size == len(blob)
        assert info.checksum == before.checksum == gpu.checksum_cpu(blob)
        assert [s.digest for s in info.copies[0].shards] == \
            [s.digest for s in before.copies[0].shards]
        assert all(s.digest for s in info.copies[0].shards)
        # PENDING: not readable, and an upsert of the key is refused a slot
        with pytest.raises(Exception, match="OBJECT_NOT_COMMITTED"):
            c.get("tri")
        assert not ks.object_exists("tri")
        assert ks.batch_patch_abort(["tri"]) == [0]
        after = ks.get_workers("tri")
        assert after.checksum == before.checksum
        assert [(s.pool_id, s.offset, s.length, s.digest)
                for s in after.copies[0].shards] == \
            [(s.pool_id, s.offset, s.length, s.digest)
             for s in before.copies[0].shards]
        _check_object(cluster3, c, "tri", blob, nshards=3)
        c.close()

    def test_abort_of_a_key_that_is_not_being_patched(self, cluster):
        c = cluster.client()
        ks = cluster.keystone.service()
        c.put("k", _rand(24, 2 * KB))
        ks.put_start("pend", 4 * KB, _cfg())
        # committed, pending from a put, missing
        assert ks.batch_patch_abort(["k", "pend", "missing"]) == \
            [INVALID_STATE, INVALID_STATE, OBJECT_NOT_FOUND]
        # a second abort finds the key committed again
        assert [st for st, _ in ks.batch_patch_start(["k"])] == [0]
        assert ks.batch_patch_abort(["k", "k"]) == [0, INVALID_STATE]
        # an in-place upsert's PENDING is not a patch's
        cfg = _cfg()
        cfg.replace = True
        ks.put_start("k", 2 * KB, cfg)
        assert ks.batch_patch_abort(["k"]) == [INVALID_STATE]
        c.close()

    def test_commit_after_start_is_the_ordinary_put_complete(self, cluster):
        c = cluster.client()
        ks = cluster.keystone.service()
        c.put("k", _rand(25, 2 * KB))
        assert [st for st, _ in ks.batch_patch_start(["k"])] == [0]
        ks.put_complete("k", 0x1234)
        assert ks.get_workers("k").checksum == 0x1234
        assert ks.batch_patch_abort(["k"]) == [INVALID_STATE]
        c.close()

    def test_cancel_after_start_removes_the_key(self, cluster):
        """The route after a write that failed midway: the bytes are torn."""
        c = cluster.client()
        ks = cluster.keystone.service()
        c.put("k", _rand(26, 2 * KB))
        assert [st for st, _ in ks.batch_patch_start(["k"])] == [0]
        ks.put_cancel("k")
        with pytest.raises(Exception, match="OBJECT_NOT_FOUND"):
            c.get("k")
        c.close()


def test_bbctl_ranged_get_and_patch(cluster):
    """The CLI forms: get KEY --range OFF:LEN, patch KEY OFF FILE."""
    import os
    import subprocess
    bbctl = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "bin", "bbctl")

    def run(*args, data=None):
        return subprocess.run([bbctl, "--keystone", cluster.keystone.endpoint,
                               *args], input=data, capture_output=True,
                              timeout=20)

    c = cluster.client()
    blob = _rand(60, 4 * KB + 10)
    c.put("cli", blob)
    r = run("get", "cli", "--range", "1023:2050")
    assert r.returncode == 0 and r.stdout == blob[1023:3073]
    r = run("get", "cli", "--range", "4000:200")
    assert r.returncode != 0 and b"INVALID_ARGUMENT" in r.stderr
    new = _rand(61, 2 * KB)
    r = run("patch", "cli", "1024", "-", data=new)
    assert r.returncode == 0, r.stderr
    _check_object(cluster, c, "cli", _overlay(blob, KB, new))
    r = run("patch", "missing", "0", "-", data=new)
    assert r.returncode != 0 and b"OBJECT_NOT_FOUND" in r.stderr
    c.close()
