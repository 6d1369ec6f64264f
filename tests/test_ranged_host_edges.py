"""In-place range patches at byte granularity through the host client
(ClientOptions.patch_edge_tiles, no GPU): RAM_CPU clusters. After every patch
the expected digests are checksum_cpu of the patched bytes computed from
scratch. With the option off the routes are those of test_ranged_host.py."""
import os
import subprocess

import numpy as np
import pytest

import blackbird_amd as bb

gpu = bb.core.gpu
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


def _corrupt_at_5000(cluster, blob):
    sh = cluster.keystone.service().get_workers("k").copies[0].shards[0]
    _backend_of(cluster, sh.pool_id).write(sh.offset + 5000,
                                           bytes([blob[5000] ^ 0x20]))


def test_option_defaults_to_off():
    assert bb.ClientOptions().patch_edge_tiles is False


def test_unaligned_patches_in_place(cluster3):
    """The ranges test_ranged_host.py sends down the rewrite route, and a few
    with an interior between the edges."""
    c = cluster3.client(patch_edge_tiles=True)
    blob = _rand(15, 3 * 8 * KB)
    c.put("tri", blob, _cfg(max_workers_per_copy=3))
    c.put("k", blob[:5000])
    for key, nshards, cases in [
            ("tri", 3, [(1, 1024), (1024, 100), (8 * KB - 3, 7),
                        (1000, 3000), (8 * KB - 1000, 8 * KB + 2000),
                        (5, 3 * 8 * KB - 5)]),
            ("k", 1, [(1023, 2), (4096, 903), (4999, 1), (4106, 100),
                      (4090, 910), (1, 4998)])]:
        want = blob if key == "tri" else blob[:5000]
        for seed, (off, n) in enumerate(cases):
            want = _overlay(want, off, _rand(50 + seed, n))
            c.patch(key, off, want[off:off + n])
            _check_object(cluster3, c, key, want, nshards=nshards)
    c.close()


def test_replicated_unaligned(cluster3):
    c = cluster3.client(patch_edge_tiles=True)
    blob = _rand(12, 16 * KB + 5)
    c.put("rep", blob, _cfg(replication=2))
    for seed, (off, n) in enumerate([(3 * KB + 7, 2 * KB), (16 * KB - 1, 3)]):
        blob = _overlay(blob, off, _rand(40 + seed, n))
        c.patch("rep", off, blob[off:off + n])
        _check_object(cluster3, c, "rep", blob, ncopies=2)
    c.close()


def test_in_place_route_does_not_verify_the_object(cluster):
    """The mirror of test_rewrite_route_verifies_what_it_reads: the in-place
    route reads only the tiles it patches, so the patch goes through; the
    digest it records is that of the patched CLEAN bytes, and the corrupt
    byte stays detectable."""
    c = cluster.client(patch_edge_tiles=True)
    blob = _rand(18, 8 * KB)
    c.put("k", blob)
    _corrupt_at_5000(cluster, blob)
    c.patch("k", 1, b"xyz")
    ks = cluster.keystone.service()
    assert ks.get_workers("k").checksum == \
        gpu.checksum_cpu(_overlay(blob, 1, b"xyz"))
    assert c.get_range("k", 0, 8) == blob[:1] + b"xyz" + blob[4:8]
    vc = cluster.client(verify_checksum_on_get=True)
    with pytest.raises(Exception, match="CHECKSUM_MISMATCH"):
        vc.get("k")
    vc.close()
    assert ks.run_scrub_once() == 1
    c.close()


def test_option_off_keeps_the_rewrite_route(cluster):
    c = cluster.client(patch_edge_tiles=False)
    blob = _rand(18, 8 * KB)
    c.put("k", blob)
    _corrupt_at_5000(cluster, blob)
    with pytest.raises(Exception, match="CHECKSUM_MISMATCH"):
        c.patch("k", 1, b"xyz")
    assert cluster.keystone.service().get_workers("k").checksum == \
        gpu.checksum_cpu(blob)
    c.close()


def test_range_past_the_end_changes_nothing(cluster):
    c = cluster.client(patch_edge_tiles=True)
    blob = _rand(21, 4 * KB + 9)
    c.put("k", blob)
    for off, n in [(4 * KB + 9, 1), (3 * KB + 5, KB + 5), (5 * KB, 0)]:
        with pytest.raises(Exception, match="INVALID_ARGUMENT"):
            c.patch("k", off, b"\x00" * n)
    _check_object(cluster, c, "k", blob)
    c.close()


def test_bbctl_patch_edge_tiles(cluster):
    """patch KEY OFF FILE --edge-tiles: in place, so the corrupt byte outside
    the range is not noticed; without the flag the rewrite refuses it."""
    bbctl = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "bin", "bbctl")

    def run(*args, data=None):
        return subprocess.run([bbctl, "--keystone", cluster.keystone.endpoint,
                               *args], input=data, capture_output=True,
                              timeout=20)

    c = cluster.client()
    blob = _rand(60, 8 * KB)
    c.put("k", blob)
    r = run("patch", "k", "1000", "-", "--edge-tiles", data=b"hello")
    assert r.returncode == 0, r.stderr
    blob = _overlay(blob, 1000, b"hello")
    _check_object(cluster, c, "k", blob)
    _corrupt_at_5000(cluster, blob)
    r = run("patch", "k", "1", "-", data=b"xyz")
    assert r.returncode != 0 and b"CHECKSUM_MISMATCH" in r.stderr
    r = run("patch", "k", "1", "-", "--edge-tiles", data=b"xyz")
    assert r.returncode == 0, r.stderr
    assert cluster.keystone.service().get_workers("k").checksum == \
        gpu.checksum_cpu(_overlay(blob, 1, b"xyz"))
    assert b"--edge-tiles" in run("--help").stdout
    c.close()
