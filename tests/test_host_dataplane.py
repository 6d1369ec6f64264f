"""Characterization of the host client's data plane: striped and replicated
batch puts, batch gets that fall back from the compact protocol to the
per-copy one, the force_tcp grouping over several worker endpoints, and the
commit/cancel epilogue after partial failures. CPU only (DRAM tier)."""
import numpy as np
import pytest

import blackbird_amd as bb

from conftest import Cluster

# uneven three-way shard lengths; 12288 is the smallest size that still
# stripes three ways at the default min_shard_size of 4096
SIZES = [12288, 12289, 200001, 3 * 65536 + 5]

NO_SPACE = 2000
OBJECT_NOT_FOUND = 5000
OBJECT_EXISTS = 5001

both_transports = pytest.mark.parametrize("force_tcp", [False, True])


def _blob(seed, size):
    return np.random.default_rng(seed).integers(
        0, 256, size, dtype=np.uint8).tobytes()


def _items(prefix, n, seed=0):
    return [("%s%02d" % (prefix, i), _blob(seed + i, SIZES[i % len(SIZES)]))
            for i in range(n)]


def _cfg(replication=1, max_workers_per_copy=1):
    cfg = bb.PlacementConfig()
    cfg.replication = replication
    cfg.max_workers_per_copy = max_workers_per_copy
    return cfg


def _check_reads(clients, items):
    keys = [k for k, _ in items]
    for c in clients:
        res = c.batch_get(keys)
        assert [s for s, _ in res] == [0] * len(items)
        for (k, d), (_, got) in zip(items, res):
            assert got == d, k
        for k, d in items:
            assert c.get(k) == d, k


def _check_placements(ks, items, ncopies, nshards):
    for k, d in items:
        info = ks.get_workers(k)
        assert info.checksum != 0, k
        assert len(info.copies) == ncopies, k
        for cp in info.copies:
            assert len(cp.shards) == nshards, k
            assert sum(sh.length for sh in cp.shards) == len(d), k
            assert all(sh.digest != 0 for sh in cp.shards), k


@both_transports
def test_striped_batch_roundtrip(cluster3, force_tcp):
    c = cluster3.client(force_tcp=force_tcp, verify_checksum_on_get=True)
    other = cluster3.client(force_tcp=not force_tcp,
                            verify_checksum_on_get=True)
    items = _items("st", 8)
    assert c.batch_put(items, _cfg(max_workers_per_copy=3)) == [0] * 8
    ks = cluster3.keystone.service()
    _check_placements(ks, items, ncopies=1, nshards=3)
    _check_reads([c, other], items)
    assert ks.run_scrub_once() == 0
    c.close()
    other.close()


@both_transports
def test_replicated_and_striped(force_tcp):
    cl = Cluster(n_workers=4)
    try:
        c = cl.client(force_tcp=force_tcp, verify_checksum_on_get=True)
        items = _items("rs", 4, seed=20)
        cfg = _cfg(replication=2, max_workers_per_copy=2)
        assert c.batch_put(items, cfg) == [0] * 4
        ks = cl.keystone.service()
        _check_placements(ks, items, ncopies=2, nshards=2)
        _check_reads([c], items)
        assert ks.run_scrub_once() == 0
        c.close()
    finally:
        cl.stop()


@both_transports
def test_mixed_batch_get(cluster3, force_tcp):
    """Striped items make the compact batch get answer NOT_IMPLEMENTED per
    item; the client reruns the whole batch on the per-copy path."""
    c = cluster3.client(force_tcp=force_tcp, verify_checksum_on_get=True)
    single = _items("one", 3, seed=40)
    striped = _items("tri", 3, seed=50)
    assert c.batch_put(single) == [0] * 3
    assert c.batch_put(striped, _cfg(max_workers_per_copy=3)) == [0] * 3
    ks = cluster3.keystone.service()
    _check_placements(ks, single, ncopies=1, nshards=1)
    _check_placements(ks, striped, ncopies=1, nshards=3)
    mixed = [it for pair in zip(single, striped) for it in pair]
    res = c.batch_get([k for k, _ in mixed])
    assert res == [(0, d) for _, d in mixed]
    res = c.batch_get([single[0][0], "missing", striped[0][0]])
    assert res == [(0, single[0][1]), (OBJECT_NOT_FOUND, b""),
                   (0, striped[0][1])]
    c.close()


@both_transports
@pytest.mark.parametrize("max_workers_per_copy", [1, 3])
def test_partial_failure(cluster3, force_tcp, max_workers_per_copy):
    c = cluster3.client(force_tcp=force_tcp, verify_checksum_on_get=True)
    cfg = _cfg(max_workers_per_copy=max_workers_per_copy)
    first = _blob(60, SIZES[1])
    assert c.batch_put([("dup", first)], cfg) == [0]
    fresh = _blob(62, SIZES[3])
    st = c.batch_put([("dup", _blob(61, SIZES[2])), ("fresh", fresh)], cfg)
    assert st == [OBJECT_EXISTS, 0]
    assert c.get("dup") == first
    assert c.get("fresh") == fresh
    # nothing left pending, nothing wrongly cancelled
    assert c.cluster_stats().num_objects == 2
    c.close()


def test_no_space():
    cl = Cluster(n_workers=1, pool_bytes=1 << 20)
    try:
        c = cl.client(verify_checksum_on_get=True)
        small = _blob(71, 4096)
        st = c.batch_put([("big", _blob(70, 2 << 20)), ("small", small)])
        assert st == [NO_SPACE, 0]
        assert not c.exists("big")
        assert c.get("small") == small
        assert c.cluster_stats().num_objects == 1
        c.close()
    finally:
        cl.stop()
