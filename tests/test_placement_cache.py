"""The client's verified placement cache and its session bindings (no GPU):
what is stored, and exactly which mutations end a binding. A binding is a
session's hold on the digest slots of an ordered key list; a session step
that still holds one after an erase, a move or a clear must be refused."""
import pytest

import blackbird_amd as bb

KEYS = ["pc%02d" % i for i in range(8)]


def entry(i, digest=None, pool="hbm0", offset=None, size=4096):
    return (pool, i * 4096 if offset is None else offset, size,
            0x1000 + i if digest is None else digest)


def fresh(keys=KEYS):
    c = bb.PlacementCache()
    c.set_enabled(True)
    b = c.record([(k, entry(i)) for i, k in enumerate(keys)], bind_keys=keys)
    assert b.bound
    return c, b


def test_record_find_roundtrip_and_zero_digest_skipped():
    c = bb.PlacementCache()
    c.set_enabled(True)
    c.record([("a", entry(1)), ("z", entry(2, digest=0))])
    assert c.find("a") == entry(1)
    assert c.find("z") is None


def test_binding_reads_in_key_order_and_refresh_is_seen_by_find():
    order = [KEYS[5], KEYS[0], KEYS[3]]
    c, _ = fresh()
    b = c.record([], bind_keys=order)
    assert c.digests(b) == [0x1005, 0x1000, 0x1003]
    assert c.refresh(b, [7, 8, 9])
    assert [c.find(k)[3] for k in order] == [7, 8, 9]


def test_new_digest_at_same_placement_keeps_binding():
    c, b = fresh()
    c.record([(KEYS[2], entry(2, digest=0xbeef))])
    assert c.digests(b)[2] == 0xbeef


@pytest.mark.parametrize("moved", [
    entry(2, pool="hbm1"), entry(2, offset=1 << 20), entry(2, size=8192)])
def test_moved_placement_ends_binding(moved):
    c, b = fresh()
    c.record([(KEYS[2], moved)])
    assert c.digests(b) is None
    assert not c.refresh(b, [1] * len(KEYS))


@pytest.mark.parametrize("mutate", [
    lambda c: c.erase([KEYS[1]]),            # a bound key
    lambda c: c.erase(["unbound"]),          # cached, outside the binding
    lambda c: c.erase(["never-recorded"]),   # absent
    lambda c: c.clear(),
    lambda c: c.set_enabled(True),
    lambda c: c.set_enabled(False),
], ids=["erase-bound", "erase-unbound", "erase-absent", "clear", "enable",
        "disable"])
def test_mutations_end_binding(mutate):
    c, b = fresh()
    c.record([("unbound", entry(99))])
    assert c.digests(b) is not None
    mutate(c)
    assert c.digests(b) is None
    assert not c.refresh(b, [1] * len(KEYS))


def test_disable_empties_the_cache():
    c, _ = fresh()
    c.set_enabled(False)
    assert not c.enabled
    c.set_enabled(True)
    assert all(c.find(k) is None for k in KEYS)


def test_binding_survives_rehashes():
    c, b = fresh()
    c.record([("other%05d" % i, entry(i)) for i in range(10000)])
    assert c.digests(b) == [0x1000 + i for i in range(len(KEYS))]


def test_binding_with_a_missing_key_fails():
    c, _ = fresh()
    assert not c.record([], bind_keys=[KEYS[0], "missing", KEYS[1]]).bound


def test_binding_refused_by_another_cache():
    _, b = fresh()
    other, _ = fresh()
    assert other.digests(b) is None
    assert not other.refresh(b, [1] * len(KEYS))


def test_lookup_hits_need_size_within_capacity():
    c, _ = fresh()
    lk = c.lookup([(KEYS[0], 4096), (KEYS[1], 4095), ("absent", 1 << 20),
                   (KEYS[3], 1 << 20)])
    assert lk.hits == [(0, entry(0)), (3, entry(3))]
    assert lk.misses == [1, 2]


@pytest.mark.parametrize("erase_between", [False, True])
def test_settle_binds_only_if_nothing_was_invalidated(erase_between):
    c, _ = fresh()
    lk = c.lookup([(k, 4096) for k in KEYS])
    if erase_between:
        c.erase(["unrelated"])
    b = c.settle(lk, [], True)
    assert b.bound == (not erase_between)
    assert c.digests(b) == (
        None if erase_between else [0x1000 + i for i in range(len(KEYS))])


def test_settle_erases_stale_keys_and_does_not_bind():
    c, held = fresh()
    lk = c.lookup([(k, 4096) for k in KEYS])
    assert not c.settle(lk, [KEYS[4]], True).bound
    assert c.find(KEYS[4]) is None and c.find(KEYS[5]) == entry(5)
    assert c.digests(held) is None


def test_settle_does_not_bind_over_a_miss():
    c, _ = fresh()
    lk = c.lookup([(KEYS[0], 4096), ("absent", 4096)])
    assert not c.settle(lk, [], True).bound
