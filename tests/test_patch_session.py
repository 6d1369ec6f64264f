"""Patch sessions, the parts that need no GPU: the keystone's patch start by
token over host-tier clusters, BATCH_PATCH_START_TOKEN over the wire and its
layout, and the argument check of the patch session plan. Every expected
digest is checksum_cpu of the bytes, computed from scratch."""
import struct
import time

import numpy as np
import pytest

import blackbird_amd as bb

from conftest import Cluster

gpu = bb.core.gpu
KB = 1024
SIZE = 8 * KB
KEYS = ["p0", "p1", "p2"]  # p1 is replicated x2; all are striped over two


def _rand(seed, n):
    return np.random.default_rng(seed).bytes(n)


def _cfg(replication=1, replace=False):
    cfg = bb.PlacementConfig()
    cfg.max_workers_per_copy = 2
    cfg.replication = replication
    cfg.replace = replace
    return cfg


def _replication(key):
    return 2 if key == "p1" else 1


def _expected(svc, blobs):
    """(object checksums, shard digests in object, copy, shard order) of
    `blobs` as the keystone lays them out, hashed from scratch."""
    objs, shards = [], []
    for key, blob in blobs:
        objs.append(gpu.checksum_cpu(blob))
        # the lengths are read while the object is readable; the digests are
        # not taken from there
        for copy in svc.get_workers(key).copies:
            assert len(copy.shards) == 2  # striped for real
            off = 0
            for sh in copy.shards:
                shards.append(gpu.checksum_cpu(blob[off:off + sh.length]))
                off += sh.length
            assert off == len(blob)
    return objs, shards


def _recorded(svc, key):
    info = svc.get_workers(key)
    return info.checksum, [[s.digest for s in c.shards] for c in info.copies]


def _assert_pending(svc, key):
    with pytest.raises(Exception, match="OBJECT_NOT_COMMITTED"):
        svc.get_workers(key)


@pytest.fixture
def cluster4():
    c = Cluster(n_workers=4)
    yield c
    c.stop()


@pytest.fixture
def session(cluster4):
    """Three striped objects put through the host client (which records every
    shard's digest) and a striped session over them."""
    svc = cluster4.keystone.service()
    client = cluster4.client()
    blobs = [(k, _rand(100 + i, SIZE)) for i, k in enumerate(KEYS)]
    for key, blob in blobs:
        client.put(key, blob, _cfg(_replication(key)))
    assert [len(svc.get_workers(k).copies) for k in KEYS] == [1, 2, 1]
    tok = svc.create_put_session(KEYS, SIZE, _cfg(), allow_striped=True)
    assert tok != 0
    yield cluster4, svc, client, blobs, tok
    client.close()


# ------------------------------------------------------------------ keystone

class TestPatchStartToken:
    def test_answers_recorded_digests_then_pins_and_commits(self, session):
        _, svc, _, blobs, tok = session
        want_objs, want_shards = _expected(svc, blobs)
        assert len(want_shards) == 8  # 2 + 2*2 + 2
        objs, shards = svc.patch_start_token(tok)
        assert objs == want_objs
        assert shards == want_shards
        for k in KEYS:
            _assert_pending(svc, k)
        # PENDING from a patch start: an abort would put them back (and does,
        # for one, to show that it is the patch kind of PENDING)
        assert svc.batch_patch_abort(["p2"]) == [0]
        assert _recorded(svc, "p2") == (want_objs[2], [want_shards[6:8]])
        # a second start finds p0 and p1 PENDING: refused, p2 not flipped
        with pytest.raises(Exception, match="INVALID_STATE"):
            svc.patch_start_token(tok)
        assert _recorded(svc, "p2")[0] == want_objs[2]
        assert svc.batch_patch_abort(["p0", "p1"]) == [0, 0]

        before = svc.token_commits()
        svc.patch_start_token(tok)
        new_objs = [0xA0, 0xA1, 0xA2]
        new_shards = [0x10, 0x11, 0x20, 0x21, 0x22, 0x23, 0x30, 0x31]
        svc.commit_token_shards(tok, new_objs, new_shards)
        assert svc.token_commits() == before + 1
        assert _recorded(svc, "p0") == (0xA0, [[0x10, 0x11]])
        assert _recorded(svc, "p1") == (0xA1, [[0x20, 0x21], [0x22, 0x23]])
        assert _recorded(svc, "p2") == (0xA2, [[0x30, 0x31]])
        # the next step is answered what the last one committed
        assert svc.patch_start_token(tok) == (new_objs, new_shards)
        svc.commit_token_shards(tok, new_objs, new_shards)
        assert svc.token_commits() == before + 2
        # an abort after a commit finds nothing to abort: the commit cleared
        # the patch mark
        assert svc.batch_patch_abort(["p0"]) != [0]

    def test_second_start_while_pending_changes_nothing(self, session):
        _, svc, _, blobs, tok = session
        want = _expected(svc, blobs)
        svc.patch_start_token(tok)
        for _ in range(2):
            with pytest.raises(Exception, match="INVALID_STATE"):
                svc.patch_start_token(tok)
        for k in KEYS:
            _assert_pending(svc, k)
        # still the patch kind of PENDING, digests kept
        assert svc.batch_patch_abort(KEYS) == [0, 0, 0]
        assert svc.patch_start_token(tok) == want

    def test_pending_from_an_upsert_start_is_refused_too(self, session):
        _, svc, _, blobs, tok = session
        svc.upsert_start_token(tok)
        with pytest.raises(Exception, match="INVALID_STATE"):
            svc.patch_start_token(tok)
        # untouched: not the patch kind of PENDING
        assert svc.batch_patch_abort(KEYS) != [0, 0, 0]

    def test_object_without_checksum_flips_none(self, session):
        _, svc, _, blobs, _ = session
        # last in the list, so that a start that flipped as it went would
        # have flipped the three before it
        svc.put_start("bare", SIZE, _cfg())
        svc.put_complete("bare", 0)
        keys = KEYS + ["bare"]
        tok = svc.create_put_session(keys, SIZE, _cfg(), allow_striped=True)
        assert tok != 0
        with pytest.raises(Exception, match="INVALID_STATE"):
            svc.patch_start_token(tok)
        want_objs, _ = _expected(svc, blobs)  # get_workers: all readable
        assert [_recorded(svc, k)[0] for k in KEYS] == want_objs
        assert all(st != 0 for st in svc.batch_patch_abort(keys))

    def test_object_without_shard_digests_flips_none(self, session):
        _, svc, _, blobs, _ = session
        svc.put_start("noshards", SIZE, _cfg())
        svc.put_complete("noshards", 0x5EED)  # a checksum, no shard digests
        assert _recorded(svc, "noshards") == (0x5EED, [[0, 0]])
        keys = KEYS + ["noshards"]
        tok = svc.create_put_session(keys, SIZE, _cfg(), allow_striped=True)
        with pytest.raises(Exception, match="INVALID_STATE"):
            svc.patch_start_token(tok)
        assert all(st != 0 for st in svc.batch_patch_abort(keys))

    def test_removed_key_and_unknown_token_are_stale(self, session):
        _, svc, _, _, tok = session
        with pytest.raises(Exception, match="SESSION_STALE"):
            svc.patch_start_token(tok + 12345)
        svc.remove_object("p1")
        with pytest.raises(Exception, match="SESSION_STALE"):
            svc.patch_start_token(tok)
        for k in ("p0", "p2"):
            svc.get_workers(k)  # still readable: nothing flipped

    def test_another_clients_reput_in_place_is_answered(self, session):
        cluster, svc, _, blobs, tok = session
        other = cluster.client()
        try:
            fresh = _rand(777, SIZE)
            other.put("p1", fresh, _cfg(2, replace=True))
        finally:
            other.close()
        blobs = [(k, fresh if k == "p1" else b) for k, b in blobs]
        want = _expected(svc, blobs)
        assert svc.patch_start_token(tok) == want

    def test_standby_answers_not_leader(self, coord):
        def mk():
            cfg = bb.KeystoneConfig()
            cfg.enable_ha = True
            cfg.gc_interval_ms = 100000
            k = bb.KeystoneService(cfg, coord)
            k.initialize()
            k.start()
            return k

        k1 = mk()
        deadline = time.time() + 5
        while time.time() < deadline and not k1.is_leader():
            time.sleep(0.02)
        assert k1.is_leader()
        k2 = mk()
        try:
            assert not k2.is_leader()
            with pytest.raises(Exception, match="NOT_LEADER"):
                k2.patch_start_token(1)
            with pytest.raises(Exception, match="SESSION_STALE"):
                k1.patch_start_token(1)
        finally:
            k2.stop()
            k1.stop()


# --------------------------------------------------- BATCH_PATCH_START_TOKEN

class TestPatchStartTokenRpc:
    def test_client_call_mirrors_the_service(self, session):
        _, svc, client, blobs, tok = session
        want = _expected(svc, blobs)
        with pytest.raises(Exception, match="SESSION_STALE"):
            client.patch_start_token(tok + 999)
        assert client.patch_start_token(tok) == want
        for k in KEYS:
            _assert_pending(svc, k)
        with pytest.raises(Exception, match="INVALID_STATE"):
            client.patch_start_token(tok)
        before = svc.token_commits()
        client.commit_by_token_shards(tok, want[0], want[1])
        assert svc.token_commits() == before + 1
        assert client.get("p1") == blobs[1][1]

    def test_session_opened_while_a_patch_start_holds_the_objects(self, session):
        # the client's order: BATCH_PATCH_START, BATCH_SESSION_OPEN, commit
        _, svc, client, blobs, _ = session
        want = _expected(svc, blobs)
        assert [st for st, _ in svc.batch_patch_start(KEYS)] == [0, 0, 0]
        tok = client.open_session([(k, SIZE) for k in KEYS], True)
        assert tok != 0
        client.commit_by_token_shards(tok, want[0], want[1])
        assert client.patch_start_token(tok) == want
        client.commit_by_token_shards(tok, want[0], want[1])


# ---------------------------------------------------------------------- wire

class TestWire:
    CASES = [
        ("patch_start_token", {"token": 0}),
        ("patch_start_token", {"token": 0x0102030405060708}),
        ("patch_start_token_resp", {"obj_digests": [], "shard_digests": []}),
        ("patch_start_token_resp", {"obj_digests": [1, 0xFFFFFFFFFFFFFFFF],
                                    "shard_digests": [3, 4, 5, 6]}),
    ]

    def test_round_trip(self):
        for msg, value in self.CASES:
            body = bb.core.batch_wire_encode_for_test(msg, value)
            assert bb.core.batch_wire_decode_for_test(msg, body) == value

    def test_truncated_bodies_are_protocol_errors(self):
        for msg, value in self.CASES:
            body = bb.core.batch_wire_encode_for_test(msg, value)
            for cut in range(len(body)):
                with pytest.raises(bb.core.BlackbirdError,
                                   match="PROTOCOL_ERROR"):
                    bb.core.batch_wire_decode_for_test(msg, body[:cut])

    def test_trailing_byte_and_counts_larger_than_the_body(self):
        body = bb.core.batch_wire_encode_for_test(*self.CASES[3])
        for msg, hostile in (
                ("patch_start_token_resp", body + b"\0"),
                ("patch_start_token_resp", struct.pack("<I", 0xFFFFFFFF)),
                ("patch_start_token_resp", struct.pack("<IQ", 2, 5)),
                ("patch_start_token_resp",
                 struct.pack("<IQI", 1, 5, 0xFFFFFFFF)),
                ("patch_start_token_resp",
                 struct.pack("<IQIQ", 1, 5, 2, 7)),
                ("patch_start_token", struct.pack("<QB", 1, 0))):
            with pytest.raises(bb.core.BlackbirdError, match="PROTOCOL_ERROR"):
                bb.core.batch_wire_decode_for_test(msg, hostile)

    def test_frozen_layout(self):
        # written out by hand from the layouts in batch_wire.h (little endian)
        golden = {
            "patch_start_token": ({"token": 0x0102030405060708},
                                  "0807060504030201"),
            "patch_start_token_resp": (
                {"obj_digests": [0x0A], "shard_digests": [1, 0x0203]},
                "01000000" "0a00000000000000"
                "02000000" "0100000000000000" "0302000000000000"),
        }
        for msg, (value, hexed) in golden.items():
            body = bb.core.batch_wire_encode_for_test(msg, value)
            assert body.hex() == hexed, msg
            assert bb.core.batch_wire_decode_for_test(
                msg, bytes.fromhex(hexed)) == value


# ---------------------------------------------------------------- plan check

class TestPlanChecksBeforeAnyDeviceCall:
    # one shard of four tiles that is its whole object; the check runs before
    # any device call, so these raise the same with and without a GPU
    LENS, SIZES, OLD = [4 * KB], [4 * KB], [0x1234]

    def plan(self, segs):
        return gpu.fused_patch_plan(segs, self.LENS, self.SIZES, self.OLD,
                                    self.OLD, 1)

    def test_run_covering_a_tile_of_another_run(self):
        segs = [(0x10000, 0x20000, 2 * KB, 0, 0, 0, 0),
                (0x30000, 0x20400, 2 * KB, 1, 1, 0, 0)]
        with pytest.raises(bb.core.BlackbirdError, match="INVALID_ARGUMENT"):
            self.plan(segs)

    def test_misaligned_address(self):
        for src, dst in [(0x10008, 0x20000), (0x10000, 0x20004)]:
            with pytest.raises(bb.core.BlackbirdError,
                               match="INVALID_ARGUMENT"):
                self.plan([(src, dst, KB, 0, 0, 0, 0)])

    def test_one_old_digest_per_shard_and_object(self):
        with pytest.raises(bb.core.BlackbirdError, match="INVALID_ARGUMENT"):
            gpu.fused_patch_plan([(0x10000, 0x20000, KB, 0, 0, 0, 0)],
                                 self.LENS, self.SIZES, [], self.OLD, 1)
