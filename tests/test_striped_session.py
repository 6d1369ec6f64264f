"""Batch sessions over striped placements, the parts that need no GPU: the
keystone's striped put sessions and the commit that carries every shard's own
digest, BATCH_SESSION_OPEN over a real cluster, the wire layout of the two new
messages, striped entries of the placement cache, and the argument check of
the striped session plan."""
import pytest

import blackbird_amd as bb

from conftest import Cluster

MB = 1 << 20
SIZE = 8192


def make_pool(pool_id, worker):
    p = bb.MemoryPool()
    p.pool_id = pool_id
    p.worker_id = worker
    p.node_id = "node0"
    p.storage_class = bb.StorageClass.RAM_CPU
    p.size = 64 * MB
    return p


def make_ks(coord, nworkers):
    cfg = bb.KeystoneConfig()
    cfg.gc_interval_ms = 100000  # manual GC in tests
    k = bb.KeystoneService(cfg, coord)
    k.initialize()
    k.start()
    for i in range(nworkers):
        k.register_pool(make_pool("p%d" % i, "w%d" % i))
    return k


@pytest.fixture
def ks2(coord):
    k = make_ks(coord, 2)
    yield k
    k.stop()


def striped_cfg(replication=1):
    cfg = bb.PlacementConfig()
    cfg.max_workers_per_copy = 2
    cfg.replication = replication
    cfg.replace = True
    return cfg


def put_striped(ks, keys, cfg, ncopies=1):
    for k in keys:
        copies = ks.put_start(k, SIZE, cfg)
        assert len(copies) == ncopies
        assert all(len(c.shards) == 2 for c in copies)  # striped for real
        ks.put_complete(k, 1)


def digests_of(ks, key):
    info = ks.get_workers(key)
    return info.checksum, [[s.digest for s in c.shards] for c in info.copies]


def assert_pending(ks, key):
    with pytest.raises(Exception, match="OBJECT_NOT_COMMITTED"):
        ks.get_workers(key)


# ------------------------------------------------------------------ keystone

class TestStripedPutSession:
    KEYS = ["s0", "s1", "s2"]

    def test_striped_needs_allow_striped(self, ks2):
        cfg = striped_cfg()
        put_striped(ks2, self.KEYS, cfg)
        assert ks2.create_put_session(self.KEYS, SIZE, cfg) == 0
        assert ks2.create_put_session(self.KEYS, SIZE, cfg,
                                      allow_striped=False) == 0
        assert ks2.create_put_session(self.KEYS, SIZE, cfg,
                                      allow_striped=True) != 0

    def test_commit_stamps_checksum_and_each_shard_digest(self, ks2):
        cfg = striped_cfg()
        put_striped(ks2, self.KEYS, cfg)
        tok = ks2.create_put_session(self.KEYS, SIZE, cfg, allow_striped=True)
        before = ks2.token_commits()
        ks2.upsert_start_token(tok)
        assert_pending(ks2, "s1")
        ks2.commit_token_shards(tok, [0xA0, 0xA1, 0xA2],
                                [0x10, 0x11, 0x20, 0x21, 0x30, 0x31])
        assert ks2.token_commits() == before + 1
        assert digests_of(ks2, "s0") == (0xA0, [[0x10, 0x11]])
        assert digests_of(ks2, "s1") == (0xA1, [[0x20, 0x21]])
        assert digests_of(ks2, "s2") == (0xA2, [[0x30, 0x31]])
        # the session is kept (release=False): a second step works
        ks2.upsert_start_token(tok)
        ks2.commit_token_shards(tok, [1, 2, 3], [4, 5, 6, 7, 8, 9])
        assert digests_of(ks2, "s2") == (3, [[8, 9]])

    @pytest.mark.parametrize("objs,shards", [
        ([0xBAD] * 2, [0xBAD] * 6),   # wrong n
        ([0xBAD] * 4, [0xBAD] * 6),
        ([0xBAD] * 3, [0xBAD] * 5),   # wrong m
        ([0xBAD] * 3, [0xBAD] * 7),
        ([0xBAD] * 3, []),
    ])
    def test_wrong_counts_apply_nothing(self, ks2, objs, shards):
        cfg = striped_cfg()
        put_striped(ks2, self.KEYS, cfg)
        tok = ks2.create_put_session(self.KEYS, SIZE, cfg, allow_striped=True)
        ks2.upsert_start_token(tok)
        ks2.commit_token_shards(tok, [1, 2, 3], [4, 5, 6, 7, 8, 9])
        ks2.upsert_start_token(tok)
        with pytest.raises(Exception, match="INVALID_ARGUMENT"):
            ks2.commit_token_shards(tok, objs, shards)
        for k in self.KEYS:
            assert_pending(ks2, k)
        # nothing of the refused commit stuck: the shard digests are still
        # the previous step's (PENDING hides them, so look after a commit by
        # key that carries no shard digests)
        for k in self.KEYS:
            ks2.put_complete(k, 0x77)
        assert digests_of(ks2, "s0") == (0x77, [[4, 5]])
        assert digests_of(ks2, "s2") == (0x77, [[8, 9]])

    def test_plain_commit_token_refuses_a_striped_session(self, ks2):
        cfg = striped_cfg()
        put_striped(ks2, self.KEYS, cfg)
        tok = ks2.create_put_session(self.KEYS, SIZE, cfg, allow_striped=True)
        ks2.upsert_start_token(tok)
        with pytest.raises(Exception, match="INVALID_ARGUMENT"):
            ks2.commit_token(tok, [1, 2, 3])
        for k in self.KEYS:
            assert_pending(ks2, k)
        ks2.commit_token_shards(tok, [1, 2, 3], [4, 5, 6, 7, 8, 9])
        assert digests_of(ks2, "s1") == (2, [[6, 7]])

    def test_removing_another_object_makes_both_calls_stale(self, ks2):
        cfg = striped_cfg()
        put_striped(ks2, self.KEYS + ["other"], cfg)
        tok = ks2.create_put_session(self.KEYS, SIZE, cfg, allow_striped=True)
        ks2.remove_object("other")
        with pytest.raises(Exception, match="SESSION_STALE"):
            ks2.upsert_start_token(tok)
        with pytest.raises(Exception, match="SESSION_STALE"):
            ks2.commit_token_shards(tok, [1, 2, 3], [4, 5, 6, 7, 8, 9])
        assert digests_of(ks2, "s0") == (1, [[0, 0]])

    def test_replicated_and_striped_takes_copy_shard_order(self, coord):
        ks = make_ks(coord, 4)
        try:
            cfg = striped_cfg(replication=2)
            put_striped(ks, ["r0", "r1"], cfg, ncopies=2)
            tok = ks.create_put_session(["r0", "r1"], SIZE, cfg,
                                        allow_striped=True)
            assert tok != 0
            ks.upsert_start_token(tok)
            with pytest.raises(Exception, match="INVALID_ARGUMENT"):
                ks.commit_token_shards(tok, [1, 2], [1, 2, 3, 4])  # one copy's
            ks.commit_token_shards(tok, [0xC0, 0xC1],
                                   [1, 2, 3, 4, 5, 6, 7, 8])
            assert digests_of(ks, "r0") == (0xC0, [[1, 2], [3, 4]])
            assert digests_of(ks, "r1") == (0xC1, [[5, 6], [7, 8]])
        finally:
            ks.stop()

    def test_single_shard_session_commits_through_shards_call(self, ks2):
        cfg = bb.PlacementConfig()
        cfg.replication = 2
        keys = ["one0", "one1"]
        for k in keys:
            copies = ks2.put_start(k, SIZE, cfg)
            assert [len(c.shards) for c in copies] == [1, 1]
            ks2.put_complete(k, 1)
        tok = ks2.create_put_session(keys, SIZE, cfg)  # no allow_striped
        assert tok != 0
        ks2.upsert_start_token(tok)
        with pytest.raises(Exception, match="INVALID_ARGUMENT"):
            ks2.commit_token_shards(tok, [5, 6], [5, 6])  # m = copies, not n
        ks2.commit_token_shards(tok, [5, 6], [5, 5, 6, 6])
        assert digests_of(ks2, "one0") == (5, [[5], [5]])
        assert digests_of(ks2, "one1") == (6, [[6], [6]])
        # and the one-digest commit still serves it
        ks2.upsert_start_token(tok)
        ks2.commit_token(tok, [8, 9])
        assert digests_of(ks2, "one1") == (9, [[9], [9]])


# -------------------------------------------------------- BATCH_SESSION_OPEN

class TestSessionOpenRpc:
    @pytest.fixture
    def cluster2(self):
        c = Cluster(n_workers=2)
        yield c
        c.stop()

    def test_granted_only_while_pending(self, cluster2):
        svc = cluster2.keystone.service()
        client = cluster2.client()
        try:
            cfg = striped_cfg()
            objs = [("o0", SIZE), ("o1", SIZE)]
            assert client.open_session(objs, True) == 0  # missing keys
            for k, _ in objs:
                assert len(svc.put_start(k, SIZE, cfg)[0].shards) == 2
            # between the start and the commit: granted — striped only on
            # request
            assert client.open_session(objs, False) == 0
            assert client.open_session([("o0", SIZE), ("o1", SIZE + 1)],
                                       True) == 0  # size mismatch
            assert client.open_session(objs + [("nope", SIZE)], True) == 0
            tok = client.open_session(objs, True)
            assert tok != 0
            client.commit_by_token_shards(tok, [0xD0, 0xD1], [1, 2, 3, 4])
            assert digests_of(svc, "o0") == (0xD0, [[1, 2]])
            assert digests_of(svc, "o1") == (0xD1, [[3, 4]])
            # COMMITTED now: refused
            assert client.open_session(objs, True) == 0
            # the session opened while PENDING serves later steps
            svc.upsert_start_token(tok)
            with pytest.raises(Exception, match="INVALID_ARGUMENT"):
                client.commit_by_token_shards(tok, [1, 2], [1, 2, 3])
            client.commit_by_token_shards(tok, [7, 8], [9, 10, 11, 12],
                                          release=True)
            assert digests_of(svc, "o1") == (8, [[11, 12]])
            with pytest.raises(Exception, match="SESSION_STALE"):
                svc.upsert_start_token(tok)  # released
        finally:
            client.close()


# ---------------------------------------------------------------------- wire

class TestWire:
    CASES = [
        ("session_open", {"items": [], "allow_striped": False}),
        ("session_open", {"items": [("a", 1), ("key-two", 1 << 40)],
                          "allow_striped": True}),
        ("session_open_resp", {"token": 0}),
        ("session_open_resp", {"token": 0x0102030405060708}),
        ("commit_token_shards", {"token": 7, "release": False,
                                 "obj_digests": [], "shard_digests": []}),
        ("commit_token_shards", {"token": 7, "release": True,
                                 "obj_digests": [1, 0xFFFFFFFFFFFFFFFF],
                                 "shard_digests": [3, 4, 5, 6]}),
    ]

    @staticmethod
    def same(a, b):
        assert set(a) == set(b)
        for k in a:
            va, vb = a[k], b[k]
            if k == "items":
                va, vb = [tuple(x) for x in va], [tuple(x) for x in vb]
            assert va == vb, k

    def test_round_trip(self):
        for msg, value in self.CASES:
            body = bb.core.batch_wire_encode_for_test(msg, value)
            self.same(value, bb.core.batch_wire_decode_for_test(msg, body))

    def test_truncated_bodies_are_protocol_errors(self):
        for msg, value in self.CASES:
            body = bb.core.batch_wire_encode_for_test(msg, value)
            for cut in range(len(body)):
                with pytest.raises(bb.core.BlackbirdError,
                                   match="PROTOCOL_ERROR"):
                    bb.core.batch_wire_decode_for_test(msg, body[:cut])

    def test_trailing_byte_and_hostile_counts(self):
        import struct
        body = bb.core.batch_wire_encode_for_test(*self.CASES[5])
        with pytest.raises(bb.core.BlackbirdError, match="PROTOCOL_ERROR"):
            bb.core.batch_wire_decode_for_test("commit_token_shards",
                                               body + b"\0")
        for msg, hostile in (
                ("session_open", struct.pack("<I", 0xFFFFFFFF)),
                ("commit_token_shards", struct.pack("<QBI", 1, 0, 0xFFFFFFFF)),
                ("commit_token_shards",
                 struct.pack("<QBIQI", 1, 0, 1, 5, 0xFFFFFFFF))):
            with pytest.raises(bb.core.BlackbirdError, match="PROTOCOL_ERROR"):
                bb.core.batch_wire_decode_for_test(msg, hostile)

    # Written out by hand from the layouts in batch_wire.h (little endian;
    # str = u32 length + bytes).
    GOLDEN = {
        "session_open": (
            {"items": [("ab", 0x1000), ("c", 2)], "allow_striped": True},
            "02000000"
            "02000000" "6162" "0010000000000000"
            "01000000" "63" "0200000000000000"
            "01"),
        "session_open_resp": ({"token": 0x0102030405060708},
                              "0807060504030201"),
        "commit_token_shards": (
            {"token": 9, "release": True, "obj_digests": [0x0A],
             "shard_digests": [1, 0x0203]},
            "0900000000000000" "01"
            "01000000" "0a00000000000000"
            "02000000" "0100000000000000" "0302000000000000"),
    }

    def test_frozen_layout(self):
        for msg, (value, hexed) in self.GOLDEN.items():
            body = bb.core.batch_wire_encode_for_test(msg, value)
            assert body.hex() == hexed, msg
            self.same(value, bb.core.batch_wire_decode_for_test(
                msg, bytes.fromhex(hexed)))


# ----------------------------------------------------------- placement cache

class TestStripedCacheEntries:
    SHARDS = [("hbm0", 4096, 4096), ("hbm1", 8192, 4096)]

    def fresh(self):
        c = bb.PlacementCache()
        c.set_enabled(True)
        b = c.record_striped([("st", SIZE, 0x51, self.SHARDS)],
                             bind_keys=["st"])
        assert b.bound
        return c, b

    def test_records_binds_and_refreshes(self):
        c, b = self.fresh()
        assert c.find_shards("st") == self.SHARDS
        # the single-range fields name shard 0; the digest is the object's
        assert c.find("st") == ("hbm0", 4096, SIZE, 0x51)
        assert c.digests(b) == [0x51]
        assert c.refresh(b, [0x52])
        assert c.find("st")[3] == 0x52
        lk = c.lookup([("st", SIZE), ("st", SIZE - 1)])
        assert [i for i, _ in lk.hits] == [0] and lk.misses == [1]

    def test_identical_rerecord_keeps_bindings(self):
        c, b = self.fresh()
        c.record_striped([("st", SIZE, 0x99, list(self.SHARDS))])
        assert c.digests(b) == [0x99]

    @pytest.mark.parametrize("which", [0, 1])
    def test_one_shard_offset_changed_kills_bindings(self, which):
        c, b = self.fresh()
        moved = list(self.SHARDS)
        pool, off, ln = moved[which]
        moved[which] = (pool, off + (1 << 20), ln)
        c.record_striped([("st", SIZE, 0x51, moved)])
        assert c.digests(b) is None
        assert not c.refresh(b, [1])
        assert c.find_shards("st") == moved

    def test_striped_to_single_range_is_a_move(self):
        c, b = self.fresh()
        c.record([("st", ("hbm0", 4096, SIZE, 0x51))])
        assert c.digests(b) is None
        assert c.find_shards("st") == []

    def test_single_range_entry_keeps_its_4_tuple(self):
        c = bb.PlacementCache()
        c.set_enabled(True)
        c.record([("plain", ("hbm0", 0, 4096, 0x77))])
        assert c.find("plain") == ("hbm0", 0, 4096, 0x77)
        assert c.find_shards("plain") == []
        assert c.find_shards("absent") is None


# ---------------------------------------------------------------- plan check

def test_plan_rejects_partial_tile_inside_object_without_a_gpu():
    # 1000 bytes in the middle of a 4096-byte object: only a segment that
    # ends at its object's end may end mid-tile. The check runs before any
    # device call, so this raises the same with and without a GPU.
    segs = [(0x1000, 0x2000, 1000, 0, 0), (0x1400, 0x2400, 3072, 1, 0)]
    with pytest.raises(bb.core.BlackbirdError, match="INVALID_ARGUMENT"):
        bb.core.gpu.fused_stripe_plan(segs, [4096], 1)
    with pytest.raises(bb.core.BlackbirdError, match="INVALID_ARGUMENT"):
        bb.core.gpu.fused_stripe_plan([(0x1000, 0x2000, 16, 0, 3)], [16], 1)
