"""RPC layer edge cases: unknown methods, handler exceptions, oversized and
concurrent traffic, connection lifecycle. (The layer is otherwise covered
indirectly through every coordination/keystone test.)"""
import threading

import pytest

import blackbird_amd as bb


@pytest.fixture
def coord_pair(coord_server):
    c = bb.CoordClient()
    c.connect("127.0.0.1:%d" % coord_server.port)
    yield coord_server, c
    c.close()


class TestRpcEdgeCases:
    def test_large_values_roundtrip(self, coord_pair):
        _, c = coord_pair
        big = "x" * (8 << 20)  # 8 MiB value through the framed protocol
        c.put("/big", big)
        assert c.get("/big") == big

    def test_binary_safe_values(self, coord_pair):
        _, c = coord_pair
        blob = bytes(range(256)).decode("latin1") * 17
        c.put("/bin", blob)
        assert c.get("/bin") == blob

    def test_concurrent_calls_one_connection(self, coord_pair):
        _, c = coord_pair
        errors = []

        def worker(tid):
            try:
                for i in range(100):
                    c.put(f"/t{tid}/k{i}", str(i))
                    assert c.get(f"/t{tid}/k{i}") == str(i)
            except Exception as e:  # pragma: no cover
                errors.append(e)

        ts = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert not errors

    def test_server_survives_abrupt_disconnects(self, coord_server):
        import socket
        for _ in range(5):
            s = socket.socket()
            s.connect(("127.0.0.1", coord_server.port))
            s.send(b"\xff" * 10)  # garbage partial frame
            s.close()
        c = bb.CoordClient()
        c.connect("127.0.0.1:%d" % coord_server.port)
        c.put("/alive", "yes")
        assert c.get("/alive") == "yes"
        c.close()

    def test_call_on_closed_client_errors_cleanly(self, coord_server):
        c = bb.CoordClient()
        c.connect("127.0.0.1:%d" % coord_server.port)
        c.close()
        # endpoint still up → auto-redial succeeds and the call completes
        c2 = bb.CoordClient()
        c2.connect("127.0.0.1:%d" % coord_server.port)
        c2.close()
        coord_server.stop()
        with pytest.raises(Exception):
            c2.put("/x", "y")  # server gone → clean error, no hang


class TestHostileFrames:
    """Protocol robustness: raw garbage on the wire must never take the
    server down or wedge other connections."""

    def _sock(self, port):
        import socket
        s = socket.socket()
        s.settimeout(3)
        s.connect(("127.0.0.1", port))
        return s

    def _assert_alive(self, coord_server):
        c = bb.CoordClient()
        c.connect("127.0.0.1:%d" % coord_server.port)
        c.put("/alive", "yes")
        assert c.get("/alive") == "yes"
        c.close()

    def test_random_garbage(self, coord_server):
        import os as _os
        for _ in range(8):
            s = self._sock(coord_server.port)
            s.sendall(_os.urandom(64))
            s.close()
        self._assert_alive(coord_server)

    def test_oversized_length_header(self, coord_server):
        import struct
        s = self._sock(coord_server.port)
        # header: u32 len, u8 kind, pad, u64 id, u16 method (packed layout
        # irrelevant — a huge len must be rejected before any allocation)
        s.sendall(struct.pack("<I", 0xFFFFFFFF) + b"\x00" * 16)
        s.close()
        self._assert_alive(coord_server)

    def test_truncated_frame_then_disconnect(self, coord_server):
        import struct
        s = self._sock(coord_server.port)
        s.sendall(struct.pack("<I", 1024) + b"\x00" * 12)  # promises 1 KiB
        s.close()                                          # never sends it
        self._assert_alive(coord_server)

    def test_unknown_method_is_an_error_not_a_crash(self, coord_pair):
        server, c = coord_pair
        # CoordClient has no raw-call surface; garbage METHOD bytes reach the
        # server through a hand-built frame instead
        import struct
        s = self._sock(server.port)
        # replicate the wire header shape: u32 len, u8 kind(REQUEST=0),
        # 3 pad, u64 id, u16 method, 6 pad — conservative: send a plausible
        # 24-byte header + tiny body; whatever the exact packing, the server
        # must at worst drop the connection
        s.sendall(struct.pack("<IB3xQH6x", 4, 0, 1, 9999) + b"\x00\x01\x02\x03")
        try:
            s.recv(64)
        except Exception:
            pass
        s.close()
        self._assert_alive(server)


class TestDataPlaneHostile:
    """Malformed/hostile requests against the worker's network-exposed data
    port must be rejected with a clean error before any large allocation or
    out-of-bounds memory access (ADVICE round-1 highs)."""

    HDR = "<IBQH"  # u32 body_len, u8 kind, u64 id, u16 method (packed, 15 B)
    DATA_READ = 201
    DATA_PULL = 206

    def _call(self, endpoint, method, body, timeout=10.0):
        import socket
        import struct
        host, port = endpoint.rsplit(":", 1)
        s = socket.create_connection((host, int(port)), timeout=timeout)
        s.settimeout(timeout)
        try:
            s.sendall(struct.pack(self.HDR, len(body), 0, 1, method) + body)
            hdr = b""
            while len(hdr) < 15:
                chunk = s.recv(15 - len(hdr))
                if not chunk:
                    raise ConnectionError("server closed")
                hdr += chunk
            body_len, kind, rid, m = struct.unpack(self.HDR, hdr)
            resp = b""
            while len(resp) < body_len:
                chunk = s.recv(min(65536, body_len - len(resp)))
                if not chunk:
                    raise ConnectionError("short response")
                resp += chunk
            status = struct.unpack("<i", resp[:4])[0]
            (msg_len,) = struct.unpack("<I", resp[4:8])
            msg = resp[8:8 + msg_len].decode(errors="replace")
            return status, msg, resp[8 + msg_len:]
        finally:
            s.close()

    @staticmethod
    def _s(txt):
        import struct
        b = txt.encode()
        return struct.pack("<I", len(b)) + b

    def test_data_read_huge_length_rejected(self, cluster):
        import struct
        pool = cluster.workers[0].pool_descriptors()[0]
        # length = 16 GiB: must be rejected before the response buffer resize
        body = self._s(pool.pool_id) + struct.pack("<QQ", 0, 16 << 30)
        status, msg, _ = self._call(cluster.workers[0].data_endpoint,
                                    self.DATA_READ, body)
        assert status != 0
        assert "out of bounds" in msg

    def test_data_read_beyond_capacity_rejected(self, cluster):
        import struct
        pool = cluster.workers[0].pool_descriptors()[0]
        body = self._s(pool.pool_id) + struct.pack("<QQ", 0, pool.size + 4096)
        status, msg, _ = self._call(cluster.workers[0].data_endpoint,
                                    self.DATA_READ, body)
        assert status != 0

    def test_data_pull_dst_out_of_bounds_rejected(self, cluster):
        import struct
        w = cluster.workers[0]
        pool = w.pool_descriptors()[0]
        # craft a PullReq whose dst range overflows the destination pool and
        # whose src resolves locally (same pool) — without the bounds check
        # this memcpy'd past the pool
        length = 1 << 20
        dst_offset = pool.size - 4096  # dst_offset + length >> capacity
        body = bb.core.encode_pull_req_for_test(
            pool.pool_id, dst_offset, length, pool.pool_id, 0, length)
        status, msg, _ = self._call(w.data_endpoint, self.DATA_PULL, body)
        assert status != 0
        assert "out of bounds" in msg

    def test_data_pull_src_out_of_bounds_rejected(self, cluster):
        w = cluster.workers[0]
        pool = w.pool_descriptors()[0]
        # src slice overruns the (locally resolved) source pool
        length = 1 << 20
        body = bb.core.encode_pull_req_for_test(
            pool.pool_id, 0, length, pool.pool_id, pool.size - 4096, length)
        status, msg, _ = self._call(w.data_endpoint, self.DATA_PULL, body)
        assert status != 0
        assert "out of bounds" in msg

    def test_data_pull_hostile_vector_count_is_protocol_error(self, cluster):
        import struct
        w = cluster.workers[0]
        pool = w.pool_descriptors()[0]
        # PullReq: dst_pool, dst_offset, total_len, srcs — claim 2^32-1 shard
        # placements with no bytes behind them. The serde guard must surface a
        # decode failure (PROTOCOL_ERROR), not a valid empty vector.
        body = (self._s(pool.pool_id) + struct.pack("<QQ", 0, 0)
                + struct.pack("<I", 0xFFFFFFFF))
        status, msg, _ = self._call(w.data_endpoint, self.DATA_PULL, body)
        assert status != 0
        assert "bad request" in msg


# ---------------------------------------------------------------------------
# v2 batch wire codec (csrc/client/batch_wire.*), reached through the
# batch_wire_{encode,decode}_for_test bindings.

NOT_IMPLEMENTED = 1001
OBJECT_NOT_FOUND = 5000


def _cfg(**kw):
    cfg = bb.PlacementConfig()
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


CFG_FIELDS = ("replication", "max_workers_per_copy", "min_shard_size",
              "preferred_class", "required_class", "ttl_ms", "checksum",
              "preferred_worker", "replace")


def _put_resp(items):
    return {"view_version": 7, "token": 0x1122334455667788,
            "pools": ["hbm0", "pool-b"], "items": items}


def _places(n):
    return [(c % 2, 4096 * c + 256) for c in range(n)]


def _wire_cases():
    """(message, value, nitems) for every shape the codec must carry."""
    cases = []
    for items in ([("a", 4096), ("bb", 4096), ("ccc", 4096)],      # uniform
                  [("a", 1), ("bb", 1023), ("ccc", 65536 + 17)],   # per-item
                  []):                                             # empty
        for want in (False, True):
            cases.append(("put_start2_req",
                          {"items": items, "want_token": want,
                           "cfg": _cfg(replication=2, replace=True,
                                       preferred_worker="w1",
                                       preferred_class=bb.StorageClass.RAM_GPU)},
                          0))
    ok = lambda n: {"status": 0, "places": _places(n)}
    err = {"status": OBJECT_NOT_FOUND}
    for items in ([ok(1)], [ok(1), err, ok(2)], [ok(9), ok(1)], []):
        cases.append(("put_start2_resp", _put_resp(items), len(items)))
    gok = lambda n, size: {"status": 0, "size": size,
                           "checksum": 0xDEADBEEF00000000 + n,
                           "places": _places(n)}
    for items in ([gok(1, 4096)],
                  [gok(1, 1), err, gok(2, 65536 + 17)],
                  [gok(9, 4096), {"status": NOT_IMPLEMENTED}, gok(1, 4096)],
                  []):
        cases.append(("get_workers2_resp",
                      {"pools": ["hbm0", "pool-b"], "items": items},
                      len(items)))
    for keys in (["a", "bb", "ccc"], []):
        cases.append(("get_workers2_req", {"keys": keys}, 0))
    cases.append(("upsert_start", {"token": 0x0102030405060708}, 0))
    for digests in ([], [1], [0xFFFFFFFFFFFFFFFF, 2, 3]):
        for release in (False, True):
            cases.append(("commit_token", {"token": 99, "release": release,
                                           "digests": digests}, 0))
    return cases


def _same(msg, want, got):
    if msg == "put_start2_req":
        assert got["items"] == want["items"]
        assert got["want_token"] == want["want_token"]
        for f in CFG_FIELDS:
            assert getattr(got["cfg"], f) == getattr(want["cfg"], f), f
    else:
        assert got == want


class TestBatchWireCodec:
    def test_round_trip(self):
        for msg, value, n in _wire_cases():
            body = bb.core.batch_wire_encode_for_test(msg, value)
            _same(msg, value, bb.core.batch_wire_decode_for_test(msg, body, n))

    def test_out_of_range_pool_index_is_reported(self):
        """The decoder hands an index past the pool table to the caller
        (every caller has its own policy for it) instead of dropping it."""
        v = _put_resp([{"status": 0, "places": [(0, 0), (5, 64)]}])
        body = bb.core.batch_wire_encode_for_test("put_start2_resp", v)
        got = bb.core.batch_wire_decode_for_test("put_start2_resp", body, 1)
        assert got["items"][0]["places"] == [(0, 0), (5, 64)]
        assert len(got["pools"]) == 2

    def test_truncation_is_protocol_error(self):
        for msg, value, n in _wire_cases():
            body = bb.core.batch_wire_encode_for_test(msg, value)
            for cut in range(len(body)):
                if msg == "put_start2_req" and cut == len(body) - 1:
                    # the trailing want_token byte is optional on the wire
                    # (requests from before it existed): without it the
                    # request decodes, asking for no token
                    got = bb.core.batch_wire_decode_for_test(msg, body[:cut])
                    assert got["want_token"] is False
                    assert got["items"] == value["items"]
                    continue
                with pytest.raises(bb.core.BlackbirdError,
                                   match="PROTOCOL_ERROR"):
                    bb.core.batch_wire_decode_for_test(msg, body[:cut], n)

    def test_commit_token_rejects_trailing_byte(self):
        body = bb.core.batch_wire_encode_for_test(
            "commit_token", {"token": 5, "release": True, "digests": [1, 2]})
        assert bb.core.batch_wire_decode_for_test("commit_token", body)
        with pytest.raises(bb.core.BlackbirdError, match="PROTOCOL_ERROR"):
            bb.core.batch_wire_decode_for_test("commit_token", body + b"\0")

    def test_hostile_count_is_protocol_error(self):
        import struct
        for msg, body in (
                ("get_workers2_req", struct.pack("<I", 0xFFFFFFFF)),
                ("put_start2_req", struct.pack("<IQ", 0xFFFFFFFF, 4096)),
                ("commit_token", struct.pack("<QBI", 1, 0, 0xFFFFFFFF))):
            with pytest.raises(bb.core.BlackbirdError, match="PROTOCOL_ERROR"):
                bb.core.batch_wire_decode_for_test(msg, body)

    # One frozen vector per message, written out by hand from the layout in
    # batch_wire.h (little-endian, u32-length-prefixed strings) and checked
    # once against a build from before the codec existed, in both directions.
    GOLDEN = {
        "put_start2_req": (
            {"items": [("k0", 4096), ("key1", 100)], "want_token": True,
             "cfg": None},
            "02000000" "0000000000000000"            # count, non-uniform
            "0010000000000000" "6400000000000000"    # sizes
            "02000000" "6b30" "04000000" "6b657931"  # keys
            "02000000" "01000000" "0010000000000000"  # repl, stripes, min shard
            "01" "01" "00" "0000000000000000"        # preferred RAM_GPU, no req
            "01" "02000000" "7731" "01"              # checksum, "w1", replace
            "01"),                                   # want_token
        "put_start2_resp": (
            {"view_version": 3, "token": 0x0A0B, "pools": ["hbm0", "p1"],
             "items": [{"status": 0, "places": [(0, 256), (1, 512)]},
                       {"status": OBJECT_NOT_FOUND}]},
            "0300000000000000" "0b0a000000000000"
            "0200" "04000000" "68626d30" "02000000" "7031"
            "00" "02" "0000" "0001000000000000" "0100" "0002000000000000"
            "01" "88130000"),
        "get_workers2_req": (
            {"keys": ["k0", "key1"]},
            "02000000" "02000000" "6b30" "04000000" "6b657931"),
        "get_workers2_resp": (
            {"pools": ["hbm0"],
             "items": [{"status": 0, "size": 4096, "checksum": 0x1234,
                        "places": [(0, 256)]},
                       {"status": NOT_IMPLEMENTED}]},
            "0100" "04000000" "68626d30"
            "00" "0010000000000000" "3412000000000000" "01"
            "0000" "0001000000000000"
            "01" "e9030000"),
        "upsert_start": ({"token": 0x0102030405060708}, "0807060504030201"),
        "commit_token": (
            {"token": 9, "release": True, "digests": [1, 0x0203]},
            "0900000000000000" "01" "02000000"
            "0100000000000000" "0302000000000000"),
    }

    def test_frozen_layout(self):
        nitems = {"put_start2_resp": 2, "get_workers2_resp": 2}
        for msg, (value, hexed) in self.GOLDEN.items():
            if msg == "put_start2_req":
                value = dict(value, cfg=_cfg(
                    replication=2, replace=True, preferred_worker="w1",
                    preferred_class=bb.StorageClass.RAM_GPU))
            body = bb.core.batch_wire_encode_for_test(msg, value)
            assert body.hex() == hexed, msg
            _same(msg, value, bb.core.batch_wire_decode_for_test(
                msg, bytes.fromhex(hexed), nitems.get(msg, 0)))
