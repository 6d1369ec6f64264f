#!/usr/bin/env python3
"""Keystone RPCs by method over one fixed host-client scenario.

The keystone keeps no per-method counter, so the client talks to it through a
small TCP relay in this script that reads the method id out of every request
frame ([u32 body_len][u8 kind][u64 id][u16 method][body], kind 0 = request)
and passes the bytes on untouched. Method names come from rpc/methods.h.

Two clusters, each with a one-sided client and a force_tcp client of its own:

  inproc  three workers in this process, a RAM_CPU and an SSD pool each
  daemon  coordd, keystoned and two workerd (a RAM_CPU pool each) as
          processes of their own, so the client reaches the pools by their
          shm names

The sequence per client: put and get of 1 MiB; batch put and batch get of 4
objects; put and get of 4 objects of 256 KiB striped over the workers. On the
in-process cluster, where the keystone can be told to, one object is then
migrated RAM_CPU -> SSD and back and read after each move.

Two builds that issue the same RPCs print the same JSON line. CPU only.

  python scripts/pool_access_rpc_counts.py
"""
import json
import os
import re
import signal
import socket
import struct
import subprocess
import sys
import tempfile
import threading
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import blackbird_amd as bb  # noqa: E402

MB = 1 << 20
HEADER = struct.Struct("<IBQH")
BIN = os.path.join(REPO, "bin")


def method_names():
    text = open(os.path.join(
        REPO, "csrc/include/blackbird/rpc/methods.h")).read()
    return {int(v): k for k, v in
            re.findall(r"constexpr uint16_t (\w+) = (\d+);", text)}


class CountingRelay:
    """Listens on a loopback port and relays every connection to `target`,
    counting the request frames that pass towards it."""

    def __init__(self, target):
        host, port = target.rsplit(":", 1)
        self.target = (host, int(port))
        self.counts = {}
        self.lock = threading.Lock()
        self.sock = socket.socket()
        self.sock.bind(("127.0.0.1", 0))
        self.sock.listen(16)
        self.endpoint = "127.0.0.1:%d" % self.sock.getsockname()[1]
        threading.Thread(target=self._accept, daemon=True).start()

    def _accept(self):
        while True:
            try:
                down, _ = self.sock.accept()
            except OSError:
                return
            up = socket.create_connection(self.target)
            for s in (down, up):
                s.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
            threading.Thread(target=self._requests, args=(down, up),
                             daemon=True).start()
            threading.Thread(target=self._pump, args=(up, down),
                             daemon=True).start()

    @staticmethod
    def _pump(src, dst):
        try:
            while data := src.recv(1 << 16):
                dst.sendall(data)
        except OSError:
            pass
        for s in (src, dst):
            try:
                s.shutdown(socket.SHUT_RDWR)
            except OSError:
                pass

    def _requests(self, down, up):
        buf = b""
        try:
            while data := down.recv(1 << 16):
                up.sendall(data)
                buf += data
                while len(buf) >= HEADER.size:
                    body_len, kind, _, method = HEADER.unpack_from(buf)
                    if len(buf) < HEADER.size + body_len:
                        break
                    if kind == 0:
                        with self.lock:
                            self.counts[method] = self.counts.get(method, 0) + 1
                    buf = buf[HEADER.size + body_len:]
        except OSError:
            pass
        try:
            up.shutdown(socket.SHUT_RDWR)
        except OSError:
            pass

    def take(self, names):
        with self.lock:
            out = {names.get(m, str(m)): n
                   for m, n in sorted(self.counts.items())}
            self.counts = {}
        return out

    def close(self):
        self.sock.close()


def sequence(c, tag, stripe_over, migrate=None):
    one = os.urandom(MB)
    c.put(tag + "one", one)
    assert c.get(tag + "one") == one
    items = [("%sb%d" % (tag, i), os.urandom(MB)) for i in range(4)]
    assert c.batch_put(items) == [0] * 4
    for (k, d), (s, got) in zip(items, c.batch_get([k for k, _ in items])):
        assert s == 0 and got == d, k
    cfg = bb.PlacementConfig()
    cfg.max_workers_per_copy = stripe_over
    striped = [("%ss%d" % (tag, i), os.urandom(256 << 10))
               for i in range(4)]
    assert c.batch_put(striped, cfg) == [0] * 4
    for (k, d), (s, got) in zip(striped,
                                c.batch_get([k for k, _ in striped])):
        assert s == 0 and got == d, k
    for k, d in striped:
        assert c.get(k) == d, k
    if migrate:
        for cls in (bb.StorageClass.SSD, bb.StorageClass.RAM_CPU):
            migrate(tag + "one", cls)
            assert c.get(tag + "one") == one, cls


def run_clients(relay, names, stripe_over, migrate=None):
    out = {}
    for label, force_tcp in (("one_sided", False), ("force_tcp", True)):
        o = bb.ClientOptions()
        o.keystone_endpoint = relay.endpoint
        o.force_tcp = force_tcp
        o.verify_checksum_on_get = True
        c = bb.Client(o)
        c.connect()
        sequence(c, label[0], stripe_over, migrate)
        c.close()
        out[label] = relay.take(names)
    return out


def inproc(names, tmp):
    cs = bb.CoordServer()
    cs.start("127.0.0.1", 0)
    ep = "127.0.0.1:%d" % cs.port
    kc = bb.KeystoneConfig()
    kc.listen_address = "127.0.0.1:0"
    kc.coord_endpoint = ep
    kc.gc_interval_ms = 100000
    srv = bb.create_and_start_keystone(kc)
    ks = srv.service()
    workers = []
    for i in range(3):
        wc = bb.WorkerConfig()
        wc.worker_id = "w%d" % i
        wc.coord_endpoint = ep
        wc.data_listen_address = "127.0.0.1:0"
        pools = []
        for cls, name in ((bb.StorageClass.RAM_CPU, "ram"),
                          (bb.StorageClass.SSD, "ssd")):
            p = bb.PoolConfig()
            p.pool_id = "%s%d" % (name, i)
            p.storage_class = cls
            p.size_bytes = 32 * MB
            if cls == bb.StorageClass.SSD:
                p.mount_path = tmp
            pools.append(p)
        wc.pools = pools
        w = bb.WorkerService(wc)
        w.initialize()
        w.start()
        workers.append(w)
    deadline = time.time() + 5
    while time.time() < deadline and len(ks.get_memory_pools()) < 6:
        time.sleep(0.05)
    relay = CountingRelay(srv.endpoint)
    try:
        return run_clients(relay, names, 3, ks.migrate_object)
    finally:
        relay.close()
        for w in workers:
            w.stop()
        srv.stop()
        ks.stop()
        cs.stop()


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def daemon(names, tmp):
    coord_port, ks_port = free_port(), free_port()
    procs = []

    def spawn(args, log):
        procs.append(subprocess.Popen(
            args, stdout=open(os.path.join(tmp, log), "w"),
            stderr=subprocess.STDOUT))

    try:
        spawn([BIN + "/coordd", "--listen-host", "127.0.0.1",
               "--listen-port", str(coord_port)], "coordd.log")
        time.sleep(0.3)
        spawn([BIN + "/keystoned", "--listen-address",
               "127.0.0.1:%d" % ks_port, "--coord-endpoint",
               "127.0.0.1:%d" % coord_port], "keystoned.log")
        time.sleep(0.3)
        for i in range(2):
            cfg = {"worker_id": "dw%d" % i,
                   "coord_endpoint": "127.0.0.1:%d" % coord_port,
                   "data_listen_address": "127.0.0.1:0",
                   "pools": [{"pool_id": "dpool%d" % i,
                              "storage_class": "RAM_CPU",
                              "size_bytes": 64 * MB}]}
            path = os.path.join(tmp, "worker%d.json" % i)
            with open(path, "w") as f:
                json.dump(cfg, f)
            spawn([BIN + "/workerd", "--config", path], "workerd%d.log" % i)
        probe = bb.ClientOptions()
        probe.keystone_endpoint = "127.0.0.1:%d" % ks_port
        deadline = time.time() + 10
        while True:
            try:
                c = bb.Client(probe)
                c.connect()
                pools = c.memory_pools()
                c.close()
                if len(pools) == 2:
                    break
            except Exception:
                pass
            if time.time() > deadline:
                raise SystemExit("daemon cluster did not assemble")
            time.sleep(0.2)
        relay = CountingRelay(probe.keystone_endpoint)
        try:
            return run_clients(relay, names, 2)
        finally:
            relay.close()
    finally:
        for p in procs:
            p.send_signal(signal.SIGTERM)
        for p in procs:
            try:
                p.wait(timeout=5)
            except subprocess.TimeoutExpired:
                p.kill()


def main():
    names = method_names()
    with tempfile.TemporaryDirectory() as tmp:
        print(json.dumps({"inproc": inproc(names, tmp),
                          "daemon": daemon(names, tmp)}, sort_keys=True))


if __name__ == "__main__":
    main()
