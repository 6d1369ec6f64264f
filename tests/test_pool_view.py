"""The pool resolver (PoolMapper.local / .remote and PoolView), rung by rung,
through its test-only binding. CPU only."""
import os

import pytest

import blackbird_amd as bb

MB = 1 << 20
POOL = 4 * MB


def _worker(coord, tmp_path, pools):
    wc = bb.WorkerConfig()
    wc.worker_id = "pv%d" % os.getpid()
    wc.data_listen_address = "127.0.0.1:0"
    cfgs = []
    for pool_id, cls in pools:
        p = bb.PoolConfig()
        p.pool_id = pool_id
        p.storage_class = cls
        p.size_bytes = POOL
        if cls == bb.StorageClass.SSD:
            p.mount_path = str(tmp_path)
        cfgs.append(p)
    wc.pools = cfgs
    w = bb.WorkerService(wc, coord)
    w.initialize()
    w.start()
    return w


@pytest.fixture
def worker(coord, tmp_path):
    w = _worker(coord, tmp_path, [("pv_ram", bb.StorageClass.RAM_CPU),
                                  ("pv_ssd", bb.StorageClass.SSD)])
    yield w
    w.stop()


def test_local_ram_pool_is_a_host_view(worker):
    v = bb.PoolMapperForTest.local("pv_ram")
    assert v.base != 0 and not v.device
    assert v.size == POOL
    be = worker.backend("pv_ram")
    assert v.base == be.access_info().base_addr
    # the handle is this pool's backend: bytes written through it show
    # through the view
    assert v.local.storage_class() == bb.StorageClass.RAM_CPU
    assert v.local.capacity() == POOL
    data = os.urandom(4096)
    v.local.write(8192, data)
    assert v.read(8192, 4096) == data
    assert be.read(8192, 4096) == data


def test_stopped_worker_resolves_to_nothing(coord, tmp_path):
    w = _worker(coord, tmp_path, [("pv_gone", bb.StorageClass.RAM_CPU)])
    assert bb.PoolMapperForTest.local("pv_gone").base != 0
    w.stop()
    v = bb.PoolMapperForTest.local("pv_gone")
    assert v.base == 0 and v.local is None and v.size == 0


def test_shm_name_through_a_fresh_mapper_maps_the_same_bytes(worker):
    a = worker.backend("pv_ram").access_info()
    assert a.kind == bb.AccessKind.SHM and a.shm_name
    local = bb.PoolMapperForTest.local("pv_ram")
    mapper = bb.PoolMapperForTest()
    remote = mapper.remote(a)
    assert remote.base != 0 and not remote.device and remote.local is None
    assert remote.size == POOL  # the segment's own size
    assert remote.base != local.base  # a second mapping, not the registry's
    data = os.urandom(4096)
    local.write(POOL - 4096, data)
    assert remote.read(POOL - 4096, 4096) == data
    back = os.urandom(4096)
    remote.write(0, back)
    assert local.read(0, 4096) == back
    # cached by name
    assert mapper.remote(a).base == remote.base


def test_unknown_shm_name_resolves_to_nothing():
    a = bb.AccessInfo()
    a.kind = bb.AccessKind.SHM
    a.shm_name = "/bb_no_such_segment_%d" % os.getpid()
    v = bb.PoolMapperForTest().remote(a)
    assert v.base == 0 and v.size == 0


def test_unmapped_local_pool_has_a_backend_and_no_base(worker):
    v = bb.PoolMapperForTest.local("pv_ssd")
    assert v.base == 0
    assert v.local is not None
    assert v.local.storage_class() == bb.StorageClass.SSD
    data = os.urandom(4096)
    v.local.write(4096, data)
    assert worker.backend("pv_ssd").read(4096, 4096) == data


RANGES = [(POOL - 4096, 8192), (2**64 - 1, 2), (POOL - 4096, 4096)]


def test_contains_with_known_and_unknown_size():
    known = bb.PoolViewForTest(POOL)
    assert [known.contains(o, n) for o, n in RANGES] == [False, False, True]
    unknown = bb.PoolViewForTest(0)
    assert [unknown.contains(o, n) for o, n in RANGES] == [True, True, True]


@pytest.mark.skipif(bb.core.gpu.available(), reason="pins the GPU-less rung")
def test_ipc_access_without_a_gpu_resolves_to_nothing():
    a = bb.AccessInfo()
    a.kind = bb.AccessKind.HIP_IPC
    a.ipc_handle_hex = "00" * 64
    a.device_id = 0
    mapper = bb.PoolMapperForTest()
    for _ in range(2):
        v = mapper.remote(a)
        assert v.base == 0 and not v.device and v.size == 0
