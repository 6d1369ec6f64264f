"""Storage backend tests: two-phase shard protocol, IO, checksum, stats for
the SHM/pinned/disk tiers (HBM tier is covered in test_gpu.py).
Mirrors reference tests/storage/test_iouring_disk_backend.cpp."""
import os

import pytest

import blackbird_amd as bb

MB = 1 << 20


def make(cls, size=16 * MB, tmpdir=None, pool_id="t0"):
    cfg = bb.PoolConfig()
    cfg.pool_id = pool_id
    cfg.storage_class = cls
    cfg.size_bytes = size
    if tmpdir is not None:
        cfg.mount_path = str(tmpdir)
    return bb.make_backend(cfg, "testw%d" % os.getpid())


CLASSES = [
    (bb.StorageClass.RAM_CPU, False),
    (bb.StorageClass.PINNED_CPU, False),
    (bb.StorageClass.NVME, True),
    (bb.StorageClass.SSD, True),
    (bb.StorageClass.HDD, True),
    (bb.StorageClass.CXL_MEM, False),  # no DAX path: the anonymous fallback
]


@pytest.mark.parametrize("cls,needs_dir", CLASSES)
class TestBackend:
    def test_reserve_commit_io(self, cls, needs_dir, tmp_path):
        b = make(cls, tmpdir=tmp_path if needs_dir else None,
                 pool_id="a_%s" % cls.name)
        t = b.reserve(4096)
        b.commit(t.token_id)
        data = os.urandom(4096)
        b.write(t.offset, data)
        assert b.read(t.offset, 4096) == data
        assert b.checksum(t.offset, 4096) == bb.core.gpu.checksum_cpu(data)
        st = b.stats()
        assert st.num_shards == 1 and st.used >= 4096
        b.free(t.offset, 4096)
        assert b.stats().num_shards == 0

    def test_abort_releases(self, cls, needs_dir, tmp_path):
        b = make(cls, tmpdir=tmp_path if needs_dir else None,
                 pool_id="b_%s" % cls.name)
        t = b.reserve(1 * MB)
        b.abort(t.token_id)
        assert b.stats().used == 0
        with pytest.raises(Exception, match="RESERVATION_NOT_FOUND"):
            b.commit(t.token_id)

    def test_out_of_space(self, cls, needs_dir, tmp_path):
        b = make(cls, size=1 * MB, tmpdir=tmp_path if needs_dir else None,
                 pool_id="c_%s" % cls.name)
        b.reserve(1 * MB)
        with pytest.raises(Exception, match="NO_SPACE"):
            b.reserve(1)

    def test_reserve_at_keystone_offsets(self, cls, needs_dir, tmp_path):
        b = make(cls, tmpdir=tmp_path if needs_dir else None,
                 pool_id="d_%s" % cls.name)
        t = b.reserve_at(8192, 4096)
        assert t.offset == 8192
        b.commit(t.token_id)
        with pytest.raises(Exception, match="NO_SPACE"):
            b.reserve_at(8192, 4096)  # overlap rejected

    def test_free_size_mismatch(self, cls, needs_dir, tmp_path):
        b = make(cls, tmpdir=tmp_path if needs_dir else None,
                 pool_id="e_%s" % cls.name)
        t = b.reserve(4096)
        b.commit(t.token_id)
        with pytest.raises(Exception, match="SIZE_MISMATCH"):
            b.free(t.offset, 8192)
        with pytest.raises(Exception, match="SHARD_NOT_FOUND"):
            b.free(t.offset + 4096, 4096)

    def test_io_bounds_checked(self, cls, needs_dir, tmp_path):
        b = make(cls, size=1 * MB, tmpdir=tmp_path if needs_dir else None,
                 pool_id="f_%s" % cls.name)
        with pytest.raises(Exception, match="INVALID_OFFSET"):
            b.write(1 * MB - 10, b"x" * 100)
        with pytest.raises(Exception, match="INVALID_OFFSET"):
            b.read(2 * MB, 1)


class TestDiskPersistence:
    def test_bytes_hit_the_file(self, tmp_path):
        b = make(bb.StorageClass.NVME, size=1 * MB, tmpdir=tmp_path,
                 pool_id="persist")
        t = b.reserve(4096)
        b.commit(t.token_id)
        b.write(t.offset, b"A" * 4096)
        files = list(tmp_path.iterdir())
        assert len(files) == 1
        assert files[0].stat().st_size == 1 * MB

    def test_direct_io_length_matrix(self, tmp_path):
        """Round-trip every shape class through the direct-IO pool: 4 KiB
        multiples ride the zero-copy pread/pwrite fast path (large Python
        bytes are page-aligned), odd lengths exercise the bounced tail, and
        >8 MiB ops split across the IO thread pool."""
        b = make(bb.StorageClass.NVME, size=64 * MB, tmpdir=tmp_path,
                 pool_id="matrix")
        import hashlib
        for length in [4096, 1 * MB, 1 * MB + 100, 12345,
                       8 * MB + 4096, 9 * MB + 7]:
            t = b.reserve(length)
            b.commit(t.token_id)
            data = os.urandom(length)
            b.write(t.offset, data)
            back = b.read(t.offset, length)
            assert hashlib.sha256(back).digest() == \
                hashlib.sha256(data).digest(), length
            assert b.checksum(t.offset, length) == \
                bb.core.gpu.checksum_cpu(data), length
            b.free(t.offset, length)

    def test_invalid_dir_fails_loudly(self):
        cfg = bb.PoolConfig()
        cfg.pool_id = "bad"
        cfg.storage_class = bb.StorageClass.NVME
        cfg.size_bytes = 1 * MB
        cfg.mount_path = "/nonexistent/dir"
        with pytest.raises(Exception, match="BACKEND_INIT_FAILED"):
            bb.make_backend(cfg, "testw")

    def test_disk_pool_needs_mount_path(self):
        cfg = bb.PoolConfig()
        cfg.pool_id = "bad"
        cfg.storage_class = bb.StorageClass.NVME
        cfg.size_bytes = 1 * MB
        with pytest.raises(Exception, match="CONFIG_INVALID"):
            bb.make_backend(cfg, "testw")


class TestShmAccess:
    def test_shm_advertised_and_mappable(self):
        b = make(bb.StorageClass.RAM_CPU, pool_id="shmadv")
        a = b.access_info()
        assert a.kind == bb.AccessKind.SHM
        assert a.shm_name.startswith("/bb_")
        # the segment is really there
        assert os.path.exists("/dev/shm" + a.shm_name)

    def test_hbm_requires_gpu(self):
        if bb.core.gpu.available():
            pytest.skip("GPU present — covered by gpu tests")
        cfg = bb.PoolConfig()
        cfg.pool_id = "hbm"
        cfg.storage_class = bb.StorageClass.RAM_GPU
        cfg.size_bytes = 1 * MB
        with pytest.raises(Exception, match="NO_GPU"):
            bb.make_backend(cfg, "testw")  # fails loudly, no CPU fallback


class TestCxlMemBackend:
    def test_dax_file_mapping_and_fallback(self, tmp_path):
        """CXL_MEM tier: maps a DAX device/file when given one, falls back
        to anonymous memory otherwise; full e2e put/get through the tier.
        (The reference's CxlMemoryBackend never compiled — it referenced
        nonexistent error codes)"""
        import os as _os
        from conftest import Cluster
        # file-backed "DAX" mapping (a real /dev/dax maps identically)
        dax = tmp_path / "fake-dax"
        dax.write_bytes(b"\x00" * (8 << 20))
        cl = Cluster(n_workers=1, pool_bytes=8 << 20,
                     storage_class=bb.StorageClass.CXL_MEM,
                     mount_path=str(dax))
        try:
            c = cl.client(verify_checksum_on_get=True)
            data = _os.urandom(1 << 20)
            c.put("cxl-obj", data)
            assert c.get("cxl-obj") == data
            pool = c.memory_pools()[0]
            assert pool.storage_class == bb.StorageClass.CXL_MEM
            # bytes really landed in the mapped file
            assert data[:4096] in dax.read_bytes()
            c.close()
        finally:
            cl.stop()
        # no device at all → anonymous fallback still serves
        cl2 = Cluster(n_workers=1, pool_bytes=8 << 20,
                      storage_class=bb.StorageClass.CXL_MEM)
        try:
            c = cl2.client()
            c.put("anon-cxl", b"fallback works")
            assert c.get("anon-cxl") == b"fallback works"
            c.close()
        finally:
            cl2.stop()
