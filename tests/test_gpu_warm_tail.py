"""The warm tail of the fused copy+digest launches (digest_device.hip.h,
kWarm): the waves whose range begins in the last warm_bytes of a batch store
their full tiles plainly (a put, fused_put_kernel) or load them plainly (a
get, warm_loads=True, fused_get_kernel); all other accesses are nontemporal.
It is a residency hint, so what is checked is that nothing else depends on
it: digests bit-exact against the CPU reference and equal across budgets,
destination bytes exact, pre-filled gaps between the destinations untouched.

The batches are those of test_gpu_walk_pipeline.py, with their CPU digests
computed once for both files. In the 30-object edge batch a wave owns at most
two tiles, so the budgets put the boundary between waves at every kind of
position (none, one tile, mid-batch, everything, past the batch). The batch
above the grid cap gives every wave 18 tiles, so cold and warm waves alike
run prologue, steady loop, drain and the one-by-one tiles; its boundary lies
inside the second object at a tile that is no multiple of the per-wave range,
and rounds to the wave.
"""
import os

import numpy as np
import pytest

import blackbird_amd as bb

from conftest import Cluster
from test_gpu_walk_pipeline import PAD, TILE, _case, _check, _tiles_per_wave

pytestmark = pytest.mark.gpu

gpu = bb.core.gpu
KB, MB = 1 << 10, 1 << 20


def _put(case, **kw):
    """One fused_put of the case into a pre-filled destination: digests, and
    the destination allocation's bytes."""
    src, dst = gpu.malloc(case.span), gpu.malloc(case.span)
    try:
        gpu.upload(src, case.src_image)
        gpu.upload(dst, bytes([PAD]) * case.span)
        descs = [(src + o, dst + o, s) for o, s in zip(case.offs, case.sizes)]
        return gpu.fused_put(descs, **kw), gpu.download(dst, case.span)
    finally:
        gpu.free(src)
        gpu.free(dst)


def _edge_budgets(case):
    total = sum(case.sizes)
    return [0, 1024, total // 2, total, total + 64 * KB]


@pytest.mark.parametrize("loads", [False, True])
@pytest.mark.parametrize("which", range(5))
def test_edge_batch(which, loads):
    case = _case("pipeline_edges")
    warm = _edge_budgets(case)[which]
    digests, image = _put(case, warm_bytes=warm, warm_loads=loads)
    _check(digests, case.want, (warm, loads))
    assert image == case.dst_image, (warm, loads)


def test_edge_batch_default_is_cold():
    """No keyword: the launch of before, and the same digests as any budget."""
    case = _case("pipeline_edges")
    digests, image = _put(case)
    _check(digests, case.want, "default")
    assert image == case.dst_image


def _long_boundary(case):
    """A warm tail of the long batch that begins mid-object, off the per-wave
    range: (warm_bytes, first warm tile)."""
    per = _tiles_per_wave()
    total = case.tiles()
    assert total == gpu.digest_grid_waves(total) * per
    begin = total // 2 + 7
    first = -(-case.sizes[0] // TILE)
    second = -(-case.sizes[1] // TILE)
    assert first < begin < first + second - 1, "boundary not inside object 1"
    assert begin % per, "boundary on a range edge"
    return (total - begin) * TILE, begin


@pytest.mark.parametrize("loads", [False, True])
def test_long_batch_boundary_mid_object(loads):
    case = _case("long_ranges")
    budget, begin = _long_boundary(case)
    digests, image = _put(case, warm_bytes=budget, warm_loads=loads)
    _check(digests, case.want, (begin, loads))
    assert image == case.dst_image, (begin, loads)


@pytest.mark.parametrize("loads", [False, True])
def test_plan_with_warm_tail_follows_the_source(loads):
    """FusedPutPlan captured with a warm tail of half the batch, 8 x 64 KiB:
    two replays, the source rewritten between them."""
    n, size = 8, 64 * KB
    rng = np.random.default_rng(77)
    blobs = [[rng.bytes(size) for _ in range(n)] for _ in range(2)]
    src, dst = gpu.malloc(n * size), gpu.malloc(n * size)
    try:
        descs = [(src + i * size, dst + i * size, size) for i in range(n)]
        images = []

        def before_step(k):
            if k:
                images.append(gpu.download(dst, n * size))
            gpu.upload(src, b"".join(blobs[k]))

        steps = gpu.fused_put_plan(descs, 2, warm_bytes=n * size // 2,
                                   warm_loads=loads, before_step=before_step)
        images.append(gpu.download(dst, n * size))
        for k in range(2):
            _check(steps[k], [gpu.checksum_cpu(b) for b in blobs[k]], k)
            assert images[k] == b"".join(blobs[k]), k
        assert steps[0] != steps[1]
    finally:
        gpu.free(src)
        gpu.free(dst)


def test_client_budget_on_session_steps():
    """GpuClient with a budget set, one RAM_GPU worker, 8 x 64 KiB: three
    put/get session steps, the source changed each step."""
    n, size = 8, 64 * KB
    cl = Cluster(n_workers=1, pool_bytes=64 * MB,
                 storage_class=bb.StorageClass.RAM_GPU)
    src = dst = None
    try:
        c = cl.client()
        gcl = bb.GpuClient(c, 0)
        gcl.init()
        gcl.set_placement_cache(True)
        gcl.set_warm_tail_bytes(3 * size + 1024)
        assert gcl.warm_tail_bytes == 3 * size + 1024
        src, dst = gpu.malloc(n * size), gpu.malloc(n * size)
        cfg = bb.PlacementConfig()
        cfg.replace = True
        cfg.checksum = True
        keys = ["warm%02d" % i for i in range(n)]
        pb = bb.make_put_batch([(k, src + i * size, size)
                                for i, k in enumerate(keys)])
        gb = bb.make_get_batch([(k, dst + i * size, size)
                                for i, k in enumerate(keys)])
        graph_before = gcl.session_graph_steps
        for step in range(3):
            blobs = [os.urandom(size) for _ in range(n)]
            gpu.upload(src, b"".join(blobs))
            assert gcl.batch_put_prepared(pb, cfg), step
            assert gcl.batch_get_prepared_statuses(gb, True) == [0] * n, step
            assert gpu.download(dst, n * size) == b"".join(blobs), step
        ks = cl.keystone.service()
        for k, b in zip(keys, blobs):
            assert ks.get_workers(k).checksum == gpu.checksum_cpu(b), k
        assert gcl.session_put_steps >= 2, gcl.session_put_steps
        if not os.environ.get("BB_NO_HIPGRAPH"):
            assert gcl.session_graph_steps > graph_before
        c.close()
    finally:
        if src:
            gpu.free(src)
            gpu.free(dst)
        cl.stop()
