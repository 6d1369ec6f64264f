import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blackbird_amd as bb
g = bb.core.gpu
MB = 1<<20
N, S = 512, 1*MB
mode = sys.argv[1] if len(sys.argv) > 1 else "both"
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 12
pool = g.malloc(3*N*S)
src = g.malloc(N*S)
dst = g.malloc(N*S)
g.fill_pattern(src, N*S, seed=7)
print("alloc ok mode=%s" % mode, flush=True)
for it in range(iters):
    if mode in ("both", "copy"):
        g.batched_copy([(src + i*S, pool + (i*3)*S, S) for i in range(N)])
    if mode in ("both", "sum"):
        g.checksum_device_batch([(src + i*S, S) for i in range(N)])
    if mode in ("both", "copy"):
        g.batched_copy([(pool + (i*3)*S, dst + i*S, S) for i in range(N)])
    g.sync()
    print("iter", it, "ok", flush=True)
if mode in ("both", "copy"):
    print("mismatches:", g.verify_pattern(dst, N*S, seed=7))
print("STRESS OK")

if mode == "hashbw":
    import time as _t
    # isolate checksum kernel bandwidth: one big buffer
    big = g.malloc(2048*MB)
    g.fill_pattern(big, 2048*MB, seed=3)
    for sz_mb in (256, 1024, 2048):
        n = sz_mb*MB
        g.checksum_device(big, n)  # warm
        t0=_t.perf_counter(); reps=5
        for _ in range(reps): g.checksum_device(big, n)
        dt=(_t.perf_counter()-t0)/reps
        print(f"bbhash64 single {sz_mb}MB: {n/dt/1e9:.0f} GB/s")
        objs=[(big+i*MB, MB) for i in range(sz_mb)]
        g.checksum_device_batch(objs)
        t0=_t.perf_counter()
        for _ in range(reps): g.checksum_device_batch(objs)
        dt=(_t.perf_counter()-t0)/reps
        print(f"bbhash64 batch {sz_mb}x1MB: {n/dt/1e9:.0f} GB/s")
    # copy kernel bandwidth
    half = 1024*MB
    descs=[(big+i*MB, big+half+i*MB, MB) for i in range(1024)]
    g.batched_copy(descs)
    t0=_t.perf_counter()
    for _ in range(3): g.batched_copy(descs)
    dt=(_t.perf_counter()-t0)/3
    print(f"batched_copy 1024x1MB: {half/dt/1e9:.0f} GB/s payload ({2*half/dt/1e9:.0f} GB/s HBM)")
    # fused copy+digest kernel, same descriptors
    g.fused_put(descs)
    t0=_t.perf_counter()
    for _ in range(3): g.fused_put(descs)
    dt=(_t.perf_counter()-t0)/3
    print(f"fused_put 1024x1MB: {half/dt/1e9:.0f} GB/s payload ({2*half/dt/1e9:.0f} GB/s HBM)")
