// Stand-alone measurement behind profiles/warm_tail_checks.md: does a put
// that stores the tail of its batch plainly leave that tail in the Infinity
// Cache for the get that follows?
//
// probe: 128 MiB written with plain or nontemporal 16-B stores, then 1 GiB
//        streamed through a nontemporal copy, a plain copy or nothing, then
//        the 128 MiB read with nontemporal or plain loads; the read is timed.
// pair:  the flagship shape, 512 x 1 MiB, through the copying tile walk
//        (digest_device.hip.h). Each of two streams alternates put (src ->
//        pool) and get (pool -> dst) over its own buffers, as the benchmark's
//        two lanes do. Swept: the warm tail W of each put launch, and whether
//        the get loads that tail nontemporally or plainly. Per line: put, get
//        and put+get event-timed on one stream, wall time per put+get of a
//        burst on one stream, and with both streams busy the interval
//        between a stream's pairs, halved (two pairs finish per interval).
//        Every line checks the 512 digests of both launches against the
//        first line's and the destination bytes against the source.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++20 -Icsrc/include -Icsrc/hip \
//     scripts/warm_tail_bench.hip -o warm_tail_bench
//   ./warm_tail_bench probe 7 && ./warm_tail_bench pair 50
//
// -DPARENT with the include paths of a checkout from before the warm tail
// times that walk (one line, W = 0) with the same program; run the two
// binaries alternating.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "batch_launch.hip.h"
#include "digest_device.hip.h"

using namespace blackbird::gpu;
using namespace blackbird::gpu::dev;

#define CK(x)                                                            \
  do {                                                                   \
    hipError_t e_ = (x);                                                 \
    if (e_ != hipSuccess) {                                              \
      fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_),  \
              __FILE__, __LINE__);                                       \
      exit(2);                                                           \
    }                                                                    \
  } while (0)

#ifdef PARENT
__global__ void __launch_bounds__(kBlock)
walk_parent(const CopyDesc* d, const uint64_t* p, uint32_t n, uint64_t t,
            unsigned long long* out, uint64_t) {
  digest_walk<true, kWalkDepth>(d, p, n, t, out);
}
#else
template <int kWarm>
__global__ void __launch_bounds__(kBlock)
walk_kernel(const CopyDesc* d, const uint64_t* p, uint32_t n, uint64_t t,
            unsigned long long* out, uint64_t warm_begin) {
  digest_walk<true, kWalkDepth, CopyDesc, true, kWarm>(d, p, n, t, out, nullptr,
                                                       warm_begin);
}
#endif

using KernelFn = void (*)(const CopyDesc*, const uint64_t*, uint32_t, uint64_t,
                          unsigned long long*, uint64_t);

__global__ void fill(uint64_t* p, uint64_t nwords, uint64_t seed) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords;
       i += stride)
    p[i] = blackbird::digest::splitmix64(seed ^ i);
}

// number of 8-byte words in which a and b differ
__global__ void count_diff(const uint64_t* a, const uint64_t* b, uint64_t nwords,
                           unsigned long long* ndiff) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long c = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords;
       i += stride)
    c += a[i] != b[i];
  if (c) atomicAdd(ndiff, c);
}

// ---------------------------------------------------------------- probe ----
using g_i32x4 = global_ptr<i32x4>;

template <bool kNt>
__global__ void probe_write(i32x4* p, uint64_t n16) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16;
       i += stride) {
    const i32x4 v = {(int)i, 1, 2, 3};
    if constexpr (kNt) __builtin_nontemporal_store(v, (g_i32x4)p + i);
    else ((g_i32x4)p)[i] = v;
  }
}

template <bool kNt>
__global__ void probe_copy(i32x4* dst, const i32x4* src, uint64_t n16) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16;
       i += stride) {
    if constexpr (kNt)
      __builtin_nontemporal_store(
          __builtin_nontemporal_load((global_ptr<const i32x4>)src + i),
          (g_i32x4)dst + i);
    else ((g_i32x4)dst)[i] = ((global_ptr<const i32x4>)src)[i];
  }
}

template <bool kNt>
__global__ void probe_read(const i32x4* p, uint64_t n16, int* sink) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  i32x4 acc = {};
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16;
       i += stride) {
    if constexpr (kNt) acc ^= __builtin_nontemporal_load((global_ptr<const i32x4>)p + i);
    else acc ^= ((global_ptr<const i32x4>)p)[i];
  }
  sink[blockIdx.x * blockDim.x + threadIdx.x] = acc[0] ^ acc[1] ^ acc[2] ^ acc[3];
}

static int run_probe(int reps) {
  constexpr uint64_t kHot = 128ull << 20, kStream = 1ull << 30;
  constexpr int kGrid = 2048, kThreads = 256;
  i32x4 *hot, *s_src, *s_dst;
  int* sink;
  CK(hipMalloc(&hot, kHot));
  CK(hipMalloc(&s_src, kStream));
  CK(hipMalloc(&s_dst, kStream));
  CK(hipMalloc(&sink, kGrid * kThreads * sizeof(int)));
  CK(hipMemset(s_src, 1, kStream));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const char* stream_name[] = {"none", "1 GiB nt copy", "1 GiB plain copy"};
  printf("probe: 128 MiB read, us min / med of %d (128 MiB at 4 TB/s is 33.6 us)\n",
         reps);
  for (int wnt = 0; wnt < 2; ++wnt)
    for (int sm = 0; sm < 3; ++sm)
      for (int rnt = 1; rnt >= 0; --rnt) {
        std::vector<float> us;
        for (int r = 0; r < reps; ++r) {
          if (wnt) probe_write<true><<<kGrid, kThreads>>>(hot, kHot / 16);
          else probe_write<false><<<kGrid, kThreads>>>(hot, kHot / 16);
          if (sm == 1) probe_copy<true><<<kGrid, kThreads>>>(s_dst, s_src, kStream / 16);
          if (sm == 2) probe_copy<false><<<kGrid, kThreads>>>(s_dst, s_src, kStream / 16);
          CK(hipEventRecord(e0, nullptr));
          if (rnt) probe_read<true><<<kGrid, kThreads>>>(hot, kHot / 16, sink);
          else probe_read<false><<<kGrid, kThreads>>>(hot, kHot / 16, sink);
          CK(hipEventRecord(e1, nullptr));
          CK(hipGetLastError());
          CK(hipEventSynchronize(e1));
          float ms;
          CK(hipEventElapsedTime(&ms, e0, e1));
          us.push_back(ms * 1e3f);
        }
        std::sort(us.begin(), us.end());
        printf("probe write %-5s | stream %-16s | read %-5s : %6.1f / %6.1f us\n",
               wnt ? "nt" : "plain", stream_name[sm], rnt ? "nt" : "plain",
               us.front(), us[us.size() / 2]);
        fflush(stdout);
      }
  CK(hipFree(hot));
  CK(hipFree(s_src));
  CK(hipFree(s_dst));
  CK(hipFree(sink));
  return 0;
}

// ----------------------------------------------------------------- pair ----
constexpr uint32_t kN = 512;
constexpr uint64_t kS = 1 << 20;
constexpr uint64_t kTiles = kN * (kS / 1024);

struct Lane {
  uint8_t *src, *pool, *dst;
  CopyDesc *d_put, *d_get;
  uint64_t* d_prefix;
  unsigned long long *d_out_put, *d_out_get;
  hipStream_t stream;
};

static void make_lane(Lane& L, uint64_t seed) {
  CK(hipMalloc(&L.src, kN * kS));
  CK(hipMalloc(&L.pool, kN * kS));
  CK(hipMalloc(&L.dst, kN * kS));
  CK(hipMalloc(&L.d_put, kN * sizeof(CopyDesc)));
  CK(hipMalloc(&L.d_get, kN * sizeof(CopyDesc)));
  CK(hipMalloc(&L.d_prefix, kN * sizeof(uint64_t)));
  CK(hipMalloc(&L.d_out_put, kN * sizeof(uint64_t)));
  CK(hipMalloc(&L.d_out_get, kN * sizeof(uint64_t)));
  CK(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
  std::vector<CopyDesc> put(kN), get(kN);
  std::vector<uint64_t> prefix(kN);
  for (uint32_t i = 0; i < kN; ++i) {
    put[i] = {L.src + i * kS, L.pool + i * kS, kS};
    get[i] = {L.pool + i * kS, L.dst + i * kS, kS};
    prefix[i] = i * (kS / 1024);
  }
  CK(hipMemcpy(L.d_put, put.data(), kN * sizeof(CopyDesc), hipMemcpyHostToDevice));
  CK(hipMemcpy(L.d_get, get.data(), kN * sizeof(CopyDesc), hipMemcpyHostToDevice));
  CK(hipMemcpy(L.d_prefix, prefix.data(), kN * sizeof(uint64_t), hipMemcpyHostToDevice));
  fill<<<2048, 256>>>(reinterpret_cast<uint64_t*>(L.src), kN * kS / 8, seed);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
}

struct Var {
  const char* name;
  KernelFn put, get;
  uint64_t warm_mib;  // of each put launch; the get loads the same tail
};

static uint64_t warm_begin_of(const Var& v) {
  const uint64_t warm_tiles = std::min(kTiles, v.warm_mib * 1024);
  return kTiles - warm_tiles;
}

// launched as enqueue_digest launches them
static void launch(KernelFn fn, const CopyDesc* descs, unsigned long long* out,
                   uint64_t warm_begin, const Lane& L) {
  CK(hipMemsetAsync(out, 0, kN * sizeof(uint64_t), L.stream));
  hipLaunchKernelGGL(fn, dim3(digest_grid(kTiles)), dim3(kBlock), 0, L.stream,
                     descs, L.d_prefix, kN, kTiles, out, warm_begin);
  CK(hipGetLastError());
}
static void put(const Var& v, const Lane& L) {
  launch(v.put, L.d_put, L.d_out_put, warm_begin_of(v), L);
}
static void get(const Var& v, const Lane& L) {
  launch(v.get, L.d_get, L.d_out_get, warm_begin_of(v), L);
}

static uint64_t fold_digests(const unsigned long long* d_out) {
  std::vector<uint64_t> h(kN);
  CK(hipMemcpy(h.data(), d_out, kN * sizeof(uint64_t), hipMemcpyDeviceToHost));
  uint64_t fold = 0;
  for (uint32_t i = 0; i < kN; ++i) fold = fold * 0x9E3779B97F4A7C15ull + h[i];
  return fold;
}

struct Stat {
  float min, med, max;
};
static Stat stat(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return {v.front(), v[v.size() / 2], v.back()};
}

static int run_pair(int reps) {
  Lane A, B;
  make_lane(A, 1234);
  make_lane(B, 99);
#ifdef PARENT
  std::vector<Var> vars = {{"parent W=0 nt", walk_parent, walk_parent, 0}};
#else
  // The put is the kernel with the warm-store branch at every W, W = 0
  // included. "nt": the get is that same kernel with no warm tail (all loads
  // nontemporal); "plain": the get loads the put's tail plainly.
  std::vector<Var> vars;
  static char names[12][32];
  const uint64_t ws[] = {0, 64, 128, 192, 256, 512};
  for (int i = 0; i < 6; ++i)
    for (int plain = 0; plain < 2; ++plain) {
      char* nm = names[2 * i + plain];
      snprintf(nm, 32, "W=%-3llu get %s", (unsigned long long)ws[i],
               plain ? "plain" : "nt");
      vars.push_back({nm, walk_kernel<kWarmStores>,
                      plain ? walk_kernel<kWarmLoads> : walk_kernel<kWarmNone>,
                      ws[i]});
    }
#endif
  constexpr int kEdge = 3;  // pairs dropped at either end of the dual burst
  std::vector<hipEvent_t> ev(3 * reps + 2), evb(reps + 2 * kEdge + 1);
  for (auto& e : ev) CK(hipEventCreate(&e));
  for (auto& e : evb) CK(hipEventCreate(&e));
  unsigned long long* d_ndiff;
  CK(hipMalloc(&d_ndiff, sizeof(*d_ndiff)));
  uint64_t want_fold = 0;
  bool have_fold = false;

  printf("%-16s | one stream: put, get, put+get us med (min-max) | burst us/pair |"
         " two streams: us/pair med (min-max), burst | digests\n", "variant");
  for (const Var& v : vars) {
    // correctness
    CK(hipMemsetAsync(A.dst, 0xA5, kN * kS, A.stream));
    CK(hipMemsetAsync(A.pool, 0x5A, kN * kS, A.stream));
    CK(hipMemsetAsync(d_ndiff, 0, sizeof(*d_ndiff), A.stream));
    put(v, A);
    get(v, A);
    count_diff<<<2048, 256, 0, A.stream>>>(reinterpret_cast<const uint64_t*>(A.src),
                                           reinterpret_cast<const uint64_t*>(A.dst),
                                           kN * kS / 8, d_ndiff);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(A.stream));
    unsigned long long ndiff = 0;
    CK(hipMemcpy(&ndiff, d_ndiff, sizeof(ndiff), hipMemcpyDeviceToHost));
    const uint64_t fp = fold_digests(A.d_out_put), fg = fold_digests(A.d_out_get);
    if (!have_fold) want_fold = fp, have_fold = true;
    const bool ok = ndiff == 0 && fp == want_fold && fg == want_fold;

    // one stream, events around each launch
    for (int i = 0; i < 3; ++i) put(v, A), get(v, A);
    CK(hipStreamSynchronize(A.stream));
    for (int i = 0; i < reps; ++i) {
      CK(hipMemsetAsync(A.d_out_put, 0, kN * sizeof(uint64_t), A.stream));
      CK(hipMemsetAsync(A.d_out_get, 0, kN * sizeof(uint64_t), A.stream));
      CK(hipEventRecord(ev[3 * i], A.stream));
      hipLaunchKernelGGL(v.put, dim3(digest_grid(kTiles)), dim3(kBlock), 0, A.stream,
                         A.d_put, A.d_prefix, kN, kTiles, A.d_out_put, warm_begin_of(v));
      CK(hipEventRecord(ev[3 * i + 1], A.stream));
      hipLaunchKernelGGL(v.get, dim3(digest_grid(kTiles)), dim3(kBlock), 0, A.stream,
                         A.d_get, A.d_prefix, kN, kTiles, A.d_out_get, warm_begin_of(v));
      CK(hipEventRecord(ev[3 * i + 2], A.stream));
      CK(hipGetLastError());
    }
    CK(hipStreamSynchronize(A.stream));
    std::vector<float> t_put, t_get, t_pair;
    for (int i = 0; i < reps; ++i) {
      float a, b;
      CK(hipEventElapsedTime(&a, ev[3 * i], ev[3 * i + 1]));
      CK(hipEventElapsedTime(&b, ev[3 * i + 1], ev[3 * i + 2]));
      t_put.push_back(a * 1e3f);
      t_get.push_back(b * 1e3f);
      t_pair.push_back((a + b) * 1e3f);
    }
    // one stream, a burst: wall time per pair
    CK(hipEventRecord(ev[0], A.stream));
    for (int i = 0; i < reps; ++i) put(v, A), get(v, A);
    CK(hipEventRecord(ev[1], A.stream));
    CK(hipEventSynchronize(ev[1]));
    float solo_ms;
    CK(hipEventElapsedTime(&solo_ms, ev[0], ev[1]));

    // two streams, a burst on each; events between A's pairs
    const int nb = reps + 2 * kEdge;
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(ev[0], A.stream));
    CK(hipStreamWaitEvent(B.stream, ev[0], 0));
    for (int i = 0; i < nb; ++i) {
      CK(hipEventRecord(evb[i], A.stream));
      put(v, A);
      put(v, B);
      get(v, A);
      get(v, B);
    }
    CK(hipEventRecord(evb[nb], A.stream));
    CK(hipEventRecord(ev[2], B.stream));
    CK(hipStreamWaitEvent(A.stream, ev[2], 0));
    CK(hipEventRecord(ev[1], A.stream));
    CK(hipEventSynchronize(ev[1]));
    float dual_ms;
    CK(hipEventElapsedTime(&dual_ms, ev[0], ev[1]));
    std::vector<float> t_dual;
    for (int i = kEdge; i < nb - kEdge; ++i) {
      float a;
      CK(hipEventElapsedTime(&a, evb[i], evb[i + 1]));
      t_dual.push_back(a * 1e3f / 2);
    }
    const Stat sp = stat(t_put), sg = stat(t_get), spp = stat(t_pair), sd = stat(t_dual);
    printf("%-16s | %6.1f (%6.1f-%6.1f) %6.1f (%6.1f-%6.1f) %6.1f (%6.1f-%6.1f) | %6.1f |"
           " %6.1f (%6.1f-%6.1f) %6.1f | %016llx %s\n",
           v.name, sp.med, sp.min, sp.max, sg.med, sg.min, sg.max, spp.med, spp.min,
           spp.max, solo_ms * 1e3f / reps, sd.med, sd.min, sd.max,
           dual_ms * 1e3f / (2 * nb), (unsigned long long)fp, ok ? "ok" : "MISMATCH");
    fflush(stdout);
    if (!ok) return 3;
  }
  return 0;
}

int main(int argc, char** argv) {
  const bool probe = argc > 1 && strcmp(argv[1], "probe") == 0;
  const int reps = argc > 2 ? atoi(argv[2]) : (probe ? 7 : 50);
  if (reps < 1) return 1;
#ifdef PARENT
  if (probe) return 0;
#endif
  return probe ? run_probe(reps) : run_pair(reps);
}
