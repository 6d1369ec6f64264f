// Stand-alone timing of the copying tile walk (digest_device.hip.h) on 1 MiB
// objects: a size sweep 32..512 MiB (the flagship is 512 x 1 MiB) of the walk
// with plain and with nontemporal payload loads, one launch at a time (one
// event pair per launch) and with two streams launching at once, as the two
// benchmark lanes do. Every line's digests are compared with the first line
// of that size, and at 512 MiB the destination bytes with the source. Behind
// profiles/walk_persistent_checks.md. (The sweeps over pipeline depth and
// grid size behind profiles/walk_pipeline_checks.md were run with this file
// as it stood at that change.)
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++20 -Icsrc/include -Icsrc/hip \
//     scripts/walk_bench.hip -o walk_bench && ./walk_bench 50
//
// -DPARENT with the include paths of a checkout from before the lane tables
// (constants hashed by every wave, plain loads) times that walk with the
// same program.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
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
            unsigned long long* out) {
  digest_walk<true, kWalkDepth>(d, p, n, t, out);
}
#else
template <bool kNt>
__global__ void __launch_bounds__(kBlock)
walk_kernel(const CopyDesc* d, const uint64_t* p, uint32_t n, uint64_t t,
            unsigned long long* out) {
  digest_walk<true, kWalkDepth, CopyDesc, kNt>(d, p, n, t, out);
}
#endif

__global__ void fill(uint64_t* p, uint64_t nwords, uint64_t seed) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords;
       i += stride)
    p[i] = blackbird::digest::splitmix64(seed ^ i);
}

using KernelFn = void (*)(const CopyDesc*, const uint64_t*, uint32_t, uint64_t,
                          unsigned long long*);

struct Lane {
  uint8_t *src, *dst;
  CopyDesc* d_descs;
  uint64_t* d_prefix;
  unsigned long long* d_out;
  hipStream_t stream;
};

constexpr uint32_t kN = 512;  // objects allocated; a sweep point takes the first n
constexpr uint64_t kS = 1 << 20;

static void make_lane(Lane& L, uint64_t seed) {
  CK(hipMalloc(&L.src, kN * kS));
  CK(hipMalloc(&L.dst, kN * kS));
  CK(hipMalloc(&L.d_descs, kN * sizeof(CopyDesc)));
  CK(hipMalloc(&L.d_prefix, kN * sizeof(uint64_t)));
  CK(hipMalloc(&L.d_out, kN * sizeof(uint64_t)));
  CK(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
  std::vector<CopyDesc> descs(kN);
  std::vector<uint64_t> prefix(kN);
  for (uint32_t i = 0; i < kN; ++i) {
    descs[i] = {L.src + i * kS, L.dst + i * kS, kS};
    prefix[i] = i * (kS / 1024);
  }
  CK(hipMemcpy(L.d_descs, descs.data(), kN * sizeof(CopyDesc), hipMemcpyHostToDevice));
  CK(hipMemcpy(L.d_prefix, prefix.data(), kN * sizeof(uint64_t), hipMemcpyHostToDevice));
  fill<<<2048, 256>>>(reinterpret_cast<uint64_t*>(L.src), kN * kS / 8, seed);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
}

// the first n objects, launched as enqueue_digest launches them
static void launch(KernelFn fn, uint32_t n, const Lane& L) {
  const uint64_t tiles = n * (kS / 1024);
  CK(hipMemsetAsync(L.d_out, 0, n * sizeof(uint64_t), L.stream));
  hipLaunchKernelGGL(fn, dim3(digest_grid(tiles)), dim3(kBlock), 0, L.stream,
                     L.d_descs, L.d_prefix, n, tiles, L.d_out);
  CK(hipGetLastError());
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? atoi(argv[1]) : 30;
  Lane A, B;
  make_lane(A, 1234);
  make_lane(B, 99);

  struct Var {
    const char* name;
    KernelFn fn;
  };
#ifdef PARENT
  std::vector<Var> vars = {{"parent", walk_parent}};
#else
  std::vector<Var> vars = {{"tables", walk_kernel<false>},
                           {"tables+nt", walk_kernel<true>}};
#endif
  const uint32_t sizes_mib[] = {512, 256, 128, 64, 32};

  std::vector<uint8_t> h_src(kN * kS), h_dst(kN * kS);
  CK(hipMemcpy(h_src.data(), A.src, kN * kS, hipMemcpyDeviceToHost));
  std::vector<uint64_t> h_out(kN);
  std::map<uint32_t, uint64_t> want_fold;  // per size: the first line's digests

  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));

  for (const Var& v : vars) {
    for (uint32_t n : sizes_mib) {
      // correctness: digests equal across all lines of a size, bytes equal
      CK(hipMemsetAsync(A.dst, 0xA5, kN * kS, A.stream));
      launch(v.fn, n, A);
      CK(hipStreamSynchronize(A.stream));
      CK(hipMemcpy(h_out.data(), A.d_out, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
      uint64_t fold = 0;
      for (uint32_t i = 0; i < n; ++i) fold = fold * 0x9E3779B97F4A7C15ull + h_out[i];
      if (!want_fold.count(n)) want_fold[n] = fold;
      bool ok = fold == want_fold[n];
      if (n == kN) {
        CK(hipMemcpy(h_dst.data(), A.dst, kN * kS, hipMemcpyDeviceToHost));
        ok = ok && memcmp(h_src.data(), h_dst.data(), kN * kS) == 0;
      }
      // single-stream timing, one event pair per launch
      for (int i = 0; i < 3; ++i) launch(v.fn, n, A);
      CK(hipStreamSynchronize(A.stream));
      std::vector<float> us;
      for (int i = 0; i < reps; ++i) {
        const uint64_t tiles = n * (kS / 1024);
        CK(hipMemsetAsync(A.d_out, 0, n * sizeof(uint64_t), A.stream));
        CK(hipEventRecord(e0, A.stream));
        hipLaunchKernelGGL(v.fn, dim3(digest_grid(tiles)), dim3(kBlock), 0,
                           A.stream, A.d_descs, A.d_prefix, n, tiles, A.d_out);
        CK(hipEventRecord(e1, A.stream));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        us.push_back(ms * 1e3f);
      }
      std::sort(us.begin(), us.end());
      // two lanes at once, as in the benchmark: 2*reps launches, wall time
      CK(hipDeviceSynchronize());
      CK(hipEventRecord(e0, A.stream));
      CK(hipStreamWaitEvent(B.stream, e0, 0));
      for (int i = 0; i < reps; ++i) {
        launch(v.fn, n, A);
        launch(v.fn, n, B);
      }
      hipEvent_t eb;
      CK(hipEventCreate(&eb));
      CK(hipEventRecord(eb, B.stream));
      CK(hipStreamWaitEvent(A.stream, eb, 0));
      CK(hipEventRecord(e1, A.stream));
      CK(hipEventSynchronize(e1));
      float dual_ms;
      CK(hipEventElapsedTime(&dual_ms, e0, e1));
      CK(hipEventDestroy(eb));
      printf("%-10s %3u MiB  min %6.1f  med %6.1f  max %6.1f us"
             " | dual %6.1f us/launch | digest-fold %016llx %s\n",
             v.name, n, us.front(), us[us.size() / 2], us.back(),
             dual_ms * 1e3f / (2 * reps), (unsigned long long)fold,
             ok ? "ok" : "MISMATCH");
      fflush(stdout);
      if (!ok) return 3;
    }
  }
  return 0;
}
