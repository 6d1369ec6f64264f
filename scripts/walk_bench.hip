// Stand-alone timing of the copying tile walk (digest_device.hip.h) on the
// flagship shape, 512 x 1 MiB: every pipeline depth 0..4 at several grid
// sizes, one launch at a time (one event pair per launch) and with two
// streams launching at once, as the two benchmark lanes do. Each variant's
// digests and destination bytes are checked against the source. Behind
// sections 2 of profiles/walk_pipeline_checks.md.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++20 -Icsrc/include -Icsrc/hip \
//     scripts/walk_bench.hip -o walk_bench && ./walk_bench 50
//
// -DPARENT with the include paths of a checkout from before the pipeline
// (digest_walk<kCopy, kPrefetch>) times that walk with the same program.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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
template <bool P>
__global__ void __launch_bounds__(kBlock)
walk_kernel(const CopyDesc* d, const uint64_t* p, uint32_t n, uint64_t t,
            unsigned long long* out) {
  digest_walk<true, P>(d, p, n, t, out);
}
#else
template <int K>
__global__ void __launch_bounds__(kBlock)
walk_kernel(const CopyDesc* d, const uint64_t* p, uint32_t n, uint64_t t,
            unsigned long long* out) {
  digest_walk<true, K>(d, p, n, t, out);
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

constexpr uint32_t kN = 512;
constexpr uint64_t kS = 1 << 20;
constexpr uint64_t kTiles = kN * kS / 1024;

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

static void launch(KernelFn fn, int grid, const Lane& L) {
  CK(hipMemsetAsync(L.d_out, 0, kN * sizeof(uint64_t), L.stream));
  hipLaunchKernelGGL(fn, dim3(grid), dim3(kBlock), 0, L.stream, L.d_descs,
                     L.d_prefix, kN, kTiles, L.d_out);
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
  std::vector<Var> vars = {{"parent_prefetch", walk_kernel<true>},
                           {"parent_noprefetch", walk_kernel<false>}};
#else
  std::vector<Var> vars = {{"K0", walk_kernel<0>}, {"K1", walk_kernel<1>},
                           {"K2", walk_kernel<2>}, {"K3", walk_kernel<3>},
                           {"K4", walk_kernel<4>}};
#endif
  const int grids[] = {4096, 2560, 2048, 1280, 1024, 512};

  std::vector<uint8_t> h_src(kN * kS), h_dst(kN * kS);
  CK(hipMemcpy(h_src.data(), A.src, kN * kS, hipMemcpyDeviceToHost));
  std::vector<uint64_t> h_out(kN), ref_out;

  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));

  for (const Var& v : vars) {
    for (int g : grids) {
      // correctness: digests equal across all variants and grids, bytes equal
      CK(hipMemsetAsync(A.dst, 0xA5, kN * kS, A.stream));
      launch(v.fn, g, A);
      CK(hipStreamSynchronize(A.stream));
      CK(hipMemcpy(h_out.data(), A.d_out, kN * sizeof(uint64_t), hipMemcpyDeviceToHost));
      uint64_t fold = 0;
      for (uint64_t x : h_out) fold = fold * 0x9E3779B97F4A7C15ull + x;
      bool bytes_ok = true;
      if (g == 4096 || g == 1280) {
        CK(hipMemcpy(h_dst.data(), A.dst, kN * kS, hipMemcpyDeviceToHost));
        bytes_ok = memcmp(h_src.data(), h_dst.data(), kN * kS) == 0;
      }
      // single-stream timing, one event pair per launch
      for (int i = 0; i < 3; ++i) launch(v.fn, g, A);
      CK(hipStreamSynchronize(A.stream));
      std::vector<float> us;
      for (int i = 0; i < reps; ++i) {
        CK(hipMemsetAsync(A.d_out, 0, kN * sizeof(uint64_t), A.stream));
        CK(hipEventRecord(e0, A.stream));
        hipLaunchKernelGGL(v.fn, dim3(g), dim3(kBlock), 0, A.stream, A.d_descs,
                           A.d_prefix, kN, kTiles, A.d_out);
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
        launch(v.fn, g, A);
        launch(v.fn, g, B);
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
      printf("%-18s grid %4d  min %7.1f  med %7.1f  max %7.1f us | dual %7.1f us/launch | "
             "digest-fold %016llx bytes %s\n",
             v.name, g, us.front(), us[us.size() / 2], us.back(),
             dual_ms * 1e3f / (2 * reps), (unsigned long long)fold,
             bytes_ok ? "ok" : "MISMATCH");
      fflush(stdout);
      if (!bytes_ok) return 3;
    }
  }
  return 0;
}
