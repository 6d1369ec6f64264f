// bbhash64 — MFMA-accelerated object digest for the HBM tier (gfx950), and
// the fused copy+digest put path built on it.
// Spec: csrc/include/blackbird/gpu/digest_spec.h (CPU reference is
// bit-identical). The reference had no data integrity at all; the north-star
// requires the checksum as a hand-written CDNA4 kernel visible in rocprof.
//
// Design (CDNA4):
//  - each wave consumes 1024-B tiles with one fully-coalesced dwordx4 load
//    per lane (64 lanes × 16 B = the whole tile),
//  - one v_mfma_i32_32x32x32_i8 per tile computes the 32×32 i32 projection
//    A_t × B in the wave's AGPRs (integer matmul ⇒ bit-exact, order-free),
//  - the fold groups of the spec coincide with the MFMA C-layout, so each
//    lane folds its own 16 accumulator registers in place with
//    register-resident weights — no LDS, no cross-lane work per tile,
//  - per-lane u64 partials are reduced once per wave and atomically added.
//
// Device helpers and the batched tile walk: digest_device.hip.h. Host launch
// sequence of the batched paths: batch_launch.hip.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>

#include "batch_launch.hip.h"
#include "blackbird/gpu/gpu_kernels.h"
#include "digest_device.hip.h"
#include "hip_common.h"

namespace blackbird::gpu {

using namespace blackbird::digest;
using namespace blackbird::gpu::dev;

// ---------------- batched kernels: one launch, many objects ----------------
// Hash only. No prefetch: the walk without the store is VALU-bound.
__global__ void __launch_bounds__(kBlock)
bbhash64_batch_kernel(const CopyDesc* __restrict__ descs,
                      const uint64_t* __restrict__ tile_prefix, uint32_t nobjs,
                      uint64_t total_tiles, unsigned long long* __restrict__ out) {
  digest_walk<false, 0>(descs, tile_prefix, nobjs, total_tiles, out);
}

// Fused put: copy src→dst and hash, reading the data once. The global tiles
// from warm_begin on are stored plainly (digest_walk, kWarm); >= total_tiles:
// none.
__global__ void __launch_bounds__(kBlock)
fused_put_kernel(const CopyDesc* __restrict__ descs,
                 const uint64_t* __restrict__ tile_prefix, uint32_t nobjs,
                 uint64_t total_tiles, unsigned long long* __restrict__ out,
                 uint64_t warm_begin) {
  digest_walk<true, kWalkDepth, CopyDesc, true, kWarmStores>(
      descs, tile_prefix, nobjs, total_tiles, out, nullptr, warm_begin);
}

// The same walk for the get that reads what such a put left on-die: the
// global tiles from warm_begin on are loaded plainly, every store is
// nontemporal.
__global__ void __launch_bounds__(kBlock)
fused_get_kernel(const CopyDesc* __restrict__ descs,
                 const uint64_t* __restrict__ tile_prefix, uint32_t nobjs,
                 uint64_t total_tiles, unsigned long long* __restrict__ out,
                 uint64_t warm_begin) {
  digest_walk<true, kWalkDepth, CopyDesc, true, kWarmLoads>(
      descs, tile_prefix, nobjs, total_tiles, out, nullptr, warm_begin);
}

__global__ void bbhash64_finalize_kernel(const CopyDesc* __restrict__ descs,
                                         uint32_t nobjs,
                                         unsigned long long* __restrict__ out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nobjs) out[i] = finalize(out[i], descs[i].nbytes);
}

namespace {

__global__ void __launch_bounds__(kBlock)
bbhash64_kernel(const uint8_t* __restrict__ data, uint64_t nbytes,
                unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const uint64_t ntiles = (nbytes + kTileBytes - 1) / kTileBytes;
  const uint64_t full_tiles = nbytes / kTileBytes;
  const uint64_t gwave =
      static_cast<uint64_t>(blockIdx.x) * kWavesPerBlock + wave;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kWavesPerBlock;

  const i32x4 b_frag = load_b_frag(lane);
  const WReg wr = load_w_reg(lane);
  const uint32_t lane_off = lane_tile_offset(lane);
  uint64_t h = 0;

  for (uint64_t t = gwave; t < ntiles; t += stride) {
    i32x4 a_frag = (t < full_tiles)
                       ? load_a_frag(data + t * kTileBytes, lane_off)
                       : load_a_frag_guarded(data, t * kTileBytes, nbytes, lane_off);
    h += hash_tile_frag(a_frag, b_frag, wr, t * 64 + lane);
  }

  h = wave_sum_u64(h);
  if (lane == 0 && h != 0) atomicAdd(out, static_cast<unsigned long long>(h));
}

// -------- layout probe (see gpu_kernels.h) --------
__global__ void mfma_i8_probe_kernel(const int8_t* __restrict__ A,
                                     const int8_t* __restrict__ Bm,
                                     int32_t* __restrict__ C) {
  const int lane = threadIdx.x & 63;
  union {
    int8_t b[16];
    i32x4 v;
  } ua, ub;
  const int k0 = (lane >> 5) * 16;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    ua.b[j] = A[(lane & 31) * 32 + k0 + j];
    ub.b[j] = Bm[(k0 + j) * 32 + (lane & 31)];
  }
  i32x16 acc = {};
  acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(ua.v, ub.v, acc, 0, 0, 0);
  const int col = lane & 31;
  const int rbase = 4 * (lane >> 5);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int row = (j & 3) + 8 * (j >> 2) + rbase;
    C[row * 32 + col] = acc[j];
  }
}

// Separate instances per entry point: a digest call never waits for
// another path's launch.
thread_local DescStaging g_hash_stage;
thread_local DescStaging g_put_stage;

// Stage, upload, digest (kCopy: and copy), wait, hand the digests back. The
// descriptors may already sit at the head of stage.pinned.
template <bool kCopy>
Result<void> digest_batch_sync(DescStaging& stage, const CopyDesc* descs,
                               uint32_t n, uint64_t* out_digests,
                               hipStream_t stream, WarmTail warm = {}) {
  const BatchBlock b{n};
  const uint64_t total = fill_block(b, stage.pinned, descs, kTileBytes);
  BB_HIP_TRY(hipMemcpyAsync(stage.device, stage.pinned, b.upload_bytes(),
                            hipMemcpyHostToDevice, stream));
  uint64_t* h_out = b.out(stage.pinned);
  BB_RETURN_IF_ERROR(
      enqueue_digest<kCopy>(stage.device, n, total, h_out, stream, warm));
  BB_HIP_TRY(hipStreamSynchronize(stream));
  std::memcpy(out_digests, h_out, b.out_bytes());
  return {};
}

}  // namespace

bool available() {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

uint64_t digest_grid_waves(uint64_t total_tiles) {
  return static_cast<uint64_t>(digest_grid(total_tiles)) * kWavesPerBlock;
}

int digest_walk_depth() { return kWalkDepth; }

Result<void> checksum_async(const void* dev_ptr, uint64_t nbytes, uint64_t* dev_out,
                            hipStream_t stream) {
  BB_HIP_TRY(hipMemsetAsync(dev_out, 0, sizeof(uint64_t), stream));
  const uint64_t ntiles = tile_count(nbytes);
  if (ntiles > 0) {
    bbhash64_kernel<<<digest_grid(ntiles), kBlock, 0, stream>>>(
        static_cast<const uint8_t*>(dev_ptr), nbytes,
        reinterpret_cast<unsigned long long*>(dev_out));
    BB_HIP_LAUNCHED("bbhash64_kernel");
  }
  return {};
}

Result<uint64_t> checksum_sync(const void* dev_ptr, uint64_t nbytes, int device,
                               hipStream_t stream) {
  BB_HIP_TRY(hipSetDevice(device));
  BB_RETURN_IF_ERROR(g_hash_stage.acquire(sizeof(uint64_t)));
  auto* d_out = static_cast<uint64_t*>(g_hash_stage.device);
  auto* h_out = static_cast<uint64_t*>(g_hash_stage.pinned);
  BB_RETURN_IF_ERROR(checksum_async(dev_ptr, nbytes, d_out, stream));
  BB_HIP_TRY(hipMemcpyAsync(h_out, d_out, sizeof(uint64_t),
                            hipMemcpyDeviceToHost, stream));
  BB_HIP_TRY(hipStreamSynchronize(stream));
  return digest::finalize(*h_out, nbytes);
}

Result<void> checksum_batch(const void* const* dev_ptrs, const uint64_t* sizes,
                            uint32_t n, uint64_t* out_digests, int device,
                            hipStream_t stream) {
  if (n == 0) return {};
  BB_HIP_TRY(hipSetDevice(device));
  const BatchBlock b{n};
  BB_RETURN_IF_ERROR(g_hash_stage.acquire(b.bytes()));
  CopyDesc* h_descs = b.descs(g_hash_stage.pinned);
  for (uint32_t i = 0; i < n; ++i) h_descs[i] = {dev_ptrs[i], nullptr, sizes[i]};
  return digest_batch_sync<false>(g_hash_stage, h_descs, n, out_digests, stream);
}

Result<void> fused_put(const PutDesc* descs, uint32_t n, uint64_t* out_digests,
                       hipStream_t stream, WarmTail warm) {
  if (n == 0) return {};
  BB_RETURN_IF_ERROR(g_put_stage.acquire(BatchBlock{n}.bytes()));
  return digest_batch_sync<true>(g_put_stage, descs, n, out_digests, stream,
                                 warm);
}

// ----------------- hipGraph-replayed session step (FusedPutPlan) -----------
// A batch session re-runs the SAME desc list every step, so the descriptors
// are uploaded once and the step is captured as a graph: one hipGraphLaunch
// replaces memset + 2 kernel launches + D2H issue each step.

struct FusedPutPlan::Impl : GraphStep {};

FusedPutPlan::~FusedPutPlan() { delete impl_; }

Result<void> FusedPutPlan::build(const PutDesc* descs, uint32_t n, int device,
                                 WarmTail warm) {
  if (impl_) return Error{ErrorCode::INVALID_ARGUMENT, "plan already built"};
  if (n == 0) return Error{ErrorCode::INVALID_ARGUMENT, "empty desc list"};
  BB_HIP_TRY(hipSetDevice(device));
  auto impl = std::make_unique<Impl>();
  const BatchBlock b{n};

  auto h_block = std::make_unique<unsigned char[]>(b.upload_bytes());
  const uint64_t total = fill_block(b, h_block.get(), descs, kTileBytes);
  if (total == 0) return Error{ErrorCode::INVALID_ARGUMENT, "zero-byte batch"};

  BB_RETURN_IF_ERROR(impl->prepare(h_block.get(), b.upload_bytes(), b.bytes(),
                                   b.out_bytes()));
  BB_RETURN_IF_ERROR(impl->capture([&](hipStream_t s) {
    return enqueue_digest<true>(impl->dev, n, total, impl->h_out, s, warm);
  }));
  n_ = n;
  impl_ = impl.release();
  return {};
}

Result<void> FusedPutPlan::run(uint64_t* out_digests) {
  if (!impl_) return Error{ErrorCode::INVALID_ARGUMENT, "plan not built"};
  BB_RETURN_IF_ERROR(impl_->replay());
  std::memcpy(out_digests, impl_->h_out, impl_->out_bytes);
  return {};
}

Result<void> mfma_i8_probe(const int8_t* host_a, const int8_t* host_b,
                           int32_t* host_c, int device) {
  BB_HIP_TRY(hipSetDevice(device));
  int8_t *dA = nullptr, *dB = nullptr;
  int32_t* dC = nullptr;
  BB_HIP_TRY(hipMalloc(&dA, 1024));
  BB_HIP_TRY(hipMalloc(&dB, 1024));
  BB_HIP_TRY(hipMalloc(&dC, 1024 * sizeof(int32_t)));
  {
    // copies and launch ordered on ONE pool stream
    XferStream xs;
    BB_RETURN_IF_ERROR(acquire_xfer_stream(xs));
    BB_HIP_TRY(hipMemcpyAsync(dA, host_a, 1024, hipMemcpyHostToDevice, xs.stream));
    BB_HIP_TRY(hipMemcpyAsync(dB, host_b, 1024, hipMemcpyHostToDevice, xs.stream));
    mfma_i8_probe_kernel<<<1, 64, 0, xs.stream>>>(dA, dB, dC);
    BB_HIP_LAUNCHED("mfma_i8_probe_kernel");
    BB_HIP_TRY(hipMemcpyAsync(host_c, dC, 1024 * sizeof(int32_t),
                              hipMemcpyDeviceToHost, xs.stream));
    BB_HIP_TRY(hipStreamSynchronize(xs.stream));
  }
  BB_HIP_TRY(hipFree(dA));
  BB_HIP_TRY(hipFree(dB));
  BB_HIP_TRY(hipFree(dC));
  return {};
}

}  // namespace blackbird::gpu
