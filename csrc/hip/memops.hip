// Batched scatter/gather copy + test-pattern kernels for the HBM tier
// (gfx950). One launch moves a whole batch of objects between slab locations
// and staging/ring buffers — the fused multi-object path behind
// batch_put/batch_get (reference analogue: the per-shard ucp_put_nbx loop in
// blackbird_client.cpp:252-267, replaced here by one kernel over all shards).
//
// CDNA4 notes: 16 B/lane dwordx4 vector moves, grid-stride over 4 KiB chunks
// so a batch of any shape fills 256 CUs; descriptors are binary-searched per
// chunk (L2-resident, lane-uniform per wave).
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>

#include "batch_launch.hip.h"
#include "blackbird/gpu/digest_spec.h"
#include "blackbird/gpu/gpu_kernels.h"
#include "digest_device.hip.h"
#include "hip_common.h"

namespace blackbird::gpu {

namespace {

using dev::kBlock;
constexpr uint64_t kChunk = 4096;  // copy work quantum

using ulong1 = unsigned long long;
using v16 = __attribute__((ext_vector_type(4))) unsigned int;

__global__ void __launch_bounds__(kBlock)
batched_copy_kernel(const CopyDesc* __restrict__ segs,
                    const uint64_t* __restrict__ chunk_prefix, uint32_t nsegs,
                    uint64_t total_chunks) {
  const uint64_t gid0 = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const uint64_t wave_id = gid0 >> 6;          // one chunk per wave
  const int lane = threadIdx.x & 63;
  const uint64_t wave_stride =
      (static_cast<uint64_t>(gridDim.x) * kBlock) >> 6;

  for (uint64_t c = wave_id; c < total_chunks; c += wave_stride) {
    const uint32_t si = dev::find_seg(chunk_prefix, nsegs, c);
    const CopyDesc s = segs[si];
    const uint64_t off = (c - chunk_prefix[si]) * kChunk;
    const uint64_t len = min(kChunk, s.nbytes - off);
    // global address space (digest_device.hip.h): global_load/global_store,
    // not flat accesses
    const dev::global_ptr<const uint8_t> src =
        dev::as_global(static_cast<const uint8_t*>(s.src) + off);
    const dev::global_ptr<uint8_t> dst =
        dev::as_global(static_cast<uint8_t*>(s.dst) + off);

    const bool aligned = ((reinterpret_cast<uintptr_t>(src) |
                           reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    if (aligned) {
      // 16 B per lane: 64 lanes × 16 = 1024 B per iteration; nontemporal —
      // streamed bytes are never re-read from cache by this kernel
      uint64_t nvec = len >> 4;
      for (uint64_t i = lane; i < nvec; i += 64) {
        v16 v = __builtin_nontemporal_load((dev::global_ptr<const v16>)src + i);
        __builtin_nontemporal_store(v, (dev::global_ptr<v16>)dst + i);
      }
      // tail bytes
      for (uint64_t i = (nvec << 4) + lane; i < len; i += 64) dst[i] = src[i];
    } else {
      for (uint64_t i = lane; i < len; i += 64) dst[i] = src[i];
    }
  }
}

__global__ void __launch_bounds__(kBlock)
fill_kernel(ulong1* __restrict__ out, uint64_t nwords, uint64_t seed) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
       i < nwords; i += stride)
    out[i] = digest::splitmix64(seed ^ i);
}

__global__ void __launch_bounds__(kBlock)
verify_kernel(const ulong1* __restrict__ in, uint64_t nwords, uint64_t seed,
              ulong1* __restrict__ bad) {
  uint64_t local = 0;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
       i < nwords; i += stride)
    if (in[i] != digest::splitmix64(seed ^ i)) ++local;
  if (local) atomicAdd(bad, local);
}

int grid_for(uint64_t work_items) {
  uint64_t blocks = (work_items + kBlock - 1) / kBlock;
  if (blocks < 1) blocks = 1;
  if (blocks > 4096) blocks = 4096;
  return static_cast<int>(blocks);
}

// batched_copy() returns BEFORE the stream executes, so the staged
// descriptors must outlive the call: see DescStaging::in_flight.
thread_local DescStaging g_copy_stage;

}  // namespace

Result<void> batched_copy(const CopyDesc* descs, uint32_t n, hipStream_t stream) {
  if (n == 0) return {};
  const BatchBlock b{n};
  BB_RETURN_IF_ERROR(g_copy_stage.acquire(b.upload_bytes()));
  const uint64_t total = fill_block(b, g_copy_stage.pinned, descs, kChunk);
  if (total == 0) return {};

  void* d_block = g_copy_stage.device;
  BB_HIP_TRY(hipMemcpyAsync(d_block, g_copy_stage.pinned, b.upload_bytes(),
                            hipMemcpyHostToDevice, stream));
  // one wave per chunk → want total waves ≈ total chunks
  const int blocks = grid_for(total * 64);
  batched_copy_kernel<<<blocks, kBlock, 0, stream>>>(
      b.descs(d_block), b.prefix(d_block), n, total);
  BB_HIP_LAUNCHED("batched_copy_kernel");
  return g_copy_stage.in_flight(stream);
}

Result<void> fill_pattern(void* dev_ptr, uint64_t nbytes, uint64_t seed,
                          hipStream_t stream) {
  const uint64_t nwords = nbytes / 8;
  if (nwords > 0) {
    fill_kernel<<<grid_for(nwords / 4), kBlock, 0, stream>>>(
        static_cast<ulong1*>(dev_ptr), nwords, seed);
    BB_HIP_LAUNCHED("fill_kernel");
  }
  return {};
}

Result<uint64_t> verify_pattern(const void* dev_ptr, uint64_t nbytes, uint64_t seed,
                                hipStream_t stream) {
  const uint64_t nwords = nbytes / 8;
  ulong1* d_bad = nullptr;
  BB_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_bad), 8));
  BB_HIP_TRY(hipMemsetAsync(d_bad, 0, 8, stream));
  if (nwords > 0) {
    verify_kernel<<<grid_for(nwords / 4), kBlock, 0, stream>>>(
        static_cast<const ulong1*>(dev_ptr), nwords, seed, d_bad);
    BB_HIP_LAUNCHED("verify_kernel");
  }
  uint64_t bad = 0;
  BB_HIP_TRY(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, stream));
  BB_HIP_TRY(hipStreamSynchronize(stream));
  BB_HIP_TRY(hipFree(d_bad));
  return bad;
}

namespace {
// Shared pool of pre-created non-blocking transfer streams. The library
// never touches the legacy (null) stream — a null-stream op in ANY thread
// fails while a hipGraph capture is open — but streams must NOT be
// per-thread: the staged fan-out paths run on short-lived std::async
// threads, and creating/destroying a stream per thread costs milliseconds
// on ROCm (measured 9× on the NVMe get leg). Round-robin over a fixed pool
// instead; a per-stream mutex keeps each async+sync pair atomic.
constexpr int kXferStreams = 8;
struct XferPool {
  hipStream_t s[kXferStreams] = {};
  std::mutex mu[kXferStreams];
  std::atomic<uint32_t> next{0};
  std::once_flag once;
  hipError_t init_rc = hipSuccess;

  hipError_t ensure() {
    std::call_once(once, [this] {
      for (int i = 0; i < kXferStreams; ++i) {
        init_rc = hipStreamCreateWithFlags(&s[i], hipStreamNonBlocking);
        if (init_rc != hipSuccess) return;
      }
    });
    return init_rc;
  }
};
XferPool g_xfer;
}  // namespace

namespace {
constexpr int kMaxDevices = 64;
std::mutex g_anchor_mu;
hipStream_t g_anchor[kMaxDevices] = {};
}  // namespace

Result<hipStream_t> staging_anchor() {
  int dev = 0;
  BB_HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDevices)
    return Error{ErrorCode::INVALID_ARGUMENT, "device index out of range"};
  std::lock_guard<std::mutex> g(g_anchor_mu);
  if (!g_anchor[dev])
    BB_HIP_TRY(hipStreamCreateWithFlags(&g_anchor[dev], hipStreamNonBlocking));
  return g_anchor[dev];
}

Result<void> acquire_xfer_stream(XferStream& out) {
  BB_HIP_TRY(g_xfer.ensure());
  const uint32_t i = g_xfer.next.fetch_add(1) % kXferStreams;
  out.lock = std::unique_lock<std::mutex>(g_xfer.mu[i]);
  out.stream = g_xfer.s[i];
  return {};
}

Result<void> copy_sync(void* dst, const void* src, uint64_t nbytes, int kind) {
  if (nbytes == 0) return {};
  XferStream xs;
  BB_RETURN_IF_ERROR(acquire_xfer_stream(xs));
  BB_HIP_TRY(hipMemcpyAsync(dst, src, nbytes,
                            static_cast<hipMemcpyKind>(kind), xs.stream));
  BB_HIP_TRY(hipStreamSynchronize(xs.stream));
  return {};
}

Result<uint64_t> device_malloc(uint64_t nbytes, int device) {
  BB_HIP_TRY(hipSetDevice(device));
  void* p = nullptr;
  BB_HIP_TRY(hipMalloc(&p, nbytes));
  return reinterpret_cast<uint64_t>(p);
}

Result<void> device_free(uint64_t ptr) {
  BB_HIP_TRY(hipFree(reinterpret_cast<void*>(ptr)));
  return {};
}

Result<void> upload(uint64_t dst_dev, const void* src, uint64_t nbytes) {
  return copy_sync(reinterpret_cast<void*>(dst_dev), src, nbytes,
                   hipMemcpyHostToDevice);
}

Result<void> download(void* dst, uint64_t src_dev, uint64_t nbytes) {
  return copy_sync(dst, reinterpret_cast<const void*>(src_dev), nbytes,
                   hipMemcpyDeviceToHost);
}

Result<void> sync() {
  BB_HIP_TRY(hipDeviceSynchronize());
  return {};
}

}  // namespace blackbird::gpu
