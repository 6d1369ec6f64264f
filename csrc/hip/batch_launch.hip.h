// Host side of every batched launch: one block layout, one prefix sum, one
// grid rule and one enqueue sequence, shared by checksum_batch, fused_put,
// FusedPutPlan (digest.hip) and batched_copy (memops.hip) — and the capture
// scaffolding (GraphStep) under both session plans, FusedPutPlan and
// FusedStripePlan (stripe.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "blackbird/gpu/gpu_kernels.h"
#include "digest_device.hip.h"
#include "hip_common.h"

namespace blackbird::gpu {

// {descs[n] | prefix[n] | out[n]} in one allocation; the same offsets hold
// for the pinned host image and the device copy. descs+prefix are uploaded
// together; out holds the digest accumulators (unused by batched_copy).
struct BatchBlock {
  uint32_t n;

  size_t upload_bytes() const { return n * (sizeof(CopyDesc) + sizeof(uint64_t)); }
  size_t out_bytes() const { return n * sizeof(uint64_t); }
  size_t bytes() const { return upload_bytes() + out_bytes(); }

  CopyDesc* descs(void* base) const { return static_cast<CopyDesc*>(base); }
  uint64_t* prefix(void* base) const {
    return reinterpret_cast<uint64_t*>(descs(base) + n);
  }
  uint64_t* out(void* base) const { return prefix(base) + n; }
};

// Tiles that hold nbytes, the last one possibly in part: the digest's 1-KiB
// tiles, or the work quantum of another kernel.
inline uint64_t tile_count(uint64_t nbytes,
                           uint64_t quantum = digest::kTileBytes) {
  return (nbytes + quantum - 1) / quantum;
}

// The exclusive prefix sum of the tile counts of CopyDescs, StripeSegs or
// PatchSegs, which the kernels' find_seg searches. Returns the total.
template <typename Desc>
uint64_t fill_prefix(const Desc* descs, uint32_t n, uint64_t quantum,
                     uint64_t* prefix) {
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; ++i) {
    prefix[i] = total;
    total += tile_count(descs[i].nbytes, quantum);
  }
  return total;
}

// Copies the caller's descriptors into the host image (they may already be
// there) and writes their prefix sum. Returns the total number of quanta.
inline uint64_t fill_block(const BatchBlock& b, void* host, const CopyDesc* descs,
                           uint64_t quantum) {
  CopyDesc* h_descs = b.descs(host);
  if (descs != h_descs) std::memcpy(h_descs, descs, b.n * sizeof(CopyDesc));
  return fill_prefix(h_descs, b.n, quantum, b.prefix(host));
}

// Two tiles per wave, capped at 4096 workgroups; the kernels split whatever
// is left over into contiguous per-wave ranges.
inline int digest_grid(uint64_t total_tiles) {
  const uint64_t waves = (total_tiles + 1) / 2;
  uint64_t blocks = (waves + dev::kWavesPerBlock - 1) / dev::kWavesPerBlock;
  if (blocks < 1) blocks = 1;
  if (blocks > 4096) blocks = 4096;
  return static_cast<int>(blocks);
}

// Defined in digest.hip.
__global__ void bbhash64_batch_kernel(const CopyDesc*, const uint64_t*, uint32_t,
                                      uint64_t, unsigned long long*);
__global__ void fused_put_kernel(const CopyDesc*, const uint64_t*, uint32_t,
                                 uint64_t, unsigned long long*, uint64_t);
__global__ void fused_get_kernel(const CopyDesc*, const uint64_t*, uint32_t,
                                 uint64_t, unsigned long long*, uint64_t);
__global__ void bbhash64_finalize_kernel(const CopyDesc*, uint32_t,
                                         unsigned long long*);

// The digest step over an uploaded block: zero the accumulators → hash
// (kCopy: and copy) every tile → finalize per object → digests to host_out
// (pinned). Only enqueues; the caller synchronizes or captures `stream`.
// kCopy: the last warm.bytes of the batch, in whole tiles, are its warm tail
// (gpu_kernels.h, WarmTail); this is the one place that turns them into the
// kernels' tile index.
template <bool kCopy>
Result<void> enqueue_digest(void* device_block, uint32_t n, uint64_t total_tiles,
                            uint64_t* host_out, hipStream_t stream,
                            WarmTail warm = {}) {
  const BatchBlock b{n};
  const CopyDesc* d_descs = b.descs(device_block);
  const uint64_t* d_prefix = b.prefix(device_block);
  auto* d_out = reinterpret_cast<unsigned long long*>(b.out(device_block));
  BB_HIP_TRY(hipMemsetAsync(d_out, 0, b.out_bytes(), stream));
  if (total_tiles > 0) {
    const int blocks = digest_grid(total_tiles);
    if constexpr (kCopy) {
      const uint64_t warm_tiles =
          std::min<uint64_t>(total_tiles, warm.bytes / digest::kTileBytes);
      const uint64_t warm_begin = total_tiles - warm_tiles;
      if (warm.loads) {
        fused_get_kernel<<<blocks, dev::kBlock, 0, stream>>>(
            d_descs, d_prefix, n, total_tiles, d_out, warm_begin);
        BB_HIP_LAUNCHED("fused_get_kernel");
      } else {
        fused_put_kernel<<<blocks, dev::kBlock, 0, stream>>>(
            d_descs, d_prefix, n, total_tiles, d_out, warm_begin);
        BB_HIP_LAUNCHED("fused_put_kernel");
      }
    } else {
      bbhash64_batch_kernel<<<blocks, dev::kBlock, 0, stream>>>(
          d_descs, d_prefix, n, total_tiles, d_out);
      BB_HIP_LAUNCHED("bbhash64_batch_kernel");
    }
  }
  bbhash64_finalize_kernel<<<(n + 255) / 256, 256, 0, stream>>>(d_descs, n, d_out);
  BB_HIP_LAUNCHED("bbhash64_finalize_kernel");
  BB_HIP_TRY(hipMemcpyAsync(host_out, d_out, b.out_bytes(), hipMemcpyDeviceToHost,
                            stream));
  return {};
}

// A step captured once and replayed: what FusedPutPlan, FusedStripePlan and
// FusedPatchPlan (patch.hip) own and how they capture. The step's descriptors
// live in a device block uploaded once; its digests land in a pinned buffer
// (which FusedPatchPlan also uploads a step's old digests from); capture and
// replay happen on a dedicated non-blocking stream.
struct GraphStep {
  hipStream_t stream = nullptr;   // dedicated capture/replay stream
  hipGraphExec_t exec = nullptr;
  void* dev = nullptr;            // the uploaded block + its accumulators
  uint64_t* h_out = nullptr;      // pinned digest landing zone
  size_t out_bytes = 0;

  GraphStep() = default;
  GraphStep(const GraphStep&) = delete;
  GraphStep& operator=(const GraphStep&) = delete;
  ~GraphStep() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (dev) (void)hipFree(dev);
    if (h_out) (void)hipHostFree(h_out);
    if (stream) (void)hipStreamDestroy(stream);
  }

  // stream, device block of block_bytes with the first upload_bytes copied
  // from h_block, pinned landing zone of out_bytes_
  Result<void> prepare(const void* h_block, size_t upload_bytes,
                       size_t block_bytes, size_t out_bytes_) {
    out_bytes = out_bytes_;
    BB_HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    BB_HIP_TRY(hipMalloc(&dev, block_bytes));
    BB_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_out), out_bytes,
                             hipHostMallocDefault));
    return copy_sync(dev, h_block, upload_bytes, hipMemcpyHostToDevice);
  }

  // Captures what enqueue(stream) issues and instantiates it.
  template <typename Enqueue>
  Result<void> capture(Enqueue&& enqueue) {
    hipGraph_t graph = nullptr;
    // Relaxed: every captured op is issued on `stream` by THIS thread, so
    // the stricter modes buy nothing — and ROCm's ThreadLocal mode still
    // fails OTHER threads' legacy-stream hipMemcpy while a capture is open
    // ("operation would make the legacy stream depend on a capturing blocking
    // stream"), which a concurrent client must be free to do.
    BB_HIP_TRY(hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed));
    // no early return while the capture is open: collect the error, end the
    // capture, then report
    const Result<void> cap = enqueue(stream);
    hipError_t endc = hipStreamEndCapture(stream, &graph);
    if (!cap.ok()) {
      if (graph) (void)hipGraphDestroy(graph);
      return Error{cap.code(), "graph capture: " + cap.message()};
    }
    BB_HIP_TRY(endc);
    hipError_t inst = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    BB_HIP_TRY(inst);
    return {};
  }

  // one graph launch; returns with the digests in h_out
  Result<void> replay() {
    BB_HIP_TRY(hipGraphLaunch(exec, stream));
    BB_HIP_TRY(hipStreamSynchronize(stream));
    return {};
  }
};

}  // namespace blackbird::gpu
