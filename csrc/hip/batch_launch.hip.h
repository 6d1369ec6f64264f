// Host side of every batched launch: one block layout, one prefix sum, one
// grid rule and one enqueue sequence, shared by checksum_batch, fused_put,
// FusedPutPlan (digest.hip) and batched_copy (memops.hip).
#pragma once

#include <hip/hip_runtime.h>

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

// Copies the caller's descriptors into the host image (they may already be
// there) and writes the exclusive prefix sum of their sizes in units of
// `quantum` bytes. Returns the total number of quanta.
inline uint64_t fill_block(const BatchBlock& b, void* host, const CopyDesc* descs,
                           uint64_t quantum) {
  CopyDesc* h_descs = b.descs(host);
  uint64_t* h_prefix = b.prefix(host);
  if (descs != h_descs) std::memcpy(h_descs, descs, b.n * sizeof(CopyDesc));
  uint64_t total = 0;
  for (uint32_t i = 0; i < b.n; ++i) {
    h_prefix[i] = total;
    total += (h_descs[i].nbytes + quantum - 1) / quantum;
  }
  return total;
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
                                 uint64_t, unsigned long long*);
__global__ void bbhash64_finalize_kernel(const CopyDesc*, uint32_t,
                                         unsigned long long*);

// The digest step over an uploaded block: zero the accumulators → hash
// (kCopy: and copy) every tile → finalize per object → digests to host_out
// (pinned). Only enqueues; the caller synchronizes or captures `stream`.
template <bool kCopy>
Result<void> enqueue_digest(void* device_block, uint32_t n, uint64_t total_tiles,
                            uint64_t* host_out, hipStream_t stream) {
  const BatchBlock b{n};
  const CopyDesc* d_descs = b.descs(device_block);
  const uint64_t* d_prefix = b.prefix(device_block);
  auto* d_out = reinterpret_cast<unsigned long long*>(b.out(device_block));
  BB_HIP_TRY(hipMemsetAsync(d_out, 0, b.out_bytes(), stream));
  if (total_tiles > 0) {
    const int blocks = digest_grid(total_tiles);
    if constexpr (kCopy) {
      fused_put_kernel<<<blocks, dev::kBlock, 0, stream>>>(d_descs, d_prefix, n,
                                                           total_tiles, d_out);
      BB_HIP_LAUNCHED("fused_put_kernel");
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

}  // namespace blackbird::gpu
