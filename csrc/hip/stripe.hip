// fused_stripe — striped puts and gets in one copy+digest launch (gfx950).
// A striped object is moved as segments (one per shard); the scrubber needs
// each shard's own digest and the keystone the object's. Both come out of
// one pass: the tile walk of digest_device.hip.h loads every tile once, runs
// one MFMA and one group fold on it, and mixes the fold twice — with the
// slot counted from the segment's start and from the object's start
// (digest_spec.h: position enters only through the mix).
#include <hip/hip_runtime.h>

#include <cstring>

#include "batch_launch.hip.h"
#include "blackbird/gpu/gpu_kernels.h"
#include "digest_device.hip.h"
#include "hip_common.h"

namespace blackbird::gpu {

using namespace blackbird::gpu::dev;

namespace {

// {segs[nseg] | prefix[nseg] | obj_sizes[nobj] | seg_acc[nseg] | obj_acc[nobj]}
// in one allocation, same offsets in the pinned host image and on the
// device. The first three are uploaded together; the two accumulator arrays
// are zeroed, finalized and read back as one range.
struct StripeBlock {
  uint32_t nseg, nobj;

  size_t upload_bytes() const {
    return nseg * (sizeof(StripeSeg) + sizeof(uint64_t)) + nobj * sizeof(uint64_t);
  }
  size_t out_bytes() const { return (size_t{nseg} + nobj) * sizeof(uint64_t); }
  size_t bytes() const { return upload_bytes() + out_bytes(); }

  StripeSeg* segs(void* base) const { return static_cast<StripeSeg*>(base); }
  uint64_t* prefix(void* base) const {
    return reinterpret_cast<uint64_t*>(segs(base) + nseg);
  }
  uint64_t* obj_sizes(void* base) const { return prefix(base) + nseg; }
  uint64_t* seg_acc(void* base) const { return obj_sizes(base) + nobj; }
  uint64_t* obj_acc(void* base) const { return seg_acc(base) + nseg; }
};
static_assert(sizeof(StripeSeg) % sizeof(uint64_t) == 0);

__global__ void __launch_bounds__(kBlock)
fused_stripe_kernel(const StripeSeg* __restrict__ segs,
                    const uint64_t* __restrict__ tile_prefix, uint32_t nseg,
                    uint64_t total_tiles, unsigned long long* __restrict__ seg_acc,
                    unsigned long long* __restrict__ obj_acc) {
  digest_walk<true, kWalkDepth>(segs, tile_prefix, nseg, total_tiles, seg_acc,
                                obj_acc);
}

// acc = {seg_acc[nseg] | obj_acc[nobj]}: each sum finalized with the length
// it was taken over.
__global__ void fused_stripe_finalize_kernel(
    const StripeSeg* __restrict__ segs, uint32_t nseg,
    const uint64_t* __restrict__ obj_sizes, uint32_t nobj,
    unsigned long long* __restrict__ acc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nseg) acc[i] = digest::finalize(acc[i], segs[i].nbytes);
  else if (i - nseg < nobj) acc[i] = digest::finalize(acc[i], obj_sizes[i - nseg]);
}

thread_local DescStaging g_stripe_stage;

}  // namespace

Result<void> fused_stripe(const StripeSeg* segs, uint32_t nseg,
                          const uint64_t* obj_sizes, uint32_t nobj,
                          uint64_t* out_seg_digests, uint64_t* out_obj_digests,
                          hipStream_t stream) {
  if (nseg == 0) return {};
  BB_RETURN_IF_ERROR(check_stripe_segs(segs, nseg, obj_sizes, nobj));
  XferStream xs;  // never the legacy stream
  if (!stream) {
    BB_RETURN_IF_ERROR(acquire_xfer_stream(xs));
    stream = xs.stream;
  }
  const StripeBlock b{nseg, nobj};
  BB_RETURN_IF_ERROR(g_stripe_stage.acquire(b.bytes()));
  void* host = g_stripe_stage.pinned;
  void* dev = g_stripe_stage.device;

  std::memcpy(b.segs(host), segs, nseg * sizeof(StripeSeg));
  std::memcpy(b.obj_sizes(host), obj_sizes, nobj * sizeof(uint64_t));
  uint64_t* h_prefix = b.prefix(host);
  uint64_t total = 0;
  for (uint32_t i = 0; i < nseg; ++i) {
    h_prefix[i] = total;
    total += (segs[i].nbytes + digest::kTileBytes - 1) / digest::kTileBytes;
  }
  BB_HIP_TRY(hipMemcpyAsync(dev, host, b.upload_bytes(), hipMemcpyHostToDevice,
                            stream));

  auto* d_seg_acc = reinterpret_cast<unsigned long long*>(b.seg_acc(dev));
  auto* d_obj_acc = reinterpret_cast<unsigned long long*>(b.obj_acc(dev));
  BB_HIP_TRY(hipMemsetAsync(d_seg_acc, 0, b.out_bytes(), stream));
  if (total > 0) {
    fused_stripe_kernel<<<digest_grid(total), kBlock, 0, stream>>>(
        b.segs(dev), b.prefix(dev), nseg, total, d_seg_acc, d_obj_acc);
    BB_HIP_LAUNCHED("fused_stripe_kernel");
  }
  const uint32_t nout = nseg + nobj;
  fused_stripe_finalize_kernel<<<(nout + 255) / 256, 256, 0, stream>>>(
      b.segs(dev), nseg, b.obj_sizes(dev), nobj, d_seg_acc);
  BB_HIP_LAUNCHED("fused_stripe_finalize_kernel");
  uint64_t* h_out = b.seg_acc(host);
  BB_HIP_TRY(hipMemcpyAsync(h_out, d_seg_acc, b.out_bytes(),
                            hipMemcpyDeviceToHost, stream));
  BB_HIP_TRY(hipStreamSynchronize(stream));
  std::memcpy(out_seg_digests, h_out, nseg * sizeof(uint64_t));
  std::memcpy(out_obj_digests, b.obj_acc(host), nobj * sizeof(uint64_t));
  return {};
}

}  // namespace blackbird::gpu
