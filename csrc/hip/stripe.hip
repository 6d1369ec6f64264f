// fused_stripe — striped puts and gets in one copy+digest launch (gfx950).
// A striped object is moved as segments (one per shard); the scrubber needs
// each shard's own digest and the keystone the object's. Both come out of
// one pass: the tile walk of digest_device.hip.h loads every tile once, runs
// one MFMA and one group fold on it, and mixes the fold twice — with the
// slot counted from the segment's start and from the object's start
// (digest_spec.h: position enters only through the mix).
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>

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

// The host image of the uploaded part: segs, obj_sizes and the exclusive
// prefix sum of the segments' tile counts. Returns the total tile count.
uint64_t fill_stripe_block(const StripeBlock& b, void* host,
                           const StripeSeg* segs, const uint64_t* obj_sizes) {
  std::memcpy(b.segs(host), segs, b.nseg * sizeof(StripeSeg));
  std::memcpy(b.obj_sizes(host), obj_sizes, b.nobj * sizeof(uint64_t));
  return fill_prefix(segs, b.nseg, digest::kTileBytes, b.prefix(host));
}

// The striped step over an uploaded block: zero both accumulator arrays →
// copy and hash every tile → finalize per segment and per object → both
// digest arrays, {seg | obj}, to host_out (pinned). Only enqueues; the caller
// synchronizes or captures `stream` (the twin of enqueue_digest).
Result<void> enqueue_stripe(void* device_block, const StripeBlock& b,
                            uint64_t total_tiles, uint64_t* host_out,
                            hipStream_t stream) {
  auto* d_seg_acc =
      reinterpret_cast<unsigned long long*>(b.seg_acc(device_block));
  auto* d_obj_acc =
      reinterpret_cast<unsigned long long*>(b.obj_acc(device_block));
  BB_HIP_TRY(hipMemsetAsync(d_seg_acc, 0, b.out_bytes(), stream));
  if (total_tiles > 0) {
    fused_stripe_kernel<<<digest_grid(total_tiles), kBlock, 0, stream>>>(
        b.segs(device_block), b.prefix(device_block), b.nseg, total_tiles,
        d_seg_acc, d_obj_acc);
    BB_HIP_LAUNCHED("fused_stripe_kernel");
  }
  const uint32_t nout = b.nseg + b.nobj;
  fused_stripe_finalize_kernel<<<(nout + 255) / 256, 256, 0, stream>>>(
      b.segs(device_block), b.nseg, b.obj_sizes(device_block), b.nobj,
      d_seg_acc);
  BB_HIP_LAUNCHED("fused_stripe_finalize_kernel");
  BB_HIP_TRY(hipMemcpyAsync(host_out, d_seg_acc, b.out_bytes(),
                            hipMemcpyDeviceToHost, stream));
  return {};
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

  const uint64_t total = fill_stripe_block(b, host, segs, obj_sizes);
  BB_HIP_TRY(hipMemcpyAsync(dev, host, b.upload_bytes(), hipMemcpyHostToDevice,
                            stream));
  uint64_t* h_out = b.seg_acc(host);
  BB_RETURN_IF_ERROR(enqueue_stripe(dev, b, total, h_out, stream));
  BB_HIP_TRY(hipStreamSynchronize(stream));
  std::memcpy(out_seg_digests, h_out, nseg * sizeof(uint64_t));
  std::memcpy(out_obj_digests, b.obj_acc(host), nobj * sizeof(uint64_t));
  return {};
}

// -------------- hipGraph-replayed striped session step (FusedStripePlan) ----
// The striped counterpart of FusedPutPlan: the block is uploaded once and the
// step enqueue_stripe issues — accumulator reset included — is captured as
// one chain and replayed with one hipGraphLaunch.

struct FusedStripePlan::Impl : GraphStep {};

FusedStripePlan::~FusedStripePlan() { delete impl_; }

Result<void> FusedStripePlan::build(const StripeSeg* segs, uint32_t nseg,
                                    const uint64_t* obj_sizes, uint32_t nobj,
                                    int device) {
  if (impl_) return Error{ErrorCode::INVALID_ARGUMENT, "plan already built"};
  if (nseg == 0) return Error{ErrorCode::INVALID_ARGUMENT, "empty segment list"};
  BB_RETURN_IF_ERROR(check_stripe_segs(segs, nseg, obj_sizes, nobj));
  BB_HIP_TRY(hipSetDevice(device));
  auto impl = std::make_unique<Impl>();
  const StripeBlock b{nseg, nobj};

  auto h_block = std::make_unique<unsigned char[]>(b.upload_bytes());
  const uint64_t total = fill_stripe_block(b, h_block.get(), segs, obj_sizes);
  if (total == 0) return Error{ErrorCode::INVALID_ARGUMENT, "zero-byte batch"};

  BB_RETURN_IF_ERROR(impl->prepare(h_block.get(), b.upload_bytes(), b.bytes(),
                                   b.out_bytes()));
  BB_RETURN_IF_ERROR(impl->capture([&](hipStream_t s) {
    return enqueue_stripe(impl->dev, b, total, impl->h_out, s);
  }));
  nseg_ = nseg;
  nobj_ = nobj;
  impl_ = impl.release();
  return {};
}

Result<void> FusedStripePlan::run(uint64_t* out_seg_digests,
                                  uint64_t* out_obj_digests) {
  if (!impl_) return Error{ErrorCode::INVALID_ARGUMENT, "plan not built"};
  BB_RETURN_IF_ERROR(impl_->replay());
  std::memcpy(out_seg_digests, impl_->h_out, nseg_ * sizeof(uint64_t));
  std::memcpy(out_obj_digests, impl_->h_out + nseg_, nobj_ * sizeof(uint64_t));
  return {};
}

}  // namespace blackbird::gpu
