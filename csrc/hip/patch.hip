// fused_patch — in-place range patches with an incremental digest in one
// launch (gfx950). A run of new bytes replaces the old ones where they lie in
// the pool; the recorded digests of its shard and its object move by the
// difference of the patched tiles' terms alone (patch_plan.h), so only those
// tiles are read: old and new once each, one write. The patch walk of
// digest_device.hip.h pushes both tiles through the MFMA and the group fold
// and mixes the folds with the slot counted from the shard's start and from
// the object's start. Tiles overwritten in part, the edges of a byte range,
// go to a second kernel behind it: one wave per edge composes the tile of old
// and new bytes and adds term(composed) - term(old) to the same sums.
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

// {segs[nseg] | prefix[nseg] | edges[nedge] | lens[n] | old[n] | acc[n]},
// n = nshard + nobj, in one allocation, same offsets in the pinned host image
// and on the device. edges = the tiles overwritten in part, none in a launch
// of whole-tile runs; lens = {shard_lens | obj_sizes}; old = the recorded digests, as
// recorded, {shard | object}; acc = the wrapped sums of term(new) - term(old)
// of the patched tiles, zeroed on the device, finalized in place over old and
// read back as one range. {segs | prefix | edges | lens} is all a plan needs to
// keep; old changes every step.
struct PatchBlock {
  uint32_t nseg, nshard, nobj;
  uint32_t nedge = 0;

  uint32_t nacc() const { return nshard + nobj; }
  size_t out_bytes() const { return size_t{nacc()} * sizeof(uint64_t); }
  size_t fixed_bytes() const {  // {segs | prefix | edges | lens}
    return nseg * (sizeof(PatchSeg) + sizeof(uint64_t)) +
           nedge * sizeof(PatchEdge) + out_bytes();
  }
  size_t upload_bytes() const { return fixed_bytes() + out_bytes(); }  // + old
  size_t bytes() const { return upload_bytes() + out_bytes(); }

  PatchSeg* segs(void* base) const { return static_cast<PatchSeg*>(base); }
  uint64_t* prefix(void* base) const {
    return reinterpret_cast<uint64_t*>(segs(base) + nseg);
  }
  PatchEdge* edges(void* base) const {
    return reinterpret_cast<PatchEdge*>(prefix(base) + nseg);
  }
  uint64_t* lens(void* base) const {
    return reinterpret_cast<uint64_t*>(edges(base) + nedge);
  }
  uint64_t* old(void* base) const { return lens(base) + nacc(); }
  uint64_t* acc(void* base) const { return old(base) + nacc(); }
};
static_assert(sizeof(PatchSeg) % sizeof(uint64_t) == 0);
static_assert(sizeof(PatchEdge) % sizeof(uint64_t) == 0);

__global__ void __launch_bounds__(kBlock)
fused_patch_kernel(const PatchSeg* __restrict__ segs,
                   const uint64_t* __restrict__ tile_prefix, uint32_t nseg,
                   uint64_t total_tiles, unsigned long long* __restrict__ shard_acc,
                   unsigned long long* __restrict__ obj_acc) {
  patch_walk<kPatchDepth>(segs, tile_prefix, nseg, total_tiles, shard_acc,
                          obj_acc);
}

// One wave per edge tile (patch_edge_tile): the descriptor comes by scalar
// loads, the tile's old bytes and the window's new ones byte by byte. Launched
// behind fused_patch_kernel on the same stream, into the same accumulators.
__global__ void __launch_bounds__(kBlock)
fused_patch_edge_kernel(const PatchEdge* __restrict__ edges, uint32_t nedge,
                        unsigned long long* __restrict__ shard_acc,
                        unsigned long long* __restrict__ obj_acc) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave = wave_uniform(threadIdx.x >> 6);
  const uint32_t e = blockIdx.x * kWavesPerBlock + wave;
  if (e >= nedge) return;
  patch_edge_tile(edges[e], lane, shard_acc, obj_acc);
}

// Each delta added to the sum its old digest was finalized from, and the
// result finalized with the same length: a delta of 0 gives the old digest
// back bit for bit.
__global__ void fused_patch_finalize_kernel(const uint64_t* __restrict__ lens,
                                            const uint64_t* __restrict__ old,
                                            uint32_t n,
                                            unsigned long long* __restrict__ acc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    acc[i] = digest::finalize(digest::unfinalize(old[i], lens[i]) + acc[i],
                              lens[i]);
}

// The host image of {segs | prefix | edges | lens}. Returns the runs' total
// tile count.
uint64_t fill_patch_block(const PatchBlock& b, void* host, const PatchSeg* segs,
                          const PatchEdge* edges, const uint64_t* shard_lens,
                          const uint64_t* obj_sizes) {
  if (b.nseg) std::memcpy(b.segs(host), segs, b.nseg * sizeof(PatchSeg));
  if (b.nedge) std::memcpy(b.edges(host), edges, b.nedge * sizeof(PatchEdge));
  uint64_t* lens = b.lens(host);
  if (b.nshard) std::memcpy(lens, shard_lens, b.nshard * sizeof(uint64_t));
  if (b.nobj) std::memcpy(lens + b.nshard, obj_sizes, b.nobj * sizeof(uint64_t));
  return fill_prefix(segs, b.nseg, digest::kTileBytes, b.prefix(host));
}

// The patch step over an uploaded block whose old digests are in place: zero
// the accumulators -> patch and hash every tile of the runs -> the edge
// tiles, if any -> finalize over the old digests -> the new digests,
// {shard | object}, to host_out (pinned). One chain on one stream, no
// parallel branch. Only enqueues; the caller synchronizes or captures
// `stream` (the twin of enqueue_stripe).
Result<void> enqueue_patch(void* device_block, const PatchBlock& b,
                           uint64_t total_tiles, uint64_t* host_out,
                           hipStream_t stream) {
  auto* d_acc = reinterpret_cast<unsigned long long*>(b.acc(device_block));
  BB_HIP_TRY(hipMemsetAsync(d_acc, 0, b.out_bytes(), stream));
  if (total_tiles > 0) {
    fused_patch_kernel<<<digest_grid(total_tiles), kBlock, 0, stream>>>(
        b.segs(device_block), b.prefix(device_block), b.nseg, total_tiles,
        d_acc, d_acc + b.nshard);
    BB_HIP_LAUNCHED("fused_patch_kernel");
  }
  if (b.nedge > 0) {
    fused_patch_edge_kernel<<<(b.nedge + kWavesPerBlock - 1) / kWavesPerBlock,
                              kBlock, 0, stream>>>(
        b.edges(device_block), b.nedge, d_acc, d_acc + b.nshard);
    BB_HIP_LAUNCHED("fused_patch_edge_kernel");
  }
  fused_patch_finalize_kernel<<<(b.nacc() + 255) / 256, 256, 0, stream>>>(
      b.lens(device_block), b.old(device_block), b.nacc(), d_acc);
  BB_HIP_LAUNCHED("fused_patch_finalize_kernel");
  BB_HIP_TRY(hipMemcpyAsync(host_out, d_acc, b.out_bytes(),
                            hipMemcpyDeviceToHost, stream));
  return {};
}

thread_local DescStaging g_patch_stage;

}  // namespace

int patch_walk_depth() { return kPatchDepth; }

Result<void> fused_patch(const PatchSeg* segs, uint32_t nseg,
                         const uint64_t* shard_lens, const uint64_t* shard_old,
                         uint32_t nshard, const uint64_t* obj_sizes,
                         const uint64_t* obj_old, uint32_t nobj,
                         uint64_t* out_shard_digests, uint64_t* out_obj_digests,
                         hipStream_t stream, const PatchEdge* edges,
                         uint32_t nedge) {
  BB_RETURN_IF_ERROR(check_patch_segs(segs, nseg, shard_lens, shard_old, nshard,
                                      obj_sizes, obj_old, nobj));
  BB_RETURN_IF_ERROR(check_patch_edges(edges, nedge, segs, nseg, shard_lens,
                                       nshard, obj_sizes, nobj));
  // before any HIP call: a launch without a tile needs no device
  uint64_t total = 0;
  for (uint32_t i = 0; i < nseg; ++i) total += tile_count(segs[i].nbytes);
  if (total == 0 && nedge == 0) {  // nothing patched: every digest stands
    if (nshard) std::memcpy(out_shard_digests, shard_old, nshard * sizeof(uint64_t));
    if (nobj) std::memcpy(out_obj_digests, obj_old, nobj * sizeof(uint64_t));
    return {};
  }
  XferStream xs;  // never the legacy stream
  if (!stream) {
    BB_RETURN_IF_ERROR(acquire_xfer_stream(xs));
    stream = xs.stream;
  }
  const PatchBlock b{nseg, nshard, nobj, nedge};
  BB_RETURN_IF_ERROR(g_patch_stage.acquire(b.bytes()));
  void* host = g_patch_stage.pinned;
  void* dev = g_patch_stage.device;

  fill_patch_block(b, host, segs, edges, shard_lens, obj_sizes);
  uint64_t* h_old = b.old(host);
  if (nshard) std::memcpy(h_old, shard_old, nshard * sizeof(uint64_t));
  if (nobj) std::memcpy(h_old + nshard, obj_old, nobj * sizeof(uint64_t));
  BB_HIP_TRY(hipMemcpyAsync(dev, host, b.upload_bytes(), hipMemcpyHostToDevice,
                            stream));
  uint64_t* h_out = b.acc(host);
  BB_RETURN_IF_ERROR(enqueue_patch(dev, b, total, h_out, stream));
  BB_HIP_TRY(hipStreamSynchronize(stream));
  if (nshard) std::memcpy(out_shard_digests, h_out, nshard * sizeof(uint64_t));
  if (nobj) std::memcpy(out_obj_digests, h_out + nshard, nobj * sizeof(uint64_t));
  return {};
}

// ---------------- hipGraph-replayed patch session step (FusedPatchPlan) ----
// The patch counterpart of FusedStripePlan: {segs | prefix | edges | lens} is
// uploaded
// once; what changes every step, the old digests, rides the captured chain as
// its first node, a copy from the plan's pinned zone, which the last node
// fills with the new digests.

struct FusedPatchPlan::Impl : GraphStep {};

FusedPatchPlan::~FusedPatchPlan() { delete impl_; }

Result<void> FusedPatchPlan::build(const PatchSeg* segs, uint32_t nseg,
                                   const uint64_t* shard_lens, uint32_t nshard,
                                   const uint64_t* obj_sizes, uint32_t nobj,
                                   int device, const PatchEdge* edges,
                                   uint32_t nedge) {
  if (impl_) return Error{ErrorCode::INVALID_ARGUMENT, "plan already built"};
  if (nseg == 0 && nedge == 0)
    return Error{ErrorCode::INVALID_ARGUMENT, "empty run list"};
  BB_RETURN_IF_ERROR(
      check_patch_geometry(segs, nseg, shard_lens, nshard, obj_sizes, nobj));
  BB_RETURN_IF_ERROR(check_patch_edges(edges, nedge, segs, nseg, shard_lens,
                                       nshard, obj_sizes, nobj));
  const PatchBlock b{nseg, nshard, nobj, nedge};
  auto h_block = std::make_unique<unsigned char[]>(b.fixed_bytes());
  const uint64_t total =
      fill_patch_block(b, h_block.get(), segs, edges, shard_lens, obj_sizes);
  if (total == 0 && nedge == 0) return Error{ErrorCode::INVALID_ARGUMENT, "zero-byte batch"};

  BB_HIP_TRY(hipSetDevice(device));
  auto impl = std::make_unique<Impl>();
  BB_RETURN_IF_ERROR(impl->prepare(h_block.get(), b.fixed_bytes(), b.bytes(),
                                   b.out_bytes()));
  BB_RETURN_IF_ERROR(impl->capture([&](hipStream_t s) -> Result<void> {
    BB_HIP_TRY(hipMemcpyAsync(b.old(impl->dev), impl->h_out, b.out_bytes(),
                              hipMemcpyHostToDevice, s));
    return enqueue_patch(impl->dev, b, total, impl->h_out, s);
  }));
  nshard_ = nshard;
  nobj_ = nobj;
  impl_ = impl.release();
  return {};
}

Result<void> FusedPatchPlan::run(const uint64_t* shard_old,
                                 const uint64_t* obj_old,
                                 uint64_t* out_shard_digests,
                                 uint64_t* out_obj_digests) {
  if (!impl_) return Error{ErrorCode::INVALID_ARGUMENT, "plan not built"};
  BB_RETURN_IF_ERROR(check_patch_digests(shard_old, nshard_, obj_old, nobj_));
  uint64_t* zone = impl_->h_out;
  if (nshard_) std::memcpy(zone, shard_old, nshard_ * sizeof(uint64_t));
  if (nobj_) std::memcpy(zone + nshard_, obj_old, nobj_ * sizeof(uint64_t));
  BB_RETURN_IF_ERROR(impl_->replay());
  if (nshard_) std::memcpy(out_shard_digests, zone, nshard_ * sizeof(uint64_t));
  if (nobj_) std::memcpy(out_obj_digests, zone + nshard_, nobj_ * sizeof(uint64_t));
  return {};
}

}  // namespace blackbird::gpu
