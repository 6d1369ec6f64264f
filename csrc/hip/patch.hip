// fused_patch — in-place range patches with an incremental digest in one
// launch (gfx950). A run of new bytes replaces the old ones where they lie in
// the pool; the recorded digests of its shard and its object move by the
// difference of the patched tiles' terms alone (patch_plan.h), so only those
// tiles are read: old and new once each, one write. The patch walk of
// digest_device.hip.h pushes both tiles through the MFMA and the group fold
// and mixes the folds with the slot counted from the shard's start and from
// the object's start.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "batch_launch.hip.h"
#include "blackbird/gpu/gpu_kernels.h"
#include "digest_device.hip.h"
#include "hip_common.h"

namespace blackbird::gpu {

using namespace blackbird::gpu::dev;

namespace {

// {segs[nseg] | prefix[nseg] | lens[nshard + nobj] | acc[nshard + nobj]} in
// one allocation, same offsets in the pinned host image and on the device.
// lens = {shard_lens | obj_sizes}; acc = {shard_acc | obj_acc}, seeded by the
// host with unfinalize(old digest, length). All of it is uploaded in one
// copy; acc is finalized in place and read back as one range.
struct PatchBlock {
  uint32_t nseg, nshard, nobj;

  uint32_t nacc() const { return nshard + nobj; }
  size_t out_bytes() const { return size_t{nacc()} * sizeof(uint64_t); }
  size_t bytes() const {
    return nseg * (sizeof(PatchSeg) + sizeof(uint64_t)) + 2 * out_bytes();
  }

  PatchSeg* segs(void* base) const { return static_cast<PatchSeg*>(base); }
  uint64_t* prefix(void* base) const {
    return reinterpret_cast<uint64_t*>(segs(base) + nseg);
  }
  uint64_t* lens(void* base) const { return prefix(base) + nseg; }
  uint64_t* acc(void* base) const { return lens(base) + nacc(); }
};
static_assert(sizeof(PatchSeg) % sizeof(uint64_t) == 0);

__global__ void __launch_bounds__(kBlock)
fused_patch_kernel(const PatchSeg* __restrict__ segs,
                   const uint64_t* __restrict__ tile_prefix, uint32_t nseg,
                   uint64_t total_tiles, unsigned long long* __restrict__ shard_acc,
                   unsigned long long* __restrict__ obj_acc) {
  patch_walk<kPatchDepth>(segs, tile_prefix, nseg, total_tiles, shard_acc,
                          obj_acc);
}

// Each sum finalized with the length its digest is taken over.
__global__ void fused_patch_finalize_kernel(const uint64_t* __restrict__ lens,
                                            uint32_t n,
                                            unsigned long long* __restrict__ acc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) acc[i] = digest::finalize(acc[i], lens[i]);
}

thread_local DescStaging g_patch_stage;

}  // namespace

int patch_walk_depth() { return kPatchDepth; }

Result<void> fused_patch(const PatchSeg* segs, uint32_t nseg,
                         const uint64_t* shard_lens, const uint64_t* shard_old,
                         uint32_t nshard, const uint64_t* obj_sizes,
                         const uint64_t* obj_old, uint32_t nobj,
                         uint64_t* out_shard_digests, uint64_t* out_obj_digests,
                         hipStream_t stream) {
  BB_RETURN_IF_ERROR(check_patch_segs(segs, nseg, shard_lens, shard_old, nshard,
                                      obj_sizes, obj_old, nobj));
  // before any HIP call: a launch without a tile needs no device
  std::vector<uint64_t> prefix(nseg);
  const uint64_t total =
      fill_prefix(segs, nseg, digest::kTileBytes, prefix.data());
  if (total == 0) {  // nothing patched: every digest stands
    if (nshard) std::memcpy(out_shard_digests, shard_old, nshard * sizeof(uint64_t));
    if (nobj) std::memcpy(out_obj_digests, obj_old, nobj * sizeof(uint64_t));
    return {};
  }
  XferStream xs;  // never the legacy stream
  if (!stream) {
    BB_RETURN_IF_ERROR(acquire_xfer_stream(xs));
    stream = xs.stream;
  }
  const PatchBlock b{nseg, nshard, nobj};
  BB_RETURN_IF_ERROR(g_patch_stage.acquire(b.bytes()));
  void* host = g_patch_stage.pinned;
  void* dev = g_patch_stage.device;

  std::memcpy(b.segs(host), segs, nseg * sizeof(PatchSeg));
  std::memcpy(b.prefix(host), prefix.data(), nseg * sizeof(uint64_t));
  uint64_t* h_lens = b.lens(host);
  uint64_t* h_acc = b.acc(host);
  for (uint32_t i = 0; i < nshard; ++i) {
    h_lens[i] = shard_lens[i];
    h_acc[i] = digest::unfinalize(shard_old[i], shard_lens[i]);
  }
  for (uint32_t i = 0; i < nobj; ++i) {
    h_lens[nshard + i] = obj_sizes[i];
    h_acc[nshard + i] = digest::unfinalize(obj_old[i], obj_sizes[i]);
  }
  BB_HIP_TRY(hipMemcpyAsync(dev, host, b.bytes(), hipMemcpyHostToDevice, stream));

  auto* d_acc = reinterpret_cast<unsigned long long*>(b.acc(dev));
  fused_patch_kernel<<<digest_grid(total), kBlock, 0, stream>>>(
      b.segs(dev), b.prefix(dev), nseg, total, d_acc, d_acc + nshard);
  BB_HIP_LAUNCHED("fused_patch_kernel");
  fused_patch_finalize_kernel<<<(b.nacc() + 255) / 256, 256, 0, stream>>>(
      b.lens(dev), b.nacc(), d_acc);
  BB_HIP_LAUNCHED("fused_patch_finalize_kernel");
  BB_HIP_TRY(hipMemcpyAsync(h_acc, d_acc, b.out_bytes(), hipMemcpyDeviceToHost,
                            stream));
  BB_HIP_TRY(hipStreamSynchronize(stream));
  if (nshard) std::memcpy(out_shard_digests, h_acc, nshard * sizeof(uint64_t));
  if (nobj) std::memcpy(out_obj_digests, h_acc + nshard, nobj * sizeof(uint64_t));
  return {};
}

}  // namespace blackbird::gpu
