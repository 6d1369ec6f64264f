// Host-callable entry points for the CDNA4 (gfx950) kernels of the HBM tier.
// All functions are implemented in csrc/hip/*.hip, compiled for gfx950 only.
// They fail loudly (Result error) when no GPU is present — no silent CPU
// fallback on a GPU box.
#pragma once

#include <cstdint>

#include "blackbird/common/result.h"
#include "blackbird/gpu/patch_plan.h"
#include "blackbird/gpu/stripe_plan.h"

// Forward decl to avoid pulling hip_runtime into every TU.
struct ihipStream_t;
typedef struct ihipStream_t* hipStream_t;

namespace blackbird::gpu {

bool available();        // HIP runtime + ≥1 device
int device_count();

// ------------------------------------------------------------- checksum
// 64-bit object digest computed on-device with MFMA i8 matrix products:
// data is consumed as 32×32 int8 tiles A_t; each tile is projected through a
// fixed pseudo-random matrix B (mfma_i32_32x32x32_i8), the 32×32 i32 product
// is folded to a u64, weighted by splitmix64(tile_index) and summed (u64
// wraparound) — position-sensitive, order-independent (parallel-friendly),
// bitwise reproducible on CPU (gpu_checksum_cpu). Tail bytes (<1 KiB) are
// hashed on the fly inside the kernel.
//
// dev_ptr: device pointer; stream: HIP stream (nullptr = default).
// Result digest is written to *out (host) after stream sync by the _sync
// variant; the async variant writes into a device/pinned u64.
Result<uint64_t> checksum_sync(const void* dev_ptr, uint64_t nbytes, int device,
                               hipStream_t stream);
Result<void> checksum_async(const void* dev_ptr, uint64_t nbytes,
                            uint64_t* dev_out, hipStream_t stream);

// Exact CPU reference of the same digest (used for verification and for
// DRAM/disk-tier objects).
uint64_t checksum_cpu(const void* ptr, uint64_t nbytes);

// Streaming CPU digest: hash `nbytes` starting at tile index `first_tile`
// (chunk must start on a 1 KiB tile boundary of the object; the final chunk
// may end mid-tile — zero-padded per spec). Combine partials with +, then
// checksum_cpu_finalize(H, object_size).
uint64_t checksum_cpu_tiles(const void* chunk, uint64_t nbytes,
                            uint64_t first_tile);
uint64_t checksum_cpu_finalize(uint64_t h, uint64_t object_nbytes);
// The sum H a recorded digest was finalized from: what a range patch adds
// checksum_cpu_tiles(new) - checksum_cpu_tiles(old) to before it finalizes
// again (patch_plan.h).
uint64_t checksum_cpu_unfinalize(uint64_t digest, uint64_t object_nbytes);

// Waves the batched digest/fused kernels launch for a batch of total_tiles
// 1-KiB tiles; each owns one contiguous range of ceil(total_tiles / waves)
// tiles. And the depth of the copying kernels' load pipeline: a run of full
// tiles enters its steady loop from 3 * depth tiles on. Both exist only so
// that tests can size a batch against the kernels as built; nothing else
// should depend on them.
uint64_t digest_grid_waves(uint64_t total_tiles);
int digest_walk_depth();

// Batched digest: one launch hashes n device buffers; out_digests is a HOST
// array of n results (call blocks on `stream`).
Result<void> checksum_batch(const void* const* dev_ptrs, const uint64_t* sizes,
                            uint32_t n, uint64_t* out_digests, int device,
                            hipStream_t stream);

// Single 32×32×32 i8 MFMA with the assumed fragment layout (layout
// verification test). host_a/host_b: 1024 int8 row-major; host_c: 1024 i32.
Result<void> mfma_i8_probe(const int8_t* host_a, const int8_t* host_b,
                           int32_t* host_c, int device);

// ------------------------------------------- batched scatter/gather copy
// One launch serves a whole batch of object transfers (the fused multi-object
// path behind batch_put/batch_get). CopyDesc is the one descriptor of every
// batched kernel, on host and device.
struct CopyDesc {
  const void* src;
  void* dst;
  uint64_t nbytes;
};
// descs: HOST array of n descriptors (the implementation stages them and
// uploads them on `stream`). Returns once the work is enqueued.
Result<void> batched_copy(const CopyDesc* descs, uint32_t n, hipStream_t stream);

// Fused put: copy whole single-shard objects (src→dst, both device-local,
// 16B-aligned) AND compute their bbhash64 digests in ONE kernel — the data
// is read once instead of twice (copy + hash). out_digests: HOST array
// (call blocks on `stream`).
using PutDesc = CopyDesc;
// The warm tail of a copy+digest batch: its last `bytes`, in whole tiles and
// rounded down to whole per-wave ranges. A put (loads == false) stores the
// tail plainly where all else is stored nontemporally, so that it stays in
// the Infinity Cache; the get of the same batch shortly afterwards (loads ==
// true) loads the tail plainly where all else is loaded nontemporally, and is
// served on-die (KERNELS.md, "Store policy"). A residency hint: bytes and
// digests do not depend on it. bytes 0: none; more than the batch: all of it.
struct WarmTail {
  uint64_t bytes = 0;
  bool loads = false;
};
Result<void> fused_put(const PutDesc* descs, uint32_t n, uint64_t* out_digests,
                       hipStream_t stream, WarmTail warm = {});

// Fused striped transfer: copy every segment src→dst (both device-visible,
// 16B-aligned) AND compute, reading the data once, two digests — per segment
// the bbhash64 of its bytes alone (what the keystone records per shard), per
// object finalize(Σ checksum_cpu_tiles(segment bytes, first_tile), size) over
// the segments naming it: the object's bbhash64 when they cover it exactly.
// Segments of one object may sit anywhere in the list. The arguments go
// through check_stripe_segs (stripe_plan.h) before any HIP call. obj_sizes
// and both outputs are HOST arrays (call blocks on `stream`; nullptr = a
// stream of the shared transfer pool). nseg == 0 returns at once.
Result<void> fused_stripe(const StripeSeg* segs, uint32_t nseg,
                          const uint64_t* obj_sizes, uint32_t nobj,
                          uint64_t* out_seg_digests, uint64_t* out_obj_digests,
                          hipStream_t stream);

// Fused in-place range patch: overwrite every run's bytes at dst with the
// new bytes at src (both device-visible, 16B-aligned) AND move the recorded
// digests of the shards and objects the runs name, reading only the patched
// tiles — old and new once each. out_shard_digests[i] is
// finalize(unfinalize(shard_old[i], shard_lens[i]) + Σ term(new tiles) −
// Σ term(old tiles), shard_lens[i]) over the runs naming shard i, slots
// counted from the shard's start; out_obj_digests likewise with slots counted
// from the object's start. A shard or object no run names keeps its digest.
// When the bytes outside the runs are what the old digests were taken over,
// these are the bbhash64 digests of the patched shards and objects; when they
// are not, the new digests are as wrong as the old ones were. The arguments
// go through check_patch_segs (patch_plan.h) before any HIP call. All arrays
// are HOST arrays (call blocks on `stream`; nullptr = a stream of the shared
// transfer pool). After an error past the check, the runs' bytes are torn.
//
// edges: tiles overwritten in part (PatchEdge, patch_plan.h), the head and the
// tail of a range that is not whole tiles. A second kernel on the same stream,
// one wave per edge, composes each tile of its old bytes and the new ones in
// [lo, hi), stores only those, and adds term(composed) − term(old) to the same
// sums; they go through check_patch_edges with the runs. No alignment is
// asked of an edge. A launch of edges alone (nseg == 0) is legal; with no
// edge the HIP calls are those of a launch of runs.
Result<void> fused_patch(const PatchSeg* segs, uint32_t nseg,
                         const uint64_t* shard_lens, const uint64_t* shard_old,
                         uint32_t nshard, const uint64_t* obj_sizes,
                         const uint64_t* obj_old, uint32_t nobj,
                         uint64_t* out_shard_digests, uint64_t* out_obj_digests,
                         hipStream_t stream, const PatchEdge* edges = nullptr,
                         uint32_t nedge = 0);
// Depth of fused_patch's load pipeline, per stream (old and new): a run of
// full tiles enters its steady loop from 3 * depth tiles on. For tests to
// size themselves, as digest_walk_depth.
int patch_walk_depth();

// Pre-instantiated fused-put step for batch sessions (fixed desc list every
// step): descriptors live on-device (uploaded once by build), and the whole
// step — digest reset → fused copy+digest kernel → finalize → digest D2H —
// is captured in a hipGraph and replayed as ONE graph launch per step
// instead of 5 stream ops. run() blocks until the digests are in
// out_digests[n].
class FusedPutPlan {
 public:
  FusedPutPlan() = default;
  ~FusedPutPlan();
  FusedPutPlan(const FusedPutPlan&) = delete;
  FusedPutPlan& operator=(const FusedPutPlan&) = delete;

  // warm: as fused_put's; captured with the step
  Result<void> build(const PutDesc* descs, uint32_t n, int device,
                     WarmTail warm = {});
  bool ready() const { return impl_ != nullptr; }
  uint32_t size() const { return n_; }
  Result<void> run(uint64_t* out_digests);

 private:
  struct Impl;
  Impl* impl_ = nullptr;
  uint32_t n_ = 0;
};

// The same for a striped session (fixed segment list every step): build
// checks the segments (check_stripe_segs) before any HIP call, uploads
// {segs | prefix | obj_sizes} once and captures accumulator reset →
// fused_stripe kernel → finalize → D2H of both digest arrays as one chain;
// run() is one graph launch and blocks until out_seg_digests[nseg] and
// out_obj_digests[nobj] are filled. size() is the segment count.
class FusedStripePlan {
 public:
  FusedStripePlan() = default;
  ~FusedStripePlan();
  FusedStripePlan(const FusedStripePlan&) = delete;
  FusedStripePlan& operator=(const FusedStripePlan&) = delete;

  Result<void> build(const StripeSeg* segs, uint32_t nseg,
                     const uint64_t* obj_sizes, uint32_t nobj, int device);
  bool ready() const { return impl_ != nullptr; }
  uint32_t size() const { return nseg_; }
  Result<void> run(uint64_t* out_seg_digests, uint64_t* out_obj_digests);

 private:
  struct Impl;
  Impl* impl_ = nullptr;
  uint32_t nseg_ = 0, nobj_ = 0;
};

// The same for a patch session (fixed run list every step, other old digests
// every step): build checks the runs (check_patch_geometry) before any HIP
// call, uploads {segs | prefix | lens} once and captures H2D of the old
// digests from the plan's pinned zone → accumulator reset → fused_patch
// kernel → finalize over the old digests → D2H of the new ones into the same
// zone, as one chain. run() refuses an old digest of 0 (check_patch_digests)
// before it launches anything, then is one graph launch and blocks until
// out_shard_digests[nshard] and out_obj_digests[nobj] are filled; they are
// what fused_patch gives for the same arguments, bit for bit. size() is the
// shard count. Edges ride the plan as they ride fused_patch: checked with the
// runs, uploaded with them, their kernel one more node of the chain between
// the run kernel and finalize; a plan of edges alone is legal.
class FusedPatchPlan {
 public:
  FusedPatchPlan() = default;
  ~FusedPatchPlan();
  FusedPatchPlan(const FusedPatchPlan&) = delete;
  FusedPatchPlan& operator=(const FusedPatchPlan&) = delete;

  Result<void> build(const PatchSeg* segs, uint32_t nseg,
                     const uint64_t* shard_lens, uint32_t nshard,
                     const uint64_t* obj_sizes, uint32_t nobj, int device,
                     const PatchEdge* edges = nullptr, uint32_t nedge = 0);
  bool ready() const { return impl_ != nullptr; }
  uint32_t size() const { return nshard_; }
  Result<void> run(const uint64_t* shard_old, const uint64_t* obj_old,
                   uint64_t* out_shard_digests, uint64_t* out_obj_digests);

 private:
  struct Impl;
  Impl* impl_ = nullptr;
  uint32_t nshard_ = 0, nobj_ = 0;
};

// Simple utilities used by tests/benchmarks.
Result<void> fill_pattern(void* dev_ptr, uint64_t nbytes, uint64_t seed,
                          hipStream_t stream);
Result<uint64_t> verify_pattern(const void* dev_ptr, uint64_t nbytes, uint64_t seed,
                                hipStream_t stream);  // returns #mismatched u64

// Synchronous copy on one stream of a shared pool of NON-BLOCKING streams
// (held under that stream's mutex for the call). The library never
// issues work on the legacy (null) stream: ROCm fails legacy-stream ops in
// EVERY thread while any hipGraph capture is open (sessions capture their
// step graphs lazily), so all blocking copies route through here. kind is a
// hipMemcpyKind (int to keep hip types out of this header).
Result<void> copy_sync(void* dst, const void* src, uint64_t nbytes, int kind);

// Raw device memory helpers (Python test harness / bench plumbing).
Result<uint64_t> device_malloc(uint64_t nbytes, int device);
Result<void> device_free(uint64_t ptr);
Result<void> upload(uint64_t dst_dev, const void* src, uint64_t nbytes);
Result<void> download(void* dst, uint64_t src_dev, uint64_t nbytes);
Result<void> sync();

}  // namespace blackbird::gpu
