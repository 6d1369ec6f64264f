// GPU-native client: put/get whose SOURCE/DESTINATION buffers live in the
// client GPU's HBM. This is the MI355X replacement for the reference's UCX
// one-sided RMA (blackbird_client.cpp:204-351):
//   * shards in HBM pools on the same node are reached through
//     hipIpcOpenMemHandle and written with hipMemcpyAsync device↔device —
//     one-sided over xGMI (7 p2p links × ≈153 GB/s), no worker CPU involved;
//     multiple shards fan out over rotating HIP streams to drive several
//     links concurrently (ring-free, per the xGMI topology),
//   * small-object batches go through ONE fused scatter/gather kernel launch
//     (gpu::batched_copy) instead of per-object copies,
//   * object digests are computed by the MFMA checksum kernel, batched —
//     one launch hashes the whole batch,
//   * SHM / TCP pools fall back through a pinned staging buffer.
#pragma once

#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <unordered_map>

#include "blackbird/client/client.h"
#include "blackbird/client/placement_cache.h"
#include "blackbird/client/shuffle.h"
#include "blackbird/gpu/gpu_kernels.h"

namespace blackbird {

class RcclEngine;
struct PoolRef;  // batch_util.h

class GpuClient {
 public:
  // Wraps an existing (connected) metadata client; `device` is the client
  // GPU whose buffers the put/get calls take.
  GpuClient(Client& base, int device);
  ~GpuClient();

  Result<void> init();

  Result<void> put_device(const ObjectKey& key, const void* dev_ptr,
                          uint64_t size, const PlacementConfig& cfg = {});
  Result<uint64_t> get_device(const ObjectKey& key, void* dev_ptr,
                              uint64_t capacity, bool verify = false);

  struct DevPutItem {
    ObjectKey key;
    const void* ptr;
    uint64_t size;
  };
  struct DevGetItem {
    ObjectKey key;
    void* ptr;
    uint64_t capacity;
  };
  // ---- batch sessions (steady-state fast path) ----
  // Callers that re-put/re-get the SAME batch (same keys, buffers, order)
  // every step can pass a session object; after the first full round trip,
  // a put step costs one fused kernel launch + two tiny RPCs (8-byte upsert
  // start, token+digests commit) and a get step costs one kernel launch and
  // zero RPCs. Any server-side placement change invalidates the server
  // session (SESSION_STALE) and the client transparently falls back to the
  // full path. Sessions are bound to one item list: the item pointers are
  // re-validated each step. Requires replace=true, checksum=true
  // and the placement cache enabled; replicated placements are supported
  // (one destination per copy).
  // Striped placements (max_workers_per_copy > 1) have the same three fast
  // paths when every item of the batch rides the fused_stripe launch (each
  // copy accepted by gpu::plan_stripe, every shard a 16B-aligned
  // device-visible pointer): the session then carries the segment list
  // instead of descs, a step replays a FusedStripePlan, and a put step
  // commits the object digests together with every shard's own
  // (BATCH_COMMIT_TOKEN_SHARDS). The server session is opened with
  // BATCH_SESSION_OPEN between BATCH_PUT_START and the commit, while PENDING
  // pins the placements just resolved. A session is either all single-shard
  // or all striped; a batch with one item on another route gets none.
  // A session's hold on the placement cache is a PlacementCache::Binding:
  // the cache that issued it refuses it once any placement was erased,
  // moved or cleared, so a step never reaches a dead cache entry.
  // Worker death: a re-placing put kills the bindings (moved placements
  // end sessions holding the old pool addresses). A get-session step
  // BEFORE any re-put reads the dead pool one-sidedly: across processes
  // (production: dmabuf-IPC imports pin the memory) that is a digest
  // mismatch → RPC fallback; an EMBEDDED worker that frees its pool
  // in-process can fault — stop in-process workers only after their
  // clients.
  // Where one item's kernel objects and segments sit in a launch: a striped
  // one, a patch (first_seg then counts shards), or a plain session's desc
  // list, where every desc is both an object and its only segment.
  struct StripeRange {
    uint32_t item;
    uint32_t first_obj, ncopies;  // kernel objects [first_obj, +ncopies)
    uint32_t first_seg;           // segments of copy 0, copy 1, … back to back
  };
  struct SessionCore {
    PlacementCache::Binding binding;  // the items' digest slots, item order
    // plain form: user buffer ↔ pool range, one desc PER COPY per item (same
    // user buffer, one pool range per replica), item order
    std::vector<gpu::PutDesc> descs;
    // striped form (descs empty): the fused_stripe argument lists
    std::vector<gpu::StripeSeg> segs;
    std::vector<uint64_t> obj_sizes;
    // both forms: item i's range into the lists above
    std::vector<StripeRange> ranges;
    bool striped() const { return !segs.empty(); }
    // hipGraph replay of the step (lists fixed ⇒ captured once, one graph
    // launch per step), of the form the session holds; built lazily on the
    // first session step
    std::shared_ptr<gpu::FusedPutPlan> plan;
    std::shared_ptr<gpu::FusedStripePlan> stripe_plan;
    bool plan_failed = false;  // capture unsupported: stay on launches
    // a new desc list (`copies` descs per item): a kept plan would replay
    // the old one
    void rebind(std::vector<gpu::PutDesc> d, uint32_t copies,
                PlacementCache::Binding b) {
      descs = std::move(d);
      segs.clear();
      obj_sizes.clear();
      ranges.resize(descs.size() / copies);
      for (uint32_t i = 0; i < ranges.size(); ++i)
        ranges[i] = {i, i * copies, copies, i * copies};
      reset(std::move(b));
    }
    void rebind_striped(std::vector<gpu::StripeSeg> s,
                        std::vector<uint64_t> sizes,
                        std::vector<StripeRange> r, PlacementCache::Binding b) {
      descs.clear();
      segs = std::move(s);
      obj_sizes = std::move(sizes);
      ranges = std::move(r);
      reset(std::move(b));
    }

   private:
    void reset(PlacementCache::Binding b) {
      binding = std::move(b);
      plan.reset();
      stripe_plan.reset();
      plan_failed = false;
    }
  };
  struct BatchPutSession : SessionCore {  // descs: src=user, dst=pool
    uint64_t token = 0;  // server put-session token (0 = not established)
  };
  struct BatchGetSession : SessionCore {  // descs: src=pool, dst=user
    bool complete = false;  // covers every item
  };

  // One metadata RPC + fused transfers + one batched checksum launch.
  Result<std::vector<int32_t>> batch_put_device(
      const std::vector<DevPutItem>& items, const PlacementConfig& cfg = {},
      BatchPutSession* sess = nullptr);
  Result<std::vector<int32_t>> batch_get_device(
      const std::vector<DevGetItem>& items, bool verify = false,
      BatchGetSession* sess = nullptr);
  // fast-path step counters (tests/bench introspection)
  uint64_t session_put_steps() const { return session_put_steps_; }
  uint64_t session_get_steps() const { return session_get_steps_; }
  // session steps that replayed the captured hipGraph (vs per-op launches)
  uint64_t session_graph_steps() const { return session_graph_steps_; }
  // striped items moved by ONE fused_stripe launch (copy + shard digests +
  // object digest in one pass) instead of copy + two digest launches (puts)
  // or copy + verify launch (gets)
  uint64_t striped_fused_items() const { return striped_fused_items_; }
  uint64_t striped_fused_get_items() const { return striped_fused_get_items_; }

  // ---- ranged access ----
  // A byte range of an object, to or from a device buffer.
  struct DevRangeGet {
    ObjectKey key;
    uint64_t offset;
    void* ptr;
    uint64_t length;
  };
  struct DevRangePatch {
    ObjectKey key;
    uint64_t offset;
    const void* ptr;
    uint64_t length;
  };
  // Ranged gets: one BATCH_GET_WORKERS, then ONE gpu::batched_copy launch
  // over the pieces that lie in device-visible shards (any offset and
  // length inside the object); pieces of other shards are staged — the whole
  // shard where it fits the staging buffer, then the slice. The first copy
  // that covers the object serves an item; a failed staged read moves on to
  // the next. UNVERIFIED: no recorded digest covers a range. A range that
  // leaves its object is INVALID_ARGUMENT for that item.
  Result<std::vector<int32_t>> batch_get_device_range(
      const std::vector<DevRangeGet>& items);
  Result<void> get_device_range(const ObjectKey& key, uint64_t offset,
                                void* dev_ptr, uint64_t length);
  // In-place range patches: one BATCH_PATCH_START, then ONE gpu::fused_patch
  // launch over all items and all their copies — it writes the new bytes
  // over the old ones and moves every shard digest and object checksum by
  // the patched tiles' terms — then one BATCH_PUT_COMPLETE. Copies of an
  // item whose new object digests disagree had diverged: CHECKSUM_MISMATCH,
  // and the key is cancelled (its bytes are already written). A failed
  // launch cancels every item that rode it (torn bytes, as after a failed
  // in-place upsert). An item that cannot be patched in place — no recorded
  // checksum or shard digest, a range that is not whole 1 KiB tiles (but for
  // one ending at the object's end), a copy gpu::plan_patch refuses, a shard
  // or a source that is not a 16B-aligned device-visible pointer — takes the
  // REWRITE route: its patch start is aborted, the whole object is fetched
  // (verified) into a temporary device buffer, the range overlaid and the
  // object put back with replace=true; right on every tier and placement.
  // The patched keys leave this client's placement cache, which also ends
  // every put and get session bound to them; other clients' cached verified
  // gets mismatch and fall back to the RPC path.
  //
  // Byte granularity (set_patch_edge_tiles(true), default off): each copy is
  // planned with gpu::plan_patch_bytes, and a range that is not whole tiles
  // rides the SAME launch as whole-tile runs between at most two edge tiles,
  // each composed on the GPU of its old bytes and the new ones
  // (gpu::PatchEdge). Only the patched tiles are read, so — unlike the rewrite
  // route, which verifies the whole object — a corrupt byte outside the range
  // is not noticed here; it stays detectable, the digests move by differences.
  // Still on the rewrite route: an item whose interior run's source and pool
  // address are not both 16B-aligned (the caller's pointer and the offset
  // must share their phase mod 16), a pool that does not resolve, a shard
  // without a digest. Edge tiles ask no alignment. Sessions keep the edge
  // list with the run list, so unaligned items establish and replay one.
  //
  // Patch sessions: a caller that patches the SAME item list (keys, offsets,
  // buffers, lengths, order) every step passes a session object. The first
  // call runs the path above and, if every item rode the fused launch and
  // every replica agreed, opens a server session (BATCH_SESSION_OPEN, while
  // the patch start's PENDING pins the placements) before it commits by key;
  // the session keeps the launch's run list. Every later call costs one
  // BATCH_PATCH_START_TOKEN (8 bytes out; the recorded digests back, flat —
  // the server's, so that another writer's re-put in place is subtracted
  // right), one replay of a captured gpu::FusedPatchPlan (session_step's
  // ladder: launches under BB_NO_HIPGRAPH or after a failed capture or
  // replay) and one BATCH_COMMIT_TOKEN_SHARDS. A start that is refused has
  // flipped nothing: the session is dropped and the same call runs the full
  // path, which may establish it again. Past the start the bytes are being
  // written: a failed launch or commit cancels every key and ends the
  // session; a replica that disagrees is CHECKSUM_MISMATCH and cancelled,
  // the others commit by key, and the session ends. The session holds no
  // placement-cache binding: the server's epoch check at every start is what
  // guards the pool addresses it keeps.
  struct BatchPatchSession {
    uint64_t token = 0;  // server session token (0 = not established)
    std::vector<DevRangePatch> bound;  // the item list the lists below serve
    // the fused_patch argument lists but for the old digests
    std::vector<gpu::PatchSeg> segs;
    std::vector<gpu::PatchEdge> edges;  // set_patch_edge_tiles: may be all
    std::vector<uint64_t> shard_lens, obj_sizes;
    std::vector<uint32_t> copy_shards;  // shards of each kernel object
    std::vector<StripeRange> ranges;    // item i's objects and shards
    std::shared_ptr<gpu::FusedPatchPlan> plan;  // built on the first step
    bool plan_failed = false;  // capture unsupported: stay on launches
    void end() {
      token = 0;
      plan.reset();
      plan_failed = false;
    }
  };
  Result<std::vector<int32_t>> batch_patch_device(
      const std::vector<DevRangePatch>& items,
      BatchPatchSession* sess = nullptr);
  Result<void> patch_device(const ObjectKey& key, uint64_t offset,
                            const void* dev_ptr, uint64_t length);
  // items patched by the fused_patch launch / by the rewrite route
  uint64_t patched_fused_items() const { return patched_fused_items_; }
  uint64_t patched_rewrite_items() const { return patched_rewrite_items_; }
  // patch steps served by a session (start by token, one launch, commit by
  // token); their items count in patched_fused_items too
  uint64_t session_patch_steps() const { return session_patch_steps_; }

  // ---- pipelined batches: begin returns a token immediately; the batch
  // runs on a background thread (metadata RPCs of batch N+1 overlap the
  // GPU transfers of batch N — the single-client equivalent of running
  // two lanes). The RPC connection multiplexes by request id and kernels
  // serialize per stream, so in-flight batches never conflict; buffers
  // passed to an async batch must stay alive until async_wait returns.
  Result<uint64_t> batch_put_async(std::vector<DevPutItem> items,
                                   PlacementConfig cfg = {});
  Result<uint64_t> batch_get_async(std::vector<DevGetItem> items,
                                   bool verify = false);
  Result<std::vector<int32_t>> async_wait(uint64_t token);

  // Fused copy kernel for device-visible shards (default on): one launch
  // serves the whole batch, reading/writing IPC-mapped PEER memory directly
  // over xGMI (a kernel store drives all 7 links at once, with no per-shard
  // hipMemcpyAsync issue cost). set_fused_copy(false) falls back to SDMA
  // (hipMemcpyAsync on rotating streams) for every transfer.
  void set_fused_copy(bool on) { fused_copy_ = on; }

  // Warm-tail budget of the copy+digest launches (gpu::WarmTail): up to this
  // many bytes at the end of every such put launch are stored so that they
  // stay in the Infinity Cache, and a get loads the end of its batch to
  // match: the get of a batch that this client has just put reads that much
  // on-die. Bytes and digests do not depend on it. Striped and patch
  // launches take none. A session's captured step keeps the budget it was
  // built with. Default: what profiles/warm_tail_checks.md selected for two
  // lanes, which between them keep 256 MiB, the size of the cache.
  static constexpr uint64_t kDefaultWarmTailBytes = 128ull << 20;
  void set_warm_tail_bytes(uint64_t bytes) { warm_tail_bytes_ = bytes; }
  uint64_t warm_tail_bytes() const { return warm_tail_bytes_; }

  // In-place patches at byte granularity (batch_patch_device above). Off:
  // every range that is not whole tiles takes the rewrite route.
  void set_patch_edge_tiles(bool on) { patch_edge_tiles_ = on; }
  bool patch_edge_tiles() const { return patch_edge_tiles_; }

  // ---- collective batch shuffle (RCCL over xGMI; see shuffle.h) ----
  // Every rank calls this together: want[p] lists the objects this rank
  // wants FROM rank p (received contiguously at want[p].recv_base). Served
  // objects are resolved out of this rank's visible pools (placement cache
  // first, metadata RPC fallback) and move in grouped all-to-all-v calls.
  Result<void> batch_shuffle_rccl(RcclEngine& comm,
                                  const std::vector<ShuffleWant>& want);

  // ---- verified placement cache (opt-in) ----
  // Remembers {pool, offset, size, digest} from this client's own puts and
  // serves later gets of those keys WITHOUT a metadata RPC: a one-sided
  // read through the fused copy+digest kernel, validated against the
  // remembered digest. A mismatch (object moved/replaced/evicted) falls
  // back to the RPC path transparently — the optimistic read costs nothing
  // extra because the gather kernel hashes the bytes it already has in
  // registers. Caveat: a REMOVE by another client is not observed until the
  // freed bytes are actually overwritten (content-validated staleness);
  // call invalidate()/clear_placement_cache() where that matters.
  // The cache itself (map, lock, enabled flag, session bindings) is a
  // PlacementCache; these forward to it.
  void set_placement_cache(bool on) { cache_.set_enabled(on); }
  void invalidate(const std::vector<ObjectKey>& keys);
  void clear_placement_cache() { cache_.clear(); }

  // test hook: the device-visible base this client resolves a pool to
  uint8_t* pool_base_for_test(const PoolId& id) { return resolve_pool_base(id); }

 private:
  // Resolve a shard to a device-visible pointer (local or IPC-mapped peer
  // HBM, GPU-mapped host tier); nullptr if the pool is not device-visible
  // from this process.
  uint8_t* resolve_device_ptr(const ShardPlacement& s);
  Result<std::vector<int32_t>> batch_put_device_once(
      const std::vector<DevPutItem>& items, const PlacementConfig& cfg,
      BatchPutSession* sess);
  Result<std::vector<int32_t>> batch_get_device_once(
      const std::vector<DevGetItem>& items, bool verify,
      BatchGetSession* sess);
  // device-visible base of a pool (HBM local, IPC peer, or GPU-mapped host
  // tier); nullptr → staged fallback. `hint`: access info already at hand.
  uint8_t* resolve_pool_base(const PoolId& pool_id,
                             AccessInfo* access = nullptr,
                             const AccessInfo* hint = nullptr);
  // the pool table of a v2 response, each pool resolved once
  std::vector<PoolRef> resolve_pools(const std::vector<PoolId>& ids);
  // routes a batch's transfers: fused copy list, SDMA streams or staging
  template <bool Put>
  struct Router;
  // the striped items of a batch that ride one fused_stripe launch
  struct StripeBatch;
  template <typename PtrOf, typename SizeOf>
  Result<std::vector<uint64_t>> digest_items(
      const std::vector<uint32_t>& indices, PtrOf ptr_of, SizeOf size_of,
      hipStream_t stream);
  // put epilogues shared by the v1 and v2 paths
  Result<void> complete_puts(
      const std::vector<DevPutItem>& items, const Router<true>& rt,
      size_t stride,
      std::map<uint32_t, std::vector<std::vector<uint64_t>>>* shard_digests,
      std::vector<int32_t>& statuses, bool apply_statuses);
  void cancel_failed(const std::vector<DevPutItem>& items,
                     const std::vector<int32_t>& statuses);
  Result<std::vector<int32_t>> batch_put_device_v2(
      const std::vector<DevPutItem>& items, const PlacementConfig& cfg,
      BatchPutSession* sess);
  // session fast paths; statuses when taken, nullopt → run the full path.
  // `striped_route`: the caller is the striped put path; a session of the
  // other form is left alone (the full path re-establishes it).
  std::optional<Result<std::vector<int32_t>>> try_session_put(
      const std::vector<DevPutItem>& items, BatchPutSession* sess,
      bool striped_route);
  std::optional<Result<std::vector<int32_t>>> try_session_get(
      const std::vector<DevGetItem>& items, BatchGetSession* sess);
  // a get step's stale hits: their keys leave the cache (which ends every
  // session on it), the get session ends, the items are refetched verified
  Result<std::vector<int32_t>> refetch_stale(
      const std::vector<DevGetItem>& items, const std::vector<uint32_t>& miss,
      BatchGetSession& sess);
  // what both put paths do with the placements they transferred: record
  // them and, with `bind`, hand the binding to `rebind` — or end the
  // session if the cache would not bind
  template <typename Rebind>
  void record_puts(const std::vector<PlacementCache::Put>& cached, bool bind,
                   uint64_t token, BatchPutSession* sess, Rebind rebind);
  Result<std::vector<int32_t>> batch_get_device_v2(
      const std::vector<DevGetItem>& items, bool verify,
      BatchGetSession* sess);
  // the RPC leg of the v2 get (cache misses route here)
  Result<std::vector<int32_t>> batch_get_device_rpc(
      const std::vector<DevGetItem>& items, bool verify);
  // items[idx] through the RPC leg, answers scattered into statuses
  Result<void> refetch(const std::vector<DevGetItem>& items,
                       const std::vector<uint32_t>& idx, bool verify,
                       std::vector<int32_t>& statuses);
  Result<void> staged_write(const ShardPlacement& s, const void* dev_src);
  Result<void> staged_write_buf(const ShardPlacement& s, const void* dev_src,
                                void* staging, uint64_t staging_size);
  // fan staged writes (direct-IO/TCP pools) out over pinned buffers
  Result<void> staged_write_many(
      const std::vector<std::pair<ShardPlacement, const void*>>& work);
  Result<void> staged_read(const ShardPlacement& s, void* dev_dst);
  Result<void> staged_read_buf(const ShardPlacement& s, void* dev_dst,
                               void* staging, uint64_t staging_size);
  // fan staged reads (host/TCP pools) out over a small pinned-buffer pool
  Result<void> staged_read_many(
      const std::vector<std::pair<ShardPlacement, void*>>& work);
  // reusable pinned staging buffers for the fan-out paths (hipHostMalloc is
  // milliseconds per call — allocating per batch dominated the NVMe legs)
  void* acquire_staging_buf();
  void release_staging_buf(void* p);

  Client& c_;
  int device_;
  std::mutex async_mu_;
  uint64_t next_async_ = 1;
  std::unordered_map<uint64_t, std::future<Result<std::vector<int32_t>>>>
      async_;
  static constexpr int kStreams = 7;  // one per xGMI link
  hipStream_t streams_[kStreams] = {};
  // dedicated streams for the staged fan-out threads (D2H pipelining that
  // never touches the batch streams or the legacy stream)
  hipStream_t fan_streams_[8] = {};
  void* staging_ = nullptr;  // pinned bounce buffer for TCP/SHM pools
  uint64_t staging_size_ = 64ull << 20;
  std::mutex staging_mu_;  // async batches share the bounce buffer
  static constexpr uint64_t kFanBuf = 16ull << 20;  // per-thread fan-out buf
  static constexpr int kFanThreads = 8;
  std::mutex staging_pool_mu_;
  std::vector<void*> staging_pool_;  // idle pinned kFanBuf buffers
  PlacementCache cache_;  // own lock; sessions hold Bindings into it
  std::atomic<uint64_t> session_put_steps_{0};
  std::atomic<uint64_t> session_get_steps_{0};
  std::atomic<uint64_t> session_graph_steps_{0};
  std::atomic<uint64_t> striped_fused_items_{0};
  std::atomic<uint64_t> striped_fused_get_items_{0};
  std::atomic<uint64_t> patched_fused_items_{0};
  std::atomic<uint64_t> patched_rewrite_items_{0};
  std::atomic<uint64_t> session_patch_steps_{0};
  // the rewrite route of one patch item (info: what the keystone holds)
  Result<void> patch_by_rewrite(const DevRangePatch& item,
                                const GetWorkersResponse& info);
  // One session step's launch, whichever form the session holds: the replay
  // of its captured graph when there is one, fused_put / fused_stripe
  // launches otherwise (builds the plan lazily; BB_NO_HIPGRAPH=1 or a failed
  // capture or replay pins the session to launches until it is rebound).
  struct StepDigests {
    std::vector<uint64_t> obj;  // one per kernel object (plain: per desc)
    std::vector<uint64_t> seg;  // one per segment; empty for the plain form
  };
  Result<StepDigests> session_step(SessionCore& sess, bool put);
  // The ladder under every session step, patch steps included: build `plan`
  // lazily (build(plan)), replay it (replay(plan), counted in
  // session_graph_steps), launch() otherwise; a failed build or replay sets
  // plan_failed, which keeps the session on launches.
  template <typename Plan, typename Build, typename Replay, typename Launch>
  Result<void> step_ladder(std::shared_ptr<Plan>& plan, bool& plan_failed,
                           const char* what, Build build, Replay replay,
                           Launch launch);
  // the patch session's step; nullopt → run the full path
  std::optional<Result<std::vector<int32_t>>> try_session_patch(
      const std::vector<DevRangePatch>& items, BatchPatchSession* sess);
  // The warm tail a copy+digest launch of this client asks for, decided here
  // for every path: a put leaves its budget's worth of the batch on-die,
  // and a get loads the same tail plainly (nontemporal loads of resident
  // lines measured slower with two lanes, profiles/warm_tail_checks.md).
  gpu::WarmTail warm_tail(bool put) const { return {warm_tail_bytes_, !put}; }
  // the body of the two async entry points
  template <typename Fn>
  Result<uint64_t> submit_async(Fn fn);
  bool fused_copy_ = true;
  uint64_t warm_tail_bytes_ = kDefaultWarmTailBytes;
  bool patch_edge_tiles_ = false;
  bool initialized_ = false;
};

}  // namespace blackbird
