// Keystone — the control plane: object metadata, put lifecycle, TTL GC,
// watermark eviction, worker/pool registries mirrored from coordination
// watchers, view versioning.
// Capability parity with reference KeystoneService (keystone_service.h:84-322,
// keystone_service.cpp:194-1004) with the same coordination key scheme
// (/blackbird/clusters/<cluster>/{workers,memory_pools,heartbeat}/...,
// keystone_service.cpp:590-604). Fresh design; also fixes reference defects:
// placement selection+reservation are atomic (no stale-used race), put_complete
// validates state, dead-worker cleanup drops the dead copies from object
// metadata instead of serving stale placements (§3.5 of SURVEY.md).
#pragma once

#include <atomic>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <unordered_map>
#include <thread>
#include <vector>

#include "blackbird/allocation/range_allocator.h"
#include "blackbird/common/result.h"
#include "blackbird/common/types.h"
#include "blackbird/coord/coord.h"
#include "blackbird/rpc/rpc.h"

namespace blackbird {

class KeystoneService {
 public:
  explicit KeystoneService(KeystoneConfig config,
                           std::shared_ptr<coord::CoordService> coord = nullptr);
  ~KeystoneService();

  Result<void> initialize();
  Result<void> start();
  void stop();
  // the RPC server reports its actually-bound endpoint here (listen_address
  // may use port 0); the service registry advertises this to clients
  void set_advertised_endpoint(const std::string& ep);

  // ------------------------------------------------------- object ops
  bool object_exists(const ObjectKey& key);
  Result<GetWorkersResponse> get_workers(const ObjectKey& key);
  Result<PutStartResponse> put_start(const ObjectKey& key, uint64_t size,
                                     const PlacementConfig& cfg);
  Result<void> put_complete(
      const ObjectKey& key, uint64_t checksum,
      const std::vector<std::vector<uint64_t>>& shard_digests = {});
  Result<void> put_cancel(const ObjectKey& key);
  Result<void> remove_object(const ObjectKey& key);
  uint64_t remove_all_objects();
  // Prefix scan over committed objects (operator tooling: `bbctl ls`).
  std::vector<ObjectSummary> list_objects(const std::string& prefix,
                                          uint32_t limit = 1000);

  // ------------------------------------------------------- batch ops
  BatchPutStartResponse batch_put_start(const std::vector<PutStartRequest>& reqs);
  std::vector<int32_t> batch_put_complete(const std::vector<PutCompleteRequest>& reqs);
  std::vector<int32_t> batch_put_cancel(const std::vector<ObjectKey>& keys);
  BatchGetWorkersResponse batch_get_workers(const std::vector<ObjectKey>& keys);
  std::vector<uint8_t> batch_object_exists(const std::vector<ObjectKey>& keys);
  std::vector<int32_t> batch_remove(const std::vector<ObjectKey>& keys);

  // ---- in-place range patches ----
  // BATCH_PATCH_START: every key that is COMMITTED, unexpired and has a
  // recorded checksum turns PENDING, which pins its placements exactly as an
  // in-place upsert does — but checksum and shard digests are KEPT: the
  // client moves them by the patched tiles' terms (gpu/patch_plan.h) and
  // commits through batch_put_complete / put_complete, which restarts the
  // TTL as for an upsert. The answer carries size, checksum and copies with
  // shard digests. Any other key gets a status (INVALID_STATE: no recorded
  // checksum) and keeps its state.
  BatchGetWorkersResponse batch_patch_start(const std::vector<ObjectKey>& keys);
  // BATCH_PATCH_ABORT, for a client that has written nothing: a key PENDING
  // from a patch start goes back to COMMITTED with checksum, digests and
  // clocks untouched; any other key gets INVALID_STATE. After a launch that
  // failed midway the bytes are torn and the route is put_cancel, which
  // removes the key — the contract of a failed in-place upsert.
  std::vector<int32_t> batch_patch_abort(const std::vector<ObjectKey>& keys);

  // ---- sessionful upserts (steady-state small-object fast path) ----
  // A put session pins an ordered key list server-side so repeat puts of the
  // same batch cost two tiny RPCs: upsert_start_token (flip every object to
  // PENDING, which pins placements against tiering/eviction) and
  // commit_token (record digests, flip back to COMMITTED). Any placement
  // change since session creation (remove / migration / scrub / repair /
  // worker death) bumps placement_epoch_ and the session fails with
  // SESSION_STALE — the client falls back to the full batch_put_start path.
  // No UCX analogue in the reference; its closest pattern is the batch RPC
  // loop at keystone_service.cpp:302-360.
  // Striped copies join only with allow_striped: the session then remembers
  // every object's shard shape and commits through commit_token_shards.
  // pending_only (BATCH_SESSION_OPEN): granted only if every object is
  // PENDING with the size the request names — a client opens its session
  // between BATCH_PUT_START and the commit, while PENDING pins the
  // placements it just resolved.
  uint64_t create_put_session(const std::vector<PutStartRequest>& reqs,
                              bool allow_striped = false,
                              bool pending_only = false);
  // BATCH_SESSION_OPEN: create_put_session(pending_only) behind the leader
  // check; token 0 = refused
  Result<uint64_t> open_session(const std::vector<PutStartRequest>& reqs,
                                bool allow_striped);
  Result<void> upsert_start_token(uint64_t token);
  // release=true erases the session after a successful commit (one-shot
  // token commits from cold batch puts — no key strings on the wire)
  Result<void> commit_token(uint64_t token, const std::vector<uint64_t>& digests,
                            bool release = false);
  // The same commit with every shard's own digest: shard_digests in object,
  // copy, shard order, one per shard the session held at creation. A wrong
  // count of either list is INVALID_ARGUMENT with nothing applied. Serves
  // single-shard sessions too (one digest per copy). commit_token refuses a
  // session holding a striped copy: it would stamp the object digest on
  // shard 0.
  Result<void> commit_token_shards(uint64_t token,
                                   const std::vector<uint64_t>& obj_digests,
                                   const std::vector<uint64_t>& shard_digests,
                                   bool release = false);
  uint64_t token_commits() const { return ctr_token_commits_.load(); }
  // BATCH_PATCH_START_TOKEN: batch_patch_start for the objects of a session
  // (opened while an earlier patch start held them PENDING), by token. All or
  // nothing: every object must be readable with a recorded checksum and
  // recorded shard digests, else INVALID_STATE and no object changes state —
  // a PENDING object too, unlike upsert_start_token: a patch step subtracts
  // old terms, which torn bytes no longer hold. On success every object is
  // PENDING with patch_started_ms set and its digests kept, and the answer is
  // what is recorded now — another writer's re-put in place included — in the
  // order commit_token_shards, the step's commit, takes the new ones.
  struct PatchStartDigests {
    std::vector<uint64_t> obj_digests;
    std::vector<uint64_t> shard_digests;  // object, copy, shard order
  };
  Result<PatchStartDigests> patch_start_token(uint64_t token);

  // ------------------------------------------------------ cluster view
  std::vector<WorkerInfo> get_workers_info();
  std::vector<MemoryPool> get_memory_pools();
  Result<void> remove_worker(const WorkerId& id);
  ClusterStats get_cluster_stats();
  uint64_t get_view_version() const { return view_version_.load(); }
  bool is_leader() const;

  // direct pool registration (single-process/embedded clusters and tests)
  void register_pool(const MemoryPool& pool);
  void register_worker(const WorkerInfo& info);

  const KeystoneConfig& config() const { return config_; }
  std::shared_ptr<coord::CoordService> coord() { return coord_; }

  // test hooks
  void run_gc_once();
  void run_eviction_once();

  // ---- tier migration (spill/promotion; BASELINE config #4) ----
  // One pass: demote cold objects out of overfull tiers, promote hot ones.
  void run_tiering_once();
  // Move `key`'s (single-copy) placement to `target` tier. Synchronous.
  Result<void> migrate_object(const ObjectKey& key, StorageClass target);

  // ---- failure repair: re-replicate objects that lost copies (the
  // reference served degraded objects forever) ----
  void run_repair_once();
  Result<void> repair_object(const ObjectKey& key);

  // ---- compaction: defragment a pool by re-packing its single-copy
  // objects (device-to-device moves through the migration machinery; the
  // reference had no compaction at all). Returns objects moved. ----
  Result<uint32_t> compact_pool(const PoolId& pool_id, uint32_t max_moves = 64);
  // Auto-compaction pass: compact every pool whose fragmentation exceeds
  // config.compact_fragmentation_threshold (no-op when the knob is 0).
  void run_compaction_once();
  // ---- digest scrubbing: re-checksum stored copies on their workers and
  // quarantine corrupt ones (dropped from metadata + ranges freed; the
  // repair pass restores replication). Single-shard copies only — the
  // digest is not combinable across shard boundaries. Returns the number
  // of corrupt copies quarantined. ----
  uint32_t run_scrub_once(uint32_t max_objects = 0);

  // ---- maintenance counters (monotonic, exported at /metrics) ----
  struct MaintenanceCounters {
    uint64_t migrations = 0;        // successful tier moves
    uint64_t repairs = 0;           // replicas restored
    uint64_t scrub_quarantined = 0; // corrupt copies dropped
    uint64_t evictions = 0;         // objects evicted over the watermark
    uint64_t gc_reclaimed = 0;      // TTL/abandoned objects collected
  };
  MaintenanceCounters counters() const {
    return {ctr_migrations_.load(), ctr_repairs_.load(),
            ctr_scrubbed_.load(), ctr_evictions_.load(), ctr_gc_.load()};
  }

 private:
  using ObjectMap = std::unordered_map<ObjectKey, ObjectMeta>;
  using DirtySet = std::map<ObjectKey, bool>;  // key → removed?

  void gc_loop();
  void keepalive_loop();
  void setup_watchers();
  void load_existing_state();
  void upsert_worker(WorkerInfo w);
  void handle_worker_event(const coord::WatchEvent& ev);
  void handle_pool_event(const coord::WatchEvent& ev);
  void handle_heartbeat_event(const coord::WatchEvent& ev);
  void cleanup_dead_worker(const WorkerId& id);
  void bump_view() { view_version_.fetch_add(1); }
  std::string prefix() const {
    return "/blackbird/clusters/" + config_.cluster_id;
  }

  // ---- object transitions; the *_locked ones need objects_mu_ held
  // exclusively ----
  // What an incoming put of `size` bytes under `cfg` does to the object at
  // `it` (objects_.end(): none yet).
  enum class Admission {
    EXISTS,    // refused: a live object and no cfg.replace
    IN_PLACE,  // same-shape upsert: flipped to PENDING, its placement stands
    REPLACE,   // the caller erases the object and places the key afresh
    FRESH,     // nothing there
  };
  Admission admit_locked(ObjectMap::iterator it, uint64_t size,
                         const PlacementConfig& cfg, uint64_t now);
  ObjectMeta pending_meta(const ObjectKey& key, uint64_t size,
                          const PlacementConfig& cfg, uint64_t now,
                          const std::vector<CopyPlacement>& copies) const;
  // drops the meta only; the ranges and the view are the caller's
  void erase_locked(ObjectMap::iterator it);
  // erase + range free + view bump
  Result<void> remove_object_locked(const ObjectKey& key);
  // the body of both get routes, under the SHARED lock: status, and on
  // success the touch and the answer
  ErrorCode read_locked(const ObjectKey& key, uint64_t now,
                        GetWorkersResponse& info);
  void remove_if_expired_locked(const ObjectKey& key, uint64_t now);

  // ---- maintenance (keystone_maintenance.cpp) ----
  // copy of a COMMITTED object's meta, taken under the exclusive lock
  Result<ObjectMeta> snapshot_committed(const ObjectKey& key);
  // One DATA_PULL per destination shard: each pulls its slice of the ordered
  // source shards. Stops at the first error.
  Result<void> pull_into(const std::vector<ShardPlacement>& dst_shards,
                         const std::vector<ShardPlacement>& src_shards);
  void persist_loop();
  void mark_dirty_locked(const ObjectKey& key, bool removed);
  DirtySet drain_dirty();
  // the coordination writes for `batch`; takes objects_mu_ exclusively
  void encode_dirty(const DirtySet& batch, std::vector<coord::KV>& puts,
                    std::vector<std::string>& dels);
  // drain the dirty set in one fenced coord round trip, re-queueing it on
  // failure (durability of commit/remove acks, and the persist loop's
  // step); call without objects_mu_ held
  void flush_dirty_now();

  KeystoneConfig config_;
  std::shared_ptr<coord::CoordService> coord_;
  RangeAllocator allocator_;

  std::shared_mutex objects_mu_;
  ObjectMap objects_;

  // ---- put sessions ----
  // metas are raw pointers into objects_ (unordered_map mapped values are
  // stable across insert/rehash); every objects_.erase or copies mutation
  // bumps placement_epoch_ under objects_mu_, so a session whose epoch no
  // longer matches is never dereferenced.
  struct PutSession {
    std::vector<ObjectMeta*> metas;
    std::vector<uint64_t> sizes;
    // shard shape at creation: shards[shard_begin[i] .. shard_begin[i+1]) are
    // the shard counts of object i's copies, in copy order
    std::vector<uint32_t> shards;
    std::vector<uint32_t> shard_begin;
    size_t total_shards = 0;
    bool striped = false;  // some copy has more than one shard
    uint64_t epoch = 0;
    uint64_t created_ms = 0;
  };
  uint64_t placement_epoch_ = 0;  // guarded by objects_mu_ (unique)
  void bump_placement_epoch_locked() { ++placement_epoch_; }
  std::shared_ptr<PutSession> find_session(uint64_t token);  // or null
  // epoch and sizes still match — and, for a session that holds a striped
  // copy, every object's copy count and shard counts; objects_mu_ held
  // (shared suffices)
  Result<void> session_current_locked(const PutSession& s) const;
  // the body of both token commits; commit_one(meta, index, now) applies one
  // object's transition
  template <typename CommitOne>
  Result<void> commit_session(uint64_t token, const PutSession& s, bool release,
                              CommitOne commit_one);
  std::mutex sessions_mu_;
  std::unordered_map<uint64_t, std::shared_ptr<PutSession>> put_sessions_;
  std::atomic<uint64_t> next_session_token_{1};
  std::atomic<uint64_t> ctr_token_commits_{0};

  std::shared_mutex workers_mu_;
  std::map<WorkerId, WorkerInfo> workers_;

  std::atomic<uint64_t> view_version_{0};
  std::atomic<bool> running_{false};
  // watch callbacks currently executing on coordination dispatcher threads;
  // stop() drains this so no callback can touch members during teardown
  std::atomic<int> cb_inflight_{0};
  std::mutex adv_mu_;
  std::string advertised_endpoint_;
  std::atomic<uint64_t> ctr_migrations_{0}, ctr_repairs_{0}, ctr_scrubbed_{0},
      ctr_evictions_{0}, ctr_gc_{0};
  std::thread gc_thread_;
  std::thread keepalive_thread_;
  std::thread persist_thread_;
  std::mutex dirty_mu_;
  DirtySet dirty_;
  std::condition_variable cv_;
  std::mutex cv_mu_;
  // Small pool of connections per worker endpoint: the RPC server is
  // thread-per-connection, so parallel migrations to one worker would
  // serialize on a single shared connection's handler thread.
  rpc::RpcClient* data_client(const std::string& endpoint);
  std::mutex data_clients_mu_;
  static constexpr int kDataConns = 4;
  struct DataConnPool {
    std::vector<std::unique_ptr<rpc::RpcClient>> conns;
    size_t cursor = 0;
  };
  std::map<std::string, DataConnPool> data_clients_;
  std::vector<uint64_t> watch_ids_;
  std::unique_ptr<coord::LeaderElector> elector_;
  std::string instance_id_;
};

}  // namespace blackbird
