// Client SDK: metadata RPC to Keystone + multi-path data plane.
// Capability parity with reference BlackbirdClient (blackbird_client.h:47-106,
// blackbird_client.cpp:87-351) — re-designed for the MI355X node:
//   * SHM pools   → one-sided memcpy into the worker's POSIX shared memory
//                   (host-tier analogue of UCX RMA),
//   * HIP_IPC     → one-sided hipMemcpy into the worker's HBM via
//                   hipIpcOpenMemHandle (the xGMI zero-copy fast path),
//   * TCP         → framed data protocol fallback (any pool, any host).
// Shard source offsets are tracked correctly per copy (the reference had a
// live bug here, blackbird_client.cpp:233). Transfers of one copy fan out
// over an IO thread pool; gets fail over across replicas.
#pragma once

#include <atomic>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>

#include "blackbird/common/result.h"
#include "blackbird/common/serde.h"
#include "blackbird/common/types.h"
#include "blackbird/rpc/rpc.h"

namespace blackbird {

namespace wire {
struct PatchStartDigests;  // batch_wire.h
}

struct ClientOptions {
  std::string keystone_endpoint = "127.0.0.1:9090";
  // Service discovery: when set (and keystone_endpoint is empty), the
  // client asks the coordination service for the registered keystone
  // (`/blackbird/services/blackbird-keystone/…` — the registry the
  // reference kept in etcd). Accepts a comma-separated coordd list.
  std::string coord_endpoint;
  std::string cluster_id = "default";
  int io_threads = 4;
  bool verify_checksum_on_get = false;  // digests verified on demand
  // patch() at byte granularity: a range that is not whole 1 KiB tiles is
  // patched in place too, its edge tiles composed of old and new bytes.
  // Off: such a range takes the rewrite route, which verifies the object.
  bool patch_edge_tiles = false;
  int rpc_timeout_ms = 30000;
  // diagnostics / transport comparison: skip the one-sided SHM/IPC fast
  // paths and go through the worker data plane (TCP) only
  bool force_tcp = false;
};

// Cached one-sided mappings (SHM segments, HIP-IPC handles) shared by client
// instances in a process.
class PoolMapper;

class Client {
 public:
  explicit Client(ClientOptions opts = {});
  ~Client();

  Result<void> connect();
  void close();

  // ------------------------------------------------------ object ops
  Result<void> put(const ObjectKey& key, const void* data, uint64_t size,
                   const PlacementConfig& cfg = {});
  Result<std::string> get(const ObjectKey& key);
  Result<uint64_t> get_into(const ObjectKey& key, void* dst, uint64_t capacity);
  // ---- ranged access ----
  // [offset, offset+length) of the object: the intersecting sub-ranges of the
  // first copy that reads completely, with replica failover as in get. Any
  // offset and length inside the object; a range that leaves it is
  // INVALID_ARGUMENT. UNVERIFIED, whatever verify_checksum_on_get says: the
  // recorded digests cover whole shards and whole objects, never a range.
  Result<std::string> get_range(const ObjectKey& key, uint64_t offset,
                                uint64_t length);
  // Overwrites [offset, offset+size) of a committed object in place, on
  // every copy, and moves the recorded object checksum and shard digests by
  // the patched tiles' terms alone (gpu/patch_plan.h): BATCH_PATCH_START,
  // read the old range, write the new one, BATCH_PUT_COMPLETE. Bytes outside
  // the range are neither read nor re-hashed, so corruption there stays
  // detectable. A range that is not made of whole 1 KiB tiles (but for one
  // that ends at the object's end), an object without recorded digests, or
  // a copy that cannot be patched shard by shard takes the rewrite route:
  // get the object, overlay the range, put it back with replace=true.
  // With ClientOptions::patch_edge_tiles the copy is planned with
  // gpu::plan_patch_bytes and any range is patched in place: per shard the
  // range is read ROUNDED OUT to whole tiles (clipped at the object's end),
  // the new tiles are composed of old and new bytes, the sums move by
  // checksum_cpu_tiles(new) − checksum_cpu_tiles(old) over the rounded range,
  // and only the new bytes are written. Unlike the rewrite route this does
  // not verify the object first: a corrupt byte stays, and stays detectable.
  // Replicas whose patched digests disagree: CHECKSUM_MISMATCH, nothing
  // written. A write that fails midway leaves torn bytes: the key is
  // cancelled (removed), as after a failed in-place upsert.
  Result<void> patch(const ObjectKey& key, uint64_t offset, const void* data,
                     uint64_t size);
  // the two keystone calls behind patch (GpuClient's ranged paths use them)
  Result<BatchGetWorkersResponse> patch_start(const std::vector<ObjectKey>& keys);
  void patch_abort(const std::vector<ObjectKey>& keys);  // best effort
  Result<bool> exists(const ObjectKey& key);
  Result<void> remove(const ObjectKey& key);
  Result<uint64_t> remove_all();
  Result<std::vector<int32_t>> batch_remove(const std::vector<ObjectKey>& keys);

  // ------------------------------------------------------- batch ops
  struct PutItem {
    ObjectKey key;
    const void* data;
    uint64_t size;
  };
  // Host-tier batch session (the DRAM twin of GpuClient's BatchPutSession).
  // Reference analogue: the repeated batch_put_start/put_complete cycle
  // (reference keystone_service.cpp:302-360) re-sent every key and
  // re-allocated every step; a session pins the placements server-side and
  // reduces the steady state to token-addressed commits.
  // callers re-putting the SAME batch (same keys/buffers/sizes, replace
  // mode) pay two tiny RPCs per step — upsert start, token+digest commit —
  // around direct memcpys into the mapped pool ranges. Established by the
  // first full batch_put when every copy resolved to a mapped host pool;
  // any server-side placement change invalidates it transparently.
  struct HostPutSession {
    uint64_t token = 0;
    uint32_t dsts_per_item = 1;       // one dst per copy
    std::vector<uint8_t*> dsts;        // items.size() * dsts_per_item
    std::vector<const void*> srcs;     // bound item buffers
    std::vector<uint64_t> sizes;
    void* owner = nullptr;
  };
  // One metadata RPC for the whole batch; per-item status out. A leader
  // failover mid-batch (put_start answered by the old leader, put_complete
  // by the new one that never saw the PENDING objects) is resumed
  // transparently: items that failed with failover-shaped errors WHILE a
  // reconnect happened are redone once against the new leader.
  Result<std::vector<int32_t>> batch_put(const std::vector<PutItem>& items,
                                         const PlacementConfig& cfg = {},
                                         HostPutSession* sess = nullptr);
  Result<std::vector<std::pair<int32_t, std::string>>> batch_get(
      const std::vector<ObjectKey>& keys);
  // bumped every time meta_call_raw re-established the leader connection
  uint64_t reconnect_generation() const { return reconnect_gen_.load(); }
  // status looks like a lost-leader symptom (worth one redo after failover)?
  static bool failover_retriable(int32_t st);
  // Run once(items, /*first=*/true); if the leader connection was
  // re-established meanwhile, run the failover-shaped per-item failures once
  // more through once(redo, false) and merge. The first answer is kept when
  // the redo fails as a whole. (A session belongs to the first attempt only:
  // the redo's item list is a different one.)
  template <typename Item, typename Once>
  auto redo_after_failover(const std::vector<Item>& items, Once&& once)
      -> decltype(once(items, true)) {
    const uint64_t gen = reconnect_generation();
    auto st = once(items, true);
    if (!st.ok() || reconnect_generation() == gen) return st;
    std::vector<Item> redo;
    std::vector<size_t> redo_idx;
    for (size_t i = 0; i < items.size(); ++i)
      if (failover_retriable(status_of(st.value()[i]))) {
        redo.push_back(items[i]);
        redo_idx.push_back(i);
      }
    if (redo.empty()) return st;
    auto st2 = once(redo, false);
    if (!st2.ok()) return st;
    for (size_t j = 0; j < redo_idx.size(); ++j)
      st.value()[redo_idx[j]] = std::move(st2.value()[j]);
    return st;
  }
  // ---- sessions over striped copies (GpuClient's striped fast path) ----
  // BATCH_SESSION_OPEN for objects this client holds PENDING (between its
  // BATCH_PUT_START and the commit): {key, size} pairs; token 0 = refused.
  Result<uint64_t> open_session(
      const std::vector<std::pair<ObjectKey, uint64_t>>& objects,
      bool allow_striped);
  // BATCH_COMMIT_TOKEN_SHARDS: n object digests and every shard's own, in
  // object, copy, shard order
  Result<void> commit_by_token_shards(uint64_t token, bool release,
                                      const uint64_t* obj_digests, size_t n,
                                      const uint64_t* shard_digests, size_t m);
  // BATCH_PATCH_START_TOKEN: a patch step of a session opened while a
  // patch_start held its objects PENDING. The objects turn PENDING again and
  // the answer is what the keystone records for them now, in the order of
  // commit_by_token_shards, the step's commit. Any error: nothing changed.
  Result<wire::PatchStartDigests> patch_start_token(uint64_t token);
  // steps served by the host session fast path (tests/bench introspection)
  uint64_t host_session_steps() const { return host_session_steps_.load(); }

  // ------------------------------------------------------ cluster view
  Result<ClusterStats> cluster_stats();
  Result<std::vector<MemoryPool>> memory_pools();
  Result<std::vector<WorkerInfo>> workers_info();
  Result<PingResponse> ping();
  Result<std::vector<ObjectSummary>> list_objects(
      const std::string& prefix = "", uint32_t limit = 1000);

  // ---- central metadata call with failover ----
  // Retries on connection loss (keystone restart) and on NOT_LEADER (HA
  // standby), re-discovering the current leader through the coordination
  // registry when coord_endpoint is configured. Bounded (~8 attempts with
  // short backoff); non-retryable errors surface immediately.
  Result<std::string> meta_call_raw(uint16_t method, const std::string& body,
                                    int timeout_ms = 0);
  template <typename Req, typename Resp>
  Result<Resp> meta_call(uint16_t method, const Req& req, int timeout_ms = 0) {
    auto raw = meta_call_raw(method, serde::to_bytes(req), timeout_ms);
    if (!raw.ok()) return raw.error();
    Resp out{};
    if (!serde::from_bytes(raw.value(), out))
      return Error{ErrorCode::PROTOCOL_ERROR, "bad response body"};
    return out;
  }

 private:
  friend class GpuClient;
  // Moves one shard between `user` and its pool over the first rung that
  // works: same-process pool (host memcpy, device copy, unmapped backend),
  // SHM mapping, HIP-IPC mapping, TCP. force_tcp goes straight to TCP.
  template <bool Write>
  Result<void> move_shard(const ShardPlacement& s,
                          std::conditional_t<Write, const void*, void*> user);
  Result<void> write_shard(const ShardPlacement& s, const void* src);
  Result<void> read_shard(const ShardPlacement& s, void* dst);
  // write every copy (first error aborts) / read the first copy that reads
  // completely (a copy that does not cover the object is skipped)
  Result<void> write_copies(const std::vector<CopyPlacement>& copies,
                            const void* data, uint64_t size);
  Result<void> read_copy(const std::vector<CopyPlacement>& copies, void* dst,
                         uint64_t size);
  // One shard of a force_tcp batch and where it sits in its item's buffer,
  // bucketed under the worker endpoint that serves it.
  struct EndpointShard {
    size_t item;
    const ShardPlacement* shard;
    uint64_t offset;
  };
  using EndpointBuckets = std::map<std::string, std::vector<EndpointShard>>;
  // false: a pool of `copy` is unknown, the batch cannot be grouped
  bool bucket_copy(size_t item, const CopyPlacement& copy,
                   EndpointBuckets& out);
  rpc::RpcClient* data_client(const std::string& endpoint);
  // Pool access cache: batch responses omit per-shard AccessInfo (the pool
  // table is fetched once and invalidated by view_version — the reference's
  // own cache-invalidation pattern, types.h:394-405).
  Result<AccessInfo> pool_access(const PoolId& id);
  void refresh_pool_cache_locked();

  static int32_t status_of(int32_t st) { return st; }
  static int32_t status_of(const std::pair<int32_t, std::string>& r) {
    return r.first;
  }
  // ---- put epilogues shared by the host and GPU paths (v1 and v2) ----
  // BATCH_COMMIT_TOKEN with digests[0], digests[stride], ... (n of them)
  Result<void> commit_by_token(uint64_t token, bool release,
                               const uint64_t* digests, size_t n,
                               size_t stride = 1);
  // BATCH_PUT_COMPLETE; reqs[j] belongs to item order[j]. Per-item commit
  // failures land in *statuses (nullptr: the caller ignores them).
  Result<void> complete_by_keys(const std::vector<PutCompleteRequest>& reqs,
                                const std::vector<uint32_t>& order,
                                std::vector<int32_t>* statuses);
  // BATCH_PUT_CANCEL (best effort; nothing is sent for an empty list)
  void cancel_puts(const std::vector<ObjectKey>& keys);
  // Epilogue of the host batch puts that commit by key: completes the items
  // whose status is 0 (with shard_digests_of(i) when one is given), writes
  // per-item commit failures back into statuses, then cancels the failed
  // items that cancellable(i) admits.
  Result<void> finish_puts(
      const std::vector<PutItem>& items, const std::vector<uint64_t>& digests,
      std::vector<int32_t>& statuses,
      const std::function<std::vector<std::vector<uint64_t>>(size_t)>&
          shard_digests_of,
      const std::function<bool(size_t)>& cancellable);

  ClientOptions opts_;
  rpc::RpcClient meta_;
  std::mutex data_mu_;
  std::map<std::string, std::unique_ptr<rpc::RpcClient>> data_clients_;
  std::shared_ptr<PoolMapper> mapper_;
  std::mutex pool_cache_mu_;
  std::map<PoolId, AccessInfo> pool_cache_;
  std::mutex reconnect_mu_;  // one thread rediscovers/reconnects at a time
  std::atomic<uint64_t> reconnect_gen_{0};
  std::atomic<uint64_t> host_session_steps_{0};
  Result<std::vector<int32_t>> batch_put_once(const std::vector<PutItem>& items,
                                              const PlacementConfig& cfg,
                                              HostPutSession* sess);
  // token fast path; nullopt -> run the full path (which re-establishes)
  std::optional<std::vector<int32_t>> try_host_session_put(
      const std::vector<PutItem>& items, HostPutSession* sess);
  Result<void> put_once(const ObjectKey& key, const void* data, uint64_t size,
                        const PlacementConfig& cfg);
  Result<std::vector<std::pair<int32_t, std::string>>> batch_get_once(
      const std::vector<ObjectKey>& keys);
  // compact v2 batch protocol (pool-table responses, fixed-width placements,
  // token commits) — the host-tier twin of GpuClient's v2 paths. Single-shard
  // placements only; *fallback signals "run the v1 path instead".
  Result<std::vector<int32_t>> batch_put_once_v2(
      const std::vector<PutItem>& items, const PlacementConfig& cfg,
      HostPutSession* sess);
  Result<std::vector<std::pair<int32_t, std::string>>> batch_get_once_v2(
      const std::vector<ObjectKey>& keys, bool* fallback);
  // host-visible base of a pool (same-process host pool or SHM mapping);
  // nullptr → per-shard write_shard/read_shard fallback
  uint8_t* host_pool_base(const PoolId& id, AccessInfo* access);
};

}  // namespace blackbird
