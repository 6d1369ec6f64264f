// Keystone service: lifecycle, the object state machine (admission, commit,
// reads, removal) behind the single and batch operations, put sessions, and
// the worker/pool registries fed by coordination watchers. Maintenance and
// persistence live in keystone_maintenance.cpp.
#include "blackbird/keystone/keystone_service.h"

#include <algorithm>
#include <atomic>
#include <random>
#include <thread>

#include "blackbird/common/log.h"
#include "keystone_internal.h"

namespace blackbird {

namespace {
std::string random_id() {
  static std::mt19937_64 rng(std::random_device{}());
  char buf[20];
  snprintf(buf, sizeof(buf), "%016llx", (unsigned long long)rng());
  return buf;
}
}  // namespace

KeystoneService::KeystoneService(KeystoneConfig config,
                                 std::shared_ptr<coord::CoordService> coord)
    : config_(std::move(config)), coord_(std::move(coord)),
      instance_id_("keystone-" + random_id()) {
  if (!coord_) coord_ = coord::make_coord(config_.coord_endpoint);
}

KeystoneService::~KeystoneService() { stop(); }

Result<void> KeystoneService::initialize() {
  if (!coord_) return Error{ErrorCode::COORD_UNAVAILABLE, "no coordination service"};
  return {};
}

Result<void> KeystoneService::start() {
  if (running_.exchange(true)) return {};
  if (auto* cc = dynamic_cast<coord::CoordClient*>(coord_.get())) {
    cc->set_on_reconnect([this] {
      if (!running_.load()) return;  // teardown already under way
      // the (in-memory) coordination server restarted: workers re-register
      // themselves; re-scan to pick their state up promptly
      BB_LOG(WARN) << "coordination restarted — rescanning cluster state";
      load_existing_state();
    });
  }
  load_existing_state();
  setup_watchers();
  if (config_.enable_ha) {
    elector_ = std::make_unique<coord::LeaderElector>(
        coord_, prefix() + "/leader", instance_id_, config_.worker_ttl_ms);
    elector_->set_on_elected([this] {
      if (!running_.load()) return;
      // a promoted standby's in-memory maps are stale: rescan workers,
      // pools and (with persist_objects) the persisted object map
      BB_LOG(WARN) << "promoted to keystone leader — rescanning state";
      load_existing_state();
    });
    elector_->start();
  }
  gc_thread_ = std::thread([this] { gc_loop(); });
  keepalive_thread_ = std::thread([this] { keepalive_loop(); });
  if (config_.persist_objects)
    persist_thread_ = std::thread([this] { persist_loop(); });
  BB_LOG(INFO) << "keystone started (cluster " << config_.cluster_id << ", "
               << instance_id_ << ")";
  return {};
}

void KeystoneService::stop() {
  if (!running_.exchange(false)) return;
  {
    std::lock_guard<std::mutex> g(cv_mu_);  // no lost wakeup on stop
  }
  cv_.notify_all();
  if (gc_thread_.joinable()) gc_thread_.join();
  if (keepalive_thread_.joinable()) keepalive_thread_.join();
  if (persist_thread_.joinable()) persist_thread_.join();
  if (elector_) elector_->stop();
  for (auto id : watch_ids_) coord_->unwatch(id);
  watch_ids_.clear();
  // a watch callback may still be mid-flight on the coordination client's
  // dispatcher thread (e.g. a heartbeat expiry sweeping thousands of dead
  // copies) — wait it out before the caller may destroy this object
  while (cb_inflight_.load() > 0)
    std::this_thread::sleep_for(std::chrono::milliseconds(1));
  coord_->del("/blackbird/services/blackbird-keystone/" + instance_id_);
}

bool KeystoneService::is_leader() const {
  return !elector_ || elector_->is_leader();
}

void KeystoneService::set_advertised_endpoint(const std::string& ep) {
  // adv_mu_ held ACROSS the registry write: otherwise the keepalive thread
  // can read the empty advertised endpoint, lose the race, and overwrite
  // the registry with the configured (possibly port-0) listen address
  std::lock_guard<std::mutex> g(adv_mu_);
  advertised_endpoint_ = ep;
  coord_->put("/blackbird/services/blackbird-keystone/" + instance_id_, ep,
              config_.worker_ttl_ms * 6);
}

void KeystoneService::keepalive_loop() {
  const std::string key = "/blackbird/services/blackbird-keystone/" + instance_id_;
  while (running_) {
    {
      std::lock_guard<std::mutex> g(adv_mu_);
      const std::string& ep = advertised_endpoint_.empty()
                                  ? config_.listen_address
                                  : advertised_endpoint_;
      coord_->put(key, ep, config_.worker_ttl_ms * 6);
    }
    std::unique_lock<std::mutex> lk(cv_mu_);
    cv_.wait_for(lk, std::chrono::milliseconds(config_.worker_ttl_ms * 3),
                 [this] { return !running_.load(); });
  }
}

// ------------------------------------------------- object state machine
//
// Concurrency: commits and reads run under the SHARED objects lock, from N
// ranks at once. The fields a commit mutates (state, checksum, shard
// digests, clocks, access count) therefore go through atomic_ref wherever
// the lock is not held exclusively; the placement STRUCTURE (strings,
// offsets, vector shapes) only changes under the exclusive lock, so plain
// reads of it are safe. Same-key concurrent commits are last-writer-wins,
// consistent with in-place data overwrites being racy by design.

namespace {

bool is_committed(const ObjectMeta& m) {
  return std::atomic_ref<ObjectState>(const_cast<ObjectState&>(m.state))
             .load(std::memory_order_acquire) == ObjectState::COMMITTED;
}

// Whether `m` (nullptr: no such object) can be read at `now`: OK, or why not.
ErrorCode readable(const ObjectMeta* m, uint64_t now) {
  if (!m) return ErrorCode::OBJECT_NOT_FOUND;
  if (!is_committed(*m)) return ErrorCode::OBJECT_NOT_COMMITTED;
  if (m->ttl_ms > 0 && now > rload(m->created_ms) + m->ttl_ms)
    return ErrorCode::OBJECT_EXPIRED;
  return ErrorCode::OK;
}

// A structural copy of the placements, but for the digest slots, which a
// concurrent commit may be storing to.
void fill_info(GetWorkersResponse& info, const ObjectMeta& meta) {
  info.size = meta.size;
  info.checksum = rload(meta.checksum);
  info.copies.reserve(meta.copies.size());
  for (const auto& c : meta.copies) {
    CopyPlacement cp;
    cp.copy_index = c.copy_index;
    cp.shards.reserve(c.shards.size());
    for (const auto& sh : c.shards) {
      ShardPlacement sp;
      sp.pool_id = sh.pool_id;
      sp.worker_id = sh.worker_id;
      sp.storage_class = sh.storage_class;
      sp.offset = sh.offset;
      sp.length = sh.length;
      sp.digest = rload(sh.digest);
      sp.access = sh.access;
      cp.shards.push_back(std::move(sp));
    }
    info.copies.push_back(std::move(cp));
  }
}

// The commit itself, once the digests are in: checksum and clocks (the TTL
// starts at commit), then the release store that publishes them.
inline void publish_commit(ObjectMeta& m, uint64_t checksum, uint64_t now) {
  rstore(m.checksum, checksum);
  rstore(m.created_ms, now);
  rstore(m.last_access_ms, now);
  if (rload(m.patch_started_ms) != 0) rstore(m.patch_started_ms, uint64_t{0});
  std::atomic_ref<ObjectState>(m.state).store(ObjectState::COMMITTED, std::memory_order_release);
}

// Commit `m` with per-copy, per-shard digests. A copy whose digest list has
// the wrong shape keeps its digests, except that a single-shard copy takes
// the whole-object checksum (its shard IS the object).
void commit_meta(ObjectMeta& m, uint64_t checksum,
                 const std::vector<std::vector<uint64_t>>& sd, uint64_t now) {
  for (size_t c = 0; c < m.copies.size(); ++c) {
    auto& shards = m.copies[c].shards;
    if (c < sd.size() && sd[c].size() == shards.size()) {
      for (size_t s = 0; s < shards.size(); ++s)
        rstore(shards[s].digest, sd[c][s]);
    } else if (shards.size() == 1) {
      rstore(shards[0].digest, checksum);
    }
  }
  publish_commit(m, checksum, now);
}

// Single-shard form for session commits (copies are single-shard by
// construction): every replica holds the same bytes, so the same digest.
inline void commit_meta(ObjectMeta& m, uint64_t digest, uint64_t now) {
  for (auto& c : m.copies) rstore(c.shards[0].digest, digest);
  publish_commit(m, digest, now);
}

// A commit of an already COMMITTED object is a retry (the first attempt
// applied, e.g. before a leader failover, and its reply was lost) when it
// carries the same checksum: success, not INVALID_STATE.
ErrorCode recommit_status(const ObjectMeta& m, uint64_t checksum) {
  return rload(m.checksum) == checksum ? ErrorCode::OK
                                       : ErrorCode::INVALID_STATE;
}

}  // namespace

KeystoneService::Admission KeystoneService::admit_locked(
    ObjectMap::iterator it, uint64_t size, const PlacementConfig& cfg,
    uint64_t now) {
  if (it == objects_.end()) return Admission::FRESH;
  ObjectMeta& m = it->second;
  if (!m.expired(now) && !cfg.replace) return Admission::EXISTS;
  if (cfg.replace && m.state == ObjectState::COMMITTED && m.size == size &&
      m.copies.size() == std::max<uint32_t>(cfg.replication, 1)) {
    // same-size upsert: overwrite IN PLACE — no allocator free/alloc,
    // placements (and client placement caches) stay stable
    m.state = ObjectState::PENDING;
    m.checksum = 0;
    return Admission::IN_PLACE;
  }
  return Admission::REPLACE;  // size/shape changed, or expired
}

ObjectMeta KeystoneService::pending_meta(
    const ObjectKey& key, uint64_t size, const PlacementConfig& cfg,
    uint64_t now, const std::vector<CopyPlacement>& copies) const {
  ObjectMeta meta;
  meta.key = key;
  meta.size = size;
  meta.ttl_ms = cfg.ttl_ms ? cfg.ttl_ms : config_.object_ttl_default_ms;
  meta.created_ms = now;
  meta.last_access_ms = now;
  meta.state = ObjectState::PENDING;
  meta.replication = std::max<uint32_t>(cfg.replication, 1);
  meta.copies = copies;
  return meta;
}

void KeystoneService::erase_locked(ObjectMap::iterator it) {
  mark_dirty_locked(it->first, true);
  objects_.erase(it);
  bump_placement_epoch_locked();  // session meta pointers may now dangle
}

Result<void> KeystoneService::remove_object_locked(const ObjectKey& key) {
  allocator_.free(key);
  auto it = objects_.find(key);
  if (it != objects_.end()) erase_locked(it);
  bump_view();
  return {};
}

ErrorCode KeystoneService::read_locked(const ObjectKey& key, uint64_t now,
                                       GetWorkersResponse& info) {
  auto it = objects_.find(key);
  ObjectMeta* meta = it == objects_.end() ? nullptr : &it->second;
  const ErrorCode status = readable(meta, now);
  if (status != ErrorCode::OK) return status;
  rstore(meta->last_access_ms, now);
  std::atomic_ref<uint32_t>(meta->access_count)
      .fetch_add(1, std::memory_order_relaxed);
  fill_info(info, *meta);
  return status;
}

void KeystoneService::remove_if_expired_locked(const ObjectKey& key,
                                               uint64_t now) {
  auto it = objects_.find(key);
  if (it != objects_.end() && it->second.expired(now))
    remove_object_locked(key);
}

// ------------------------------------------------------------- object ops

bool KeystoneService::object_exists(const ObjectKey& key) {
  std::shared_lock lk(objects_mu_);
  auto it = objects_.find(key);
  return it != objects_.end() &&
         readable(&it->second, now_ms()) == ErrorCode::OK;
}

Result<GetWorkersResponse> KeystoneService::get_workers(const ObjectKey& key) {
  // the one-key form of batch_get_workers
  GetWorkersResponse resp;
  const uint64_t now = now_ms();
  ErrorCode status;
  {
    std::shared_lock lk(objects_mu_);
    status = read_locked(key, now, resp);
  }
  if (status == ErrorCode::OBJECT_EXPIRED) {
    std::unique_lock lk(objects_mu_);
    remove_if_expired_locked(key, now);
  }
  if (status != ErrorCode::OK) return Error{status, key};
  return resp;
}

Result<PutStartResponse> KeystoneService::put_start(const ObjectKey& key,
                                                    uint64_t size,
                                                    const PlacementConfig& cfg) {
  if (!is_leader()) return not_leader();
  if (key.empty()) return Error{ErrorCode::INVALID_ARGUMENT, "empty key"};
  if (size == 0) return Error{ErrorCode::INVALID_ARGUMENT, "zero-size object"};
  std::unique_lock lk(objects_mu_);
  PutStartResponse resp;
  auto it = objects_.find(key);
  switch (admit_locked(it, size, cfg, now_ms())) {
    case Admission::EXISTS:
      return Error{ErrorCode::OBJECT_EXISTS, key};
    case Admission::IN_PLACE:
      resp.copies = it->second.copies;
      resp.view_version = view_version_.load();
      return resp;
    case Admission::REPLACE:
      remove_object_locked(key);
      break;
    case Admission::FRESH:
      break;
  }
  auto placed = allocator_.allocate(key, size, cfg);
  if (!placed.ok()) return placed.error();
  objects_[key] = pending_meta(key, size, cfg, now_ms(), placed.value());
  bump_view();
  resp.copies = std::move(placed.value());
  resp.view_version = view_version_.load();
  return resp;
}

Result<void> KeystoneService::put_complete(
    const ObjectKey& key, uint64_t checksum,
    const std::vector<std::vector<uint64_t>>& shard_digests) {
  std::unique_lock lk(objects_mu_);
  auto it = objects_.find(key);
  if (it == objects_.end()) return Error{ErrorCode::OBJECT_NOT_FOUND, key};
  if (is_committed(it->second)) {
    if (recommit_status(it->second, checksum) == ErrorCode::OK) return {};
    return Error{ErrorCode::INVALID_STATE, "already committed: " + key};
  }
  commit_meta(it->second, checksum, shard_digests, now_ms());
  mark_dirty_locked(key, false);
  bump_view();
  lk.unlock();
  flush_dirty_now();
  return {};
}

Result<void> KeystoneService::put_cancel(const ObjectKey& key) {
  std::unique_lock lk(objects_mu_);
  auto it = objects_.find(key);
  if (it == objects_.end()) return Error{ErrorCode::OBJECT_NOT_FOUND, key};
  if (it->second.state == ObjectState::COMMITTED)
    return Error{ErrorCode::INVALID_STATE, "committed; use remove_object"};
  return remove_object_locked(key);
}

Result<void> KeystoneService::remove_object(const ObjectKey& key) {
  if (!is_leader()) return not_leader();
  std::unique_lock lk(objects_mu_);
  if (!objects_.count(key)) return Error{ErrorCode::OBJECT_NOT_FOUND, key};
  return remove_object_locked(key);
}

std::vector<ObjectSummary> KeystoneService::list_objects(
    const std::string& prefix, uint32_t limit) {
  std::vector<ObjectSummary> out;
  const uint64_t now = now_ms();
  std::shared_lock lk(objects_mu_);
  for (const auto& [key, meta] : objects_) {
    if (out.size() >= limit) break;
    if (readable(&meta, now) != ErrorCode::OK) continue;
    if (!prefix.empty() && key.rfind(prefix, 0) != 0) continue;
    ObjectSummary s;
    s.key = key;
    s.size = meta.size;
    s.ncopies = static_cast<uint32_t>(meta.copies.size());
    if (!meta.copies.empty() && !meta.copies[0].shards.empty())
      s.storage_class = meta.copies[0].shards[0].storage_class;
    out.push_back(std::move(s));
  }
  std::sort(out.begin(), out.end(),
            [](const ObjectSummary& a, const ObjectSummary& b) {
              return a.key < b.key;
            });
  return out;
}

uint64_t KeystoneService::remove_all_objects() {
  std::unique_lock lk(objects_mu_);
  uint64_t n = objects_.size();
  for (auto& [key, meta] : objects_) allocator_.free(key);
  objects_.clear();
  bump_placement_epoch_locked();
  bump_view();
  return n;
}

// ------------------------------------------------------------- batch ops

BatchPutStartResponse KeystoneService::batch_put_start(
    const std::vector<PutStartRequest>& reqs) {
  BatchPutStartResponse out;
  out.items.resize(reqs.size());
  if (!is_leader()) {
    for (auto& it : out.items)
      it.status = static_cast<int32_t>(ErrorCode::NOT_LEADER);
    out.view_version = view_version_.load();
    return out;
  }
  if (reqs.empty()) {
    out.view_version = view_version_.load();
    return out;
  }
  // uniform-config fast path: one objects lock + one allocator batch call
  bool uniform = true;
  for (size_t i = 1; i < reqs.size(); ++i) {
    const auto& a = reqs[i].config;
    const auto& b = reqs[0].config;
    if (a.replication != b.replication ||
        a.max_workers_per_copy != b.max_workers_per_copy ||
        a.preferred_class != b.preferred_class ||
        a.required_class != b.required_class || a.ttl_ms != b.ttl_ms) {
      uniform = false;
      break;
    }
  }
  if (!uniform) {
    for (size_t i = 0; i < reqs.size(); ++i) {
      auto res = put_start(reqs[i].key, reqs[i].size, reqs[i].config);
      if (res.ok()) out.items[i].copies = std::move(res.value().copies);
      else out.items[i].status = static_cast<int32_t>(res.code());
    }
    out.view_version = view_version_.load();
    return out;
  }

  // Lock discipline for scale-out (8 ranks hammer this concurrently): the
  // objects lock is held only for the map passes, never across allocation.
  // keys/sizes stay index-aligned with reqs; an item that is refused or
  // upserted in place leaves an empty slot the allocator skips, and
  // place[i] says whether item i is (still) being placed.
  const size_t n = reqs.size();
  std::vector<ObjectKey> keys(n);
  std::vector<uint64_t> sizes(n, 0);
  std::vector<uint8_t> place(n, 0);
  std::vector<const ObjectKey*> replaced;  // freed OUTSIDE the objects lock
  const uint64_t now = now_ms();
  {
    std::unique_lock lk(objects_mu_);
    for (size_t i = 0; i < n; ++i) {
      const auto& r = reqs[i];
      if (r.key.empty()) {
        out.items[i].status = static_cast<int32_t>(ErrorCode::INVALID_ARGUMENT);
        continue;
      }
      auto it = objects_.find(r.key);
      switch (admit_locked(it, r.size, r.config, now)) {
        case Admission::EXISTS:
          out.items[i].status = static_cast<int32_t>(ErrorCode::OBJECT_EXISTS);
          continue;
        case Admission::IN_PLACE:
          out.items[i].copies = it->second.copies;
          continue;
        case Admission::REPLACE:
          // drop the meta here, free the ranges in one allocator batch
          // below (not per key under this lock)
          erase_locked(it);
          replaced.push_back(&r.key);
          break;
        case Admission::FRESH:
          break;
      }
      place[i] = 1;
      keys[i] = r.key;
      sizes[i] = r.size;
    }
    if (!replaced.empty()) bump_view();
  }
  if (!replaced.empty()) allocator_.free_batch(replaced);
  // allocator has its own lock; two racing batches over the same fresh key
  // are serialized by the allocator's ledger (second gets OBJECT_EXISTS)
  auto placed = allocator_.allocate_batch(keys, sizes, reqs[0].config);
  // build metadata outside any lock
  std::vector<ObjectMeta> metas(n);
  for (size_t i = 0; i < n; ++i) {
    if (!place[i]) continue;
    if (placed[i].first != 0) {
      out.items[i].status = placed[i].first;
      place[i] = 0;
      continue;
    }
    metas[i] = pending_meta(reqs[i].key, reqs[i].size, reqs[i].config, now,
                            placed[i].second);
  }
  {
    std::unique_lock lk(objects_mu_);
    objects_.reserve(objects_.size() + n);  // no mid-batch rehash
    for (size_t i = 0; i < n; ++i) {
      if (!place[i]) continue;
      auto [it, inserted] = objects_.try_emplace(reqs[i].key);
      if (!inserted) {
        // raced with a concurrent put of the same key: release our ranges
        out.items[i].status = static_cast<int32_t>(ErrorCode::OBJECT_EXISTS);
        lk.unlock();
        allocator_.free(reqs[i].key);
        lk.lock();
        continue;
      }
      it->second = std::move(metas[i]);
      out.items[i].copies = std::move(placed[i].second);
    }
    bump_view();
  }
  out.view_version = view_version_.load();
  return out;
}

std::vector<int32_t> KeystoneService::batch_put_complete(
    const std::vector<PutCompleteRequest>& reqs) {
  // one SHARED lock + one view bump for the whole batch: commit batches
  // from N ranks run concurrently
  std::vector<int32_t> out(reqs.size(), 0);
  const uint64_t now = now_ms();
  bool any = false;
  {
    std::shared_lock lk(objects_mu_);
    for (size_t i = 0; i < reqs.size(); ++i) {
      auto it = objects_.find(reqs[i].key);
      if (it == objects_.end()) {
        out[i] = static_cast<int32_t>(ErrorCode::OBJECT_NOT_FOUND);
        continue;
      }
      ObjectMeta& m = it->second;
      if (is_committed(m)) {
        out[i] = static_cast<int32_t>(recommit_status(m, reqs[i].checksum));
        continue;
      }
      commit_meta(m, reqs[i].checksum, reqs[i].shard_digests, now);
      mark_dirty_locked(reqs[i].key, false);
      any = true;
    }
    if (any) bump_view();
  }
  flush_dirty_now();
  return out;
}

std::vector<int32_t> KeystoneService::batch_put_cancel(
    const std::vector<ObjectKey>& keys) {
  std::vector<int32_t> out;
  out.reserve(keys.size());
  for (const auto& k : keys)
    out.push_back(static_cast<int32_t>(put_cancel(k).code()));
  return out;
}

BatchGetWorkersResponse KeystoneService::batch_get_workers(
    const std::vector<ObjectKey>& keys) {
  // SHARED lock: get batches from N ranks run concurrently with each other
  // and with session commits. Expired objects are collected and removed in
  // a rare second exclusive pass.
  BatchGetWorkersResponse out;
  out.items.resize(keys.size());
  const uint64_t now = now_ms();
  std::vector<size_t> expired_idx;
  {
    std::shared_lock lk(objects_mu_);
    for (size_t i = 0; i < keys.size(); ++i) {
      auto& item = out.items[i];
      const ErrorCode status = read_locked(keys[i], now, item.info);
      item.status = static_cast<int32_t>(status);
      if (status == ErrorCode::OBJECT_EXPIRED) expired_idx.push_back(i);
    }
  }
  if (!expired_idx.empty()) {
    std::unique_lock lk(objects_mu_);
    for (size_t i : expired_idx) remove_if_expired_locked(keys[i], now);
  }
  return out;
}

std::vector<uint8_t> KeystoneService::batch_object_exists(
    const std::vector<ObjectKey>& keys) {
  std::vector<uint8_t> out;
  out.reserve(keys.size());
  for (const auto& k : keys) out.push_back(object_exists(k) ? 1 : 0);
  return out;
}

std::vector<int32_t> KeystoneService::batch_remove(
    const std::vector<ObjectKey>& keys) {
  std::vector<int32_t> out(keys.size(), 0);
  std::vector<const ObjectKey*> to_free;
  to_free.reserve(keys.size());
  {
    std::unique_lock lk(objects_mu_);
    for (size_t i = 0; i < keys.size(); ++i) {
      auto it = objects_.find(keys[i]);
      if (it == objects_.end()) {
        out[i] = static_cast<int32_t>(ErrorCode::OBJECT_NOT_FOUND);
        continue;
      }
      erase_locked(it);
      to_free.push_back(&keys[i]);
    }
    bump_view();
  }
  // range frees take only the allocator's own lock — once for the batch
  allocator_.free_batch(to_free);
  flush_dirty_now();  // deletions durable before the reply (retry-safe)
  return out;
}

// ------------------------------------------------- in-place range patches

BatchGetWorkersResponse KeystoneService::batch_patch_start(
    const std::vector<ObjectKey>& keys) {
  BatchGetWorkersResponse out;
  out.items.resize(keys.size());
  if (!is_leader()) {
    for (auto& it : out.items)
      it.status = static_cast<int32_t>(ErrorCode::NOT_LEADER);
    return out;
  }
  const uint64_t now = now_ms();
  // exclusive, as every COMMITTED -> PENDING flip (admit_locked)
  std::unique_lock lk(objects_mu_);
  for (size_t i = 0; i < keys.size(); ++i) {
    auto& item = out.items[i];
    auto it = objects_.find(keys[i]);
    ObjectMeta* m = it == objects_.end() ? nullptr : &it->second;
    ErrorCode status = readable(m, now);
    if (status == ErrorCode::OK && m->checksum == 0)
      status = ErrorCode::INVALID_STATE;  // nothing to move
    item.status = static_cast<int32_t>(status);
    if (status == ErrorCode::OBJECT_EXPIRED) remove_object_locked(keys[i]);
    if (status != ErrorCode::OK) continue;
    fill_info(item.info, *m);
    m->patch_started_ms = now ? now : 1;
    m->state = ObjectState::PENDING;
  }
  return out;
}

std::vector<int32_t> KeystoneService::batch_patch_abort(
    const std::vector<ObjectKey>& keys) {
  std::vector<int32_t> out(keys.size(), 0);
  if (!is_leader()) {
    out.assign(keys.size(), static_cast<int32_t>(ErrorCode::NOT_LEADER));
    return out;
  }
  std::unique_lock lk(objects_mu_);
  for (size_t i = 0; i < keys.size(); ++i) {
    auto it = objects_.find(keys[i]);
    if (it == objects_.end()) {
      out[i] = static_cast<int32_t>(ErrorCode::OBJECT_NOT_FOUND);
      continue;
    }
    ObjectMeta& m = it->second;
    if (m.state != ObjectState::PENDING || m.patch_started_ms == 0) {
      out[i] = static_cast<int32_t>(ErrorCode::INVALID_STATE);
      continue;
    }
    m.patch_started_ms = 0;
    m.state = ObjectState::COMMITTED;
  }
  return out;
}

// ------------------------------------------------- sessionful upserts

uint64_t KeystoneService::create_put_session(
    const std::vector<PutStartRequest>& reqs, bool allow_striped,
    bool pending_only) {
  if (reqs.empty()) return 0;
  auto s = std::make_shared<PutSession>();
  s->metas.reserve(reqs.size());
  s->sizes.reserve(reqs.size());
  s->shard_begin.reserve(reqs.size() + 1);
  s->created_ms = now_ms();
  {
    std::shared_lock lk(objects_mu_);
    for (const auto& r : reqs) {
      auto it = objects_.find(r.key);
      if (it == objects_.end() || it->second.copies.empty())
        return 0;
      const ObjectMeta& m = it->second;
      if (pending_only &&
          (m.size != r.size || rload(m.state) != ObjectState::PENDING))
        return 0;
      // without allow_striped sessions cover single-SHARD copies (any
      // replica count): commit_token records ONE digest per object — every
      // replica holds the same bytes — and the client resolves one
      // destination per copy
      s->shard_begin.push_back(static_cast<uint32_t>(s->shards.size()));
      for (const auto& c : m.copies) {
        if (c.shards.empty()) return 0;
        if (c.shards.size() != 1) {
          if (!allow_striped) return 0;
          s->striped = true;
        }
        s->shards.push_back(static_cast<uint32_t>(c.shards.size()));
        s->total_shards += c.shards.size();
      }
      s->metas.push_back(&it->second);
      s->sizes.push_back(m.size);
    }
    s->shard_begin.push_back(static_cast<uint32_t>(s->shards.size()));
    s->epoch = placement_epoch_;
  }
  uint64_t token = next_session_token_.fetch_add(1);
  std::lock_guard<std::mutex> g(sessions_mu_);
  put_sessions_[token] = std::move(s);
  if (put_sessions_.size() > 1024) {
    // cap the table: evict the oldest session (tokens are monotonic)
    auto oldest = put_sessions_.begin();
    for (auto it = put_sessions_.begin(); it != put_sessions_.end(); ++it)
      if (it->first < oldest->first) oldest = it;
    put_sessions_.erase(oldest);
  }
  return token;
}

Result<uint64_t> KeystoneService::open_session(
    const std::vector<PutStartRequest>& reqs, bool allow_striped) {
  if (!is_leader()) return not_leader();
  return create_put_session(reqs, allow_striped, /*pending_only=*/true);
}

std::shared_ptr<KeystoneService::PutSession> KeystoneService::find_session(
    uint64_t token) {
  std::lock_guard<std::mutex> g(sessions_mu_);
  auto it = put_sessions_.find(token);
  return it == put_sessions_.end() ? nullptr : it->second;
}

// Removal/GC/eviction hold objects_mu_ exclusively and bump the epoch, so a
// session that passes this check under the (shared) lock can dereference
// its meta pointers for as long as it keeps the lock.
Result<void> KeystoneService::session_current_locked(
    const PutSession& s) const {
  if (s.epoch != placement_epoch_)
    return Error{ErrorCode::SESSION_STALE, "placements changed"};
  for (size_t i = 0; i < s.metas.size(); ++i)
    if (s.metas[i]->size != s.sizes[i])
      return Error{ErrorCode::SESSION_STALE, "object shape changed"};
  // The shard shape sits in other cache lines of the object than its size
  // (the copies vector, and the shard counts behind its heap array), read on
  // both calls of every step: measured 2–4 % of a 4096 × 64 KiB single-shard
  // session step. Only a session that holds a striped copy pays for it — its
  // commit regroups a flat digest list by the remembered shape. An
  // all-single-shard session stamps shard 0 of each copy, as it did before
  // sessions could be striped.
  if (!s.striped) return {};
  for (size_t i = 0; i < s.metas.size(); ++i) {
    const ObjectMeta& m = *s.metas[i];
    const uint32_t* shape = s.shards.data() + s.shard_begin[i];
    bool same = m.copies.size() == s.shard_begin[i + 1] - s.shard_begin[i];
    for (size_t c = 0; same && c < m.copies.size(); ++c)
      same = m.copies[c].shards.size() == shape[c];
    if (!same) return Error{ErrorCode::SESSION_STALE, "object shape changed"};
  }
  return {};
}

Result<void> KeystoneService::upsert_start_token(uint64_t token) {
  if (!is_leader()) return not_leader();
  auto s = find_session(token);
  if (!s) return Error{ErrorCode::SESSION_STALE, "unknown put session"};
  // SHARED lock: session steps from N ranks run concurrently (the warm
  // plane would otherwise convoy on one mutex at 8 ranks × 2 lanes)
  std::shared_lock lk(objects_mu_);
  // validate ALL before flipping ANY (all-or-nothing). An object that is
  // still PENDING is fine: a client that died between start and commit may
  // retry the same session
  BB_RETURN_IF_ERROR(session_current_locked(*s));
  // PENDING pins the placements: tiering/eviction/repair/scrub only touch
  // COMMITTED objects, so the client's one-sided writes land in ranges that
  // cannot move underneath them
  for (auto* m : s->metas) rstore(m->state, ObjectState::PENDING);
  return {};
}

Result<KeystoneService::PatchStartDigests> KeystoneService::patch_start_token(
    uint64_t token) {
  if (!is_leader()) return not_leader();
  auto s = find_session(token);
  if (!s) return Error{ErrorCode::SESSION_STALE, "unknown put session"};
  const uint64_t now = now_ms();
  // exclusive, as batch_patch_start: two starts that share a key must not
  // both find it COMMITTED
  std::unique_lock lk(objects_mu_);
  BB_RETURN_IF_ERROR(session_current_locked(*s));
  PatchStartDigests out;
  out.obj_digests.reserve(s->metas.size());
  out.shard_digests.reserve(s->total_shards);
  // validate ALL before flipping ANY
  for (const ObjectMeta* m : s->metas) {
    if (readable(m, now) != ErrorCode::OK)
      return Error{ErrorCode::INVALID_STATE, "not readable: " + m->key};
    if (m->checksum == 0)
      return Error{ErrorCode::INVALID_STATE, "no recorded checksum: " + m->key};
    out.obj_digests.push_back(m->checksum);
    for (const auto& c : m->copies)
      for (const auto& sh : c.shards) {
        if (sh.digest == 0)
          return Error{ErrorCode::INVALID_STATE,
                       "no recorded shard digest: " + m->key};
        out.shard_digests.push_back(sh.digest);
      }
  }
  // a single-shard session never had its shape compared (see
  // session_current_locked); the count is what the commit will be held to
  if (out.shard_digests.size() != s->total_shards)
    return Error{ErrorCode::SESSION_STALE, "object shape changed"};
  for (ObjectMeta* m : s->metas) {
    m->patch_started_ms = now ? now : 1;
    m->state = ObjectState::PENDING;
  }
  return out;
}

Result<void> KeystoneService::commit_token(
    uint64_t token, const std::vector<uint64_t>& digests, bool release) {
  if (!is_leader()) return not_leader();
  auto s = find_session(token);
  if (!s) return Error{ErrorCode::SESSION_STALE, "unknown put session"};
  if (digests.size() != s->metas.size())
    return Error{ErrorCode::INVALID_ARGUMENT, "digest count mismatch"};
  if (s->striped)
    return Error{ErrorCode::INVALID_ARGUMENT,
                 "striped session commits with shard digests"};
  return commit_session(token, *s, release, [&](ObjectMeta& m, size_t i,
                                                uint64_t now) {
    commit_meta(m, digests[i], now);
  });
}

Result<void> KeystoneService::commit_token_shards(
    uint64_t token, const std::vector<uint64_t>& obj_digests,
    const std::vector<uint64_t>& shard_digests, bool release) {
  if (!is_leader()) return not_leader();
  auto s = find_session(token);
  if (!s) return Error{ErrorCode::SESSION_STALE, "unknown put session"};
  if (obj_digests.size() != s->metas.size())
    return Error{ErrorCode::INVALID_ARGUMENT, "digest count mismatch"};
  if (shard_digests.size() != s->total_shards)
    return Error{ErrorCode::INVALID_ARGUMENT, "shard digest count mismatch"};
  // the flat list regrouped per copy for the one commit transition; the
  // session's shape was re-checked against the object by the time this runs
  std::vector<std::vector<uint64_t>> sd;
  size_t next = 0;
  return commit_session(token, *s, release, [&](ObjectMeta& m, size_t i,
                                                uint64_t now) {
    const uint32_t ncopies = s->shard_begin[i + 1] - s->shard_begin[i];
    sd.resize(ncopies);
    for (uint32_t c = 0; c < ncopies; ++c) {
      const uint32_t ns = s->shards[s->shard_begin[i] + c];
      sd[c].assign(shard_digests.begin() + next,
                   shard_digests.begin() + next + ns);
      next += ns;
    }
    commit_meta(m, obj_digests[i], sd, now);
  });
}

// What both token commits share once their arguments are counted: the epoch
// check under the shared lock, one transition per object, dirty marking, the
// view bump, the counter, the optional release and the flush.
template <typename CommitOne>
Result<void> KeystoneService::commit_session(uint64_t token,
                                             const PutSession& s,
                                             bool release,
                                             CommitOne commit_one) {
  const uint64_t now = now_ms();
  // SHARED lock — see upsert_start_token
  std::shared_lock lk(objects_mu_);
  BB_RETURN_IF_ERROR(session_current_locked(s));
  const bool persist = config_.persist_objects;
  const size_t n = s.metas.size();
  for (size_t i = 0; i < n; ++i) {
    // metas are scattered map nodes: prefetch ahead — this loop is in the
    // hot warm-step path (one commit per session put step)
    if (i + 8 < n) __builtin_prefetch(s.metas[i + 8], 1, 1);
    ObjectMeta* m = s.metas[i];
    commit_one(*m, i, now);
    if (persist) mark_dirty_locked(m->key, false);
  }
  bump_view();
  ctr_token_commits_.fetch_add(1);
  lk.unlock();
  if (release) {
    std::lock_guard<std::mutex> g(sessions_mu_);
    put_sessions_.erase(token);
  }
  flush_dirty_now();
  return {};
}

// ------------------------------------------------------------ cluster view

std::vector<WorkerInfo> KeystoneService::get_workers_info() {
  std::shared_lock lk(workers_mu_);
  std::vector<WorkerInfo> out;
  out.reserve(workers_.size());
  for (const auto& [id, w] : workers_) out.push_back(w);
  return out;
}

std::vector<MemoryPool> KeystoneService::get_memory_pools() {
  return allocator_.pools();
}

Result<void> KeystoneService::remove_worker(const WorkerId& id) {
  {
    std::shared_lock lk(workers_mu_);
    if (!workers_.count(id)) return Error{ErrorCode::KEY_NOT_FOUND, id};
  }
  // delete the coordination keys; the watchers do the rest (same path as a
  // TTL death). Reference left this unimplemented (keystone_service.cpp:125).
  coord_->del(prefix() + "/heartbeat/" + id);
  coord_->del(prefix() + "/workers/" + id);
  auto pools = coord_->get_prefix(prefix() + "/memory_pools/" + id + "/");
  if (pools.ok())
    for (const auto& kv : pools.value()) coord_->del(kv.key);
  cleanup_dead_worker(id);
  return {};
}

ClusterStats KeystoneService::get_cluster_stats() {
  ClusterStats s;
  auto as = allocator_.stats();
  s.total_capacity = as.total_capacity;
  s.total_used = as.total_used;
  s.num_pools = as.num_pools;
  {
    std::shared_lock lk(objects_mu_);
    s.num_objects = objects_.size();
  }
  {
    std::shared_lock lk(workers_mu_);
    s.num_workers = workers_.size();
  }
  s.view_version = view_version_.load();
  return s;
}

void KeystoneService::register_pool(const MemoryPool& pool) {
  allocator_.upsert_pool(pool);
  bump_view();
}

void KeystoneService::register_worker(const WorkerInfo& info) {
  std::unique_lock lk(workers_mu_);
  workers_[info.worker_id] = info;
  bump_view();
}

// ------------------------------------------------------------- watchers

void KeystoneService::upsert_worker(WorkerInfo w) {
  std::unique_lock lk(workers_mu_);
  w.last_heartbeat_ms = now_ms();
  workers_[w.worker_id] = std::move(w);
}

void KeystoneService::load_existing_state() {
  auto workers = coord_->get_prefix(prefix() + "/workers/");
  if (workers.ok()) {
    for (const auto& kv : workers.value()) {
      auto w = WorkerInfo::from_json(json::parse_or_null(kv.value));
      if (!w.worker_id.empty()) upsert_worker(std::move(w));
    }
  }
  auto pools = coord_->get_prefix(prefix() + "/memory_pools/");
  if (pools.ok()) {
    for (const auto& kv : pools.value()) {
      auto p = MemoryPool::from_json(json::parse_or_null(kv.value));
      if (!p.pool_id.empty()) allocator_.upsert_pool(p);
    }
  }
  if (config_.persist_objects) {
    auto objs = coord_->get_prefix(prefix() + "/objects/");
    size_t restored = 0, dropped = 0;
    if (objs.ok()) {
      for (const auto& kv : objs.value()) {
        ObjectMeta meta;
        if (!serde::from_bytes(kv.value, meta) || meta.key.empty()) {
          ++dropped;
          coord_->del(kv.key);
          continue;
        }
        {
          std::shared_lock lk(objects_mu_);
          if (objects_.count(meta.key)) continue;  // already live (rescan)
        }
        auto ad = allocator_.adopt(meta.key, meta.copies);
        if (!ad.ok()) {
          // pool gone or range occupied: the bytes are unreachable
          ++dropped;
          coord_->del(kv.key);
          continue;
        }
        std::unique_lock lk(objects_mu_);
        objects_[meta.key] = std::move(meta);
        ++restored;
      }
    }
    if (restored || dropped)
      BB_LOG(INFO) << "restored " << restored << " objects from coordination ("
                   << dropped << " dropped)";
  }
  bump_view();
}

void KeystoneService::setup_watchers() {
  auto w1 = coord_->watch_prefix(prefix() + "/workers/",
                                 [this](const coord::WatchEvent& ev) {
                                   handle_worker_event(ev);
                                 });
  auto w2 = coord_->watch_prefix(prefix() + "/memory_pools/",
                                 [this](const coord::WatchEvent& ev) {
                                   handle_pool_event(ev);
                                 });
  auto w3 = coord_->watch_prefix(prefix() + "/heartbeat/",
                                 [this](const coord::WatchEvent& ev) {
                                   handle_heartbeat_event(ev);
                                 });
  for (auto& w : {w1, w2, w3})
    if (w.ok()) watch_ids_.push_back(w.value());
}

namespace {
// counts a watch callback in for as long as it runs; stop() waits these out
struct CallbackGuard {
  explicit CallbackGuard(std::atomic<int>& c) : c_(c) { c_.fetch_add(1); }
  ~CallbackGuard() { c_.fetch_sub(1); }
  std::atomic<int>& c_;
};
}  // namespace

void KeystoneService::handle_worker_event(const coord::WatchEvent& ev) {
  CallbackGuard guard(cb_inflight_);
  if (!running_.load()) return;
  auto id = ev.key.substr(ev.key.rfind('/') + 1);
  if (ev.type == coord::EventType::PUT) {
    auto w = WorkerInfo::from_json(json::parse_or_null(ev.value));
    if (w.worker_id.empty()) return;
    upsert_worker(std::move(w));
    bump_view();
  } else {
    cleanup_dead_worker(id);
  }
}

void KeystoneService::handle_pool_event(const coord::WatchEvent& ev) {
  CallbackGuard guard(cb_inflight_);
  if (!running_.load()) return;
  if (ev.type == coord::EventType::PUT) {
    auto p = MemoryPool::from_json(json::parse_or_null(ev.value));
    if (p.pool_id.empty()) return;
    allocator_.upsert_pool(p);
  } else {
    auto id = ev.key.substr(ev.key.rfind('/') + 1);
    allocator_.remove_pool(id);
  }
  bump_view();
}

void KeystoneService::handle_heartbeat_event(const coord::WatchEvent& ev) {
  CallbackGuard guard(cb_inflight_);
  if (!running_.load()) return;
  auto id = ev.key.substr(ev.key.rfind('/') + 1);
  if (ev.type == coord::EventType::PUT) {
    std::unique_lock lk(workers_mu_);
    auto it = workers_.find(id);
    if (it != workers_.end()) it->second.last_heartbeat_ms = now_ms();
  } else {
    // TTL expiry or explicit delete ⇒ the worker is dead
    BB_LOG(WARN) << "worker heartbeat lost: " << id << " (event="
                 << (ev.type == coord::EventType::DELETE ? "DELETE" : "EXPIRE")
                 << " key=" << ev.key << ")";
    cleanup_dead_worker(id);
  }
}

void KeystoneService::cleanup_dead_worker(const WorkerId& id) {
  bool existed = false;
  {
    std::unique_lock lk(workers_mu_);
    existed = workers_.erase(id) > 0;
  }
  // drop the worker's pools from the placement engine
  for (const auto& p : allocator_.pools())
    if (p.worker_id == id) allocator_.remove_pool(p.pool_id);

  // Drop dead copies from object metadata so gets never return placements on
  // a dead worker (the reference served stale placements).
  {
    std::unique_lock lk(objects_mu_);
    std::vector<ObjectKey> lost;
    for (auto& [key, meta] : objects_) {
      auto& copies = meta.copies;
      auto before = copies.size();
      auto dead = std::stable_partition(copies.begin(), copies.end(),
                                        [&](const CopyPlacement& c) {
                                          for (const auto& s : c.shards)
                                            if (s.worker_id == id) return false;
                                          return true;
                                        });
      // Trim the matching leases from the allocator ledger too: if the worker
      // re-registers the same pool_id with a fresh PoolAllocator, a later
      // free/expiry must not replay stale leases into the new allocator
      // (double allocation / freeing live ranges).
      for (auto it = dead; it != copies.end(); ++it)
        allocator_.free_ranges(key, it->shards);
      if (dead != copies.end()) bump_placement_epoch_locked();
      copies.erase(dead, copies.end());
      if (copies.empty() && before > 0) lost.push_back(key);
    }
    for (const auto& k : lost) remove_object_locked(k);
    if (!lost.empty())
      BB_LOG(WARN) << "worker " << id << " death lost " << lost.size()
                   << " objects (no surviving replicas)";
  }
  // remove persistent registration keys (worker may have died without cleanup)
  coord_->del(prefix() + "/workers/" + id);
  auto pools = coord_->get_prefix(prefix() + "/memory_pools/" + id + "/");
  if (pools.ok())
    for (const auto& kv : pools.value()) coord_->del(kv.key);
  if (existed) bump_view();
}

}  // namespace blackbird
