// Keystone maintenance: everything that moves, repairs, checks, reclaims or
// persists objects behind the clients' backs — TTL GC, watermark eviction,
// tier migration, failure repair, compaction, digest scrubbing and the
// object map's persistence into coordination.
#include <algorithm>
#include <atomic>

#include "blackbird/common/fan_out.h"
#include "blackbird/common/log.h"
#include "blackbird/keystone/keystone_service.h"
#include "blackbird/rpc/messages.h"
#include "blackbird/rpc/methods.h"
#include "keystone_internal.h"

namespace blackbird {

namespace {
constexpr int kMaintenanceThreads = 4;  // concurrent migrations or repairs
}  // namespace

// ------------------------------------------------------- gc and eviction

void KeystoneService::run_gc_once() {
  uint64_t now = now_ms();
  std::unique_lock lk(objects_mu_);
  std::vector<ObjectKey> dead;
  for (const auto& [key, meta] : objects_) {
    if (meta.expired(now)) dead.push_back(key);
    // abandoned PENDING puts: reclaim after 10 minutes (a patch start
    // keeps created_ms, its own clock counts)
    else if (meta.state == ObjectState::PENDING &&
             now > std::max(meta.created_ms, meta.patch_started_ms) + 600000)
      dead.push_back(key);
  }
  for (const auto& k : dead) remove_object_locked(k);
  if (!dead.empty()) {
    ctr_gc_.fetch_add(dead.size());
    BB_LOG(DEBUG) << "gc reclaimed " << dead.size() << " objects";
  }
}

void KeystoneService::run_eviction_once() {
  auto as = allocator_.stats();
  if (as.total_capacity == 0) return;
  double fill = static_cast<double>(as.total_used) / as.total_capacity;
  if (fill < config_.eviction_high_watermark) return;

  std::unique_lock lk(objects_mu_);
  // age-based: evict least-recently-accessed committed objects
  std::vector<std::pair<uint64_t, ObjectKey>> cand;
  for (const auto& [key, meta] : objects_)
    if (meta.state == ObjectState::COMMITTED)
      cand.emplace_back(meta.last_access_ms, key);
  std::sort(cand.begin(), cand.end());
  size_t target = static_cast<size_t>(cand.size() * config_.eviction_ratio) + 1;
  size_t evicted = 0;
  for (const auto& [ts, key] : cand) {
    if (evicted >= target) break;
    remove_object_locked(key);
    ++evicted;
  }
  ctr_evictions_.fetch_add(evicted);
  BB_LOG(INFO) << "eviction: fill " << fill << " → evicted " << evicted
               << " objects";
}

void KeystoneService::gc_loop() {
  while (running_) {
    {
      std::unique_lock<std::mutex> lk(cv_mu_);
      cv_.wait_for(lk, std::chrono::milliseconds(config_.gc_interval_ms),
                   [this] { return !running_.load(); });
    }
    if (!running_) break;
    if (!is_leader()) continue;  // standby: the leader owns maintenance
    run_gc_once();
    run_repair_once();
    if (config_.enable_tiering) run_tiering_once();
    if (config_.compact_fragmentation_threshold > 0) run_compaction_once();
    if (config_.scrub_interval_ms > 0) run_scrub_once();
    run_eviction_once();
  }
}

// ------------------------------------------------- moving bytes: the pull

rpc::RpcClient* KeystoneService::data_client(const std::string& endpoint) {
  std::lock_guard<std::mutex> g(data_clients_mu_);
  auto& pool = data_clients_[endpoint];
  // round-robin over up to kDataConns live connections (grown on demand);
  // a dead connection is replaced in its slot
  if (pool.conns.size() < kDataConns) {
    auto c = std::make_unique<rpc::RpcClient>();
    if (!c->connect(endpoint).ok())
      return pool.conns.empty() ? nullptr : pool.conns[0].get();
    pool.conns.push_back(std::move(c));
    return pool.conns.back().get();
  }
  pool.cursor = (pool.cursor + 1) % pool.conns.size();
  auto& slot = pool.conns[pool.cursor];
  if (!slot->connected()) {
    auto c = std::make_unique<rpc::RpcClient>();
    if (!c->connect(endpoint).ok()) return nullptr;
    slot = std::move(c);
  }
  return slot.get();
}

namespace {
// Sub-ranges of ordered shards `srcs` (covering [0, total)) that cover the
// object range [a, b).
std::vector<ShardPlacement> slice_shards(const std::vector<ShardPlacement>& srcs,
                                         uint64_t a, uint64_t b) {
  std::vector<ShardPlacement> out;
  uint64_t off = 0;
  for (const auto& s : srcs) {
    uint64_t s_begin = off, s_end = off + s.length;
    off = s_end;
    uint64_t lo = std::max(a, s_begin), hi = std::min(b, s_end);
    if (lo >= hi) continue;
    ShardPlacement part = s;
    part.offset = s.offset + (lo - s_begin);
    part.length = hi - lo;
    out.push_back(std::move(part));
  }
  return out;
}
}  // namespace

// EXCLUSIVE lock: the full-struct copy must not race shared-lock session
// commits. No lock is held during the transfer that follows.
Result<ObjectMeta> KeystoneService::snapshot_committed(const ObjectKey& key) {
  std::unique_lock lk(objects_mu_);
  auto it = objects_.find(key);
  if (it == objects_.end()) return Error{ErrorCode::OBJECT_NOT_FOUND, key};
  if (it->second.state != ObjectState::COMMITTED)
    return Error{ErrorCode::OBJECT_NOT_COMMITTED, key};
  return it->second;
}

Result<void> KeystoneService::pull_into(
    const std::vector<ShardPlacement>& dst_shards,
    const std::vector<ShardPlacement>& src_shards) {
  uint64_t off = 0;
  for (const auto& dst : dst_shards) {
    PullReq req;
    req.dst_pool = dst.pool_id;
    req.dst_offset = dst.offset;
    req.total_len = dst.length;
    // sources carry their access info so the puller can reach remote pools
    req.srcs = slice_shards(src_shards, off, off + dst.length);
    for (auto& sh : req.srcs) {
      auto a = allocator_.pool_access(sh.pool_id);
      if (a.ok()) sh.access = std::move(a.value());
    }
    off += dst.length;
    auto dst_access = allocator_.pool_access(dst.pool_id);
    if (!dst_access.ok()) return dst_access.error();
    auto* dc = data_client(dst_access.value().endpoint);
    if (!dc)
      return Error{ErrorCode::CONNECT_FAILED, dst_access.value().endpoint};
    auto pulled =
        dc->call_raw(rpc::methods::DATA_PULL, serde::to_bytes(req), 120000);
    if (!pulled.ok()) return pulled.error();
  }
  return {};
}

// ---------------------------------------------------------- tier migration

Result<void> KeystoneService::migrate_object(const ObjectKey& key,
                                             StorageClass target) {
  auto snapped = snapshot_committed(key);
  if (!snapped.ok()) return snapped.error();
  const ObjectMeta& snap = snapped.value();
  if (snap.copies.empty())
    return Error{ErrorCode::INVALID_STATE, "object has no copies"};

  // allocate the destination placement under a temp ledger key — same copy
  // count as the source; prefer one shard per copy, fall back to striping
  // when the target tier is too fragmented for a contiguous range
  const std::string tmp_key = key + "\x01mig";
  PlacementConfig mcfg;
  mcfg.replication = static_cast<uint32_t>(snap.copies.size());
  mcfg.max_workers_per_copy = 1;
  mcfg.required_class = target;
  auto placed = allocator_.allocate(tmp_key, snap.size, mcfg);
  if (!placed.ok()) {
    mcfg.max_workers_per_copy = 4;
    placed = allocator_.allocate(tmp_key, snap.size, mcfg);
    if (!placed.ok()) return placed.error();
  }

  // each destination copy pulls from the matching source copy
  for (size_t ci = 0; ci < placed.value().size(); ++ci) {
    auto pulled = pull_into(placed.value()[ci].shards,
                            snap.copies[ci % snap.copies.size()].shards);
    if (!pulled.ok()) {
      allocator_.free(tmp_key);
      return pulled.error();
    }
  }

  // commit the move: re-validate, swap placement, release the old ranges
  {
    std::unique_lock lk(objects_mu_);
    auto it = objects_.find(key);
    bool unchanged = it != objects_.end() &&
                     it->second.state == ObjectState::COMMITTED &&
                     it->second.copies.size() == snap.copies.size();
    for (size_t ci = 0; unchanged && ci < snap.copies.size(); ++ci)
      unchanged = it->second.copies[ci].shards == snap.copies[ci].shards;
    if (!unchanged) {
      lk.unlock();
      allocator_.free(tmp_key);
      return Error{ErrorCode::INVALID_STATE, "object changed during migration"};
    }
    allocator_.free(key);
    auto rn = allocator_.rename(tmp_key, key);
    if (!rn.ok()) {
      // old ranges already freed; keep the new placement under tmp is wrong —
      // this cannot happen (key was just freed), but guard anyway
      BB_LOG(ERROR) << "migration rename failed: " << rn.message();
    }
    it->second.copies = std::move(placed.value());
    if (it->second.copies.size() == 1 &&
        it->second.copies[0].shards.size() == 1)
      it->second.copies[0].shards[0].digest = it->second.checksum;
    it->second.access_count = 0;
    bump_placement_epoch_locked();
    mark_dirty_locked(key, false);
    bump_view();
  }
  ctr_migrations_.fetch_add(1);
  BB_LOG(INFO) << "migrated " << key << " → " << to_string(target);
  return {};
}

void KeystoneService::run_tiering_once() {
  // per-tier fill from the allocator's pool view
  struct Agg {
    uint64_t cap = 0, used = 0;
  };
  std::map<int, Agg> tiers;  // tier_rank → agg
  std::map<int, StorageClass> rank_class;
  for (const auto& p : allocator_.pools()) {
    int r = tier_rank(p.storage_class);
    tiers[r].cap += p.size;
    tiers[r].used += p.used;
    rank_class[r] = p.storage_class;
  }
  if (tiers.empty()) return;

  uint32_t moves_left = config_.tier_max_moves_per_cycle;

  // ---- demotion: fastest overfull tier → next tier with room ----
  for (auto it = tiers.begin(); it != tiers.end() && moves_left > 0; ++it) {
    auto [rank, agg] = *it;
    if (agg.cap == 0) continue;
    double fill = static_cast<double>(agg.used) / agg.cap;
    if (fill <= config_.tier_high_watermark) continue;
    // find the next tier down with capacity headroom
    StorageClass target{};
    bool found = false;
    for (auto jt = std::next(it); jt != tiers.end(); ++jt) {
      double jf = jt->second.cap
                      ? static_cast<double>(jt->second.used) / jt->second.cap
                      : 1.0;
      if (jf < config_.tier_high_watermark) {
        target = rank_class[jt->first];
        found = true;
        break;
      }
    }
    if (!found) continue;

    // LRU single-copy committed objects living in this tier
    std::vector<std::pair<uint64_t, ObjectKey>> cands;
    {
      std::shared_lock lk(objects_mu_);
      for (const auto& [key, meta] : objects_) {
        if (rload(meta.state) != ObjectState::COMMITTED ||
            meta.copies.size() != 1)
          continue;
        bool in_tier = !meta.copies[0].shards.empty();
        for (const auto& sh : meta.copies[0].shards)
          if (tier_rank(sh.storage_class) != rank) in_tier = false;
        if (in_tier) cands.emplace_back(rload(meta.last_access_ms), key);
      }
    }
    std::sort(cands.begin(), cands.end());
    uint64_t bytes_over = agg.used - static_cast<uint64_t>(
                                         agg.cap * config_.tier_high_watermark);
    // pick the batch up-front, then migrate with a small worker fan-out
    // (each migration is an independent pull; the data plane overlaps)
    std::vector<ObjectKey> batch;
    uint64_t planned = 0;
    for (const auto& [ts, key] : cands) {
      if (batch.size() >= moves_left || planned >= bytes_over) break;
      uint64_t sz = 0;
      {
        std::shared_lock lk(objects_mu_);
        auto oit = objects_.find(key);
        if (oit == objects_.end()) continue;
        sz = oit->second.size;
      }
      batch.push_back(key);
      planned += sz;
    }
    if (!batch.empty()) {
      std::atomic<uint32_t> done{0};
      fan_out(batch.size(), kMaintenanceThreads, [&](size_t bi) {
        if (migrate_object(batch[bi], target).ok()) done.fetch_add(1);
      });
      moves_left -= std::min(moves_left, done.load());
    }
  }

  // ---- promotion: hot objects move toward the fastest tier with room ----
  if (config_.promote_hot_threshold > 0 && moves_left > 0) {
    auto fastest = tiers.begin();
    if (fastest->second.cap > 0) {
      double fill =
          static_cast<double>(fastest->second.used) / fastest->second.cap;
      if (fill < config_.tier_high_watermark * 0.9) {
        StorageClass target = rank_class[fastest->first];
        std::vector<std::pair<uint32_t, ObjectKey>> hot;
        {
          std::shared_lock lk(objects_mu_);
          for (const auto& [key, meta] : objects_) {
            if (rload(meta.state) != ObjectState::COMMITTED ||
                meta.copies.size() != 1 || meta.copies[0].shards.empty())
              continue;
            const uint32_t ac = rload(meta.access_count);
            if (ac < config_.promote_hot_threshold) continue;
            if (tier_rank(meta.copies[0].shards[0].storage_class) >
                fastest->first)
              hot.emplace_back(ac, key);
          }
        }
        std::sort(hot.rbegin(), hot.rend());  // hottest first
        for (const auto& [cnt, key] : hot) {
          if (moves_left == 0) break;
          if (migrate_object(key, target).ok()) --moves_left;
        }
      }
    }
  }

  // decay access counts so "hot" means hot recently (only meaningful when
  // promotion is on — skip the full-map pass otherwise)
  if (config_.promote_hot_threshold > 0) {
    std::unique_lock lk(objects_mu_);
    for (auto& [key, meta] : objects_) meta.access_count /= 2;
  }
}

// ---------------------------------------------------------- failure repair

Result<void> KeystoneService::repair_object(const ObjectKey& key) {
  auto snapped = snapshot_committed(key);
  if (!snapped.ok()) return snapped.error();
  const ObjectMeta& snap = snapped.value();
  if (snap.copies.empty())
    return Error{ErrorCode::NO_PLACEMENT, key};
  if (snap.copies.size() >= snap.replication) return {};

  // allocate one extra copy on workers not already holding the object
  std::vector<WorkerId> holders;
  uint32_t max_idx = 0;
  for (const auto& c : snap.copies) {
    max_idx = std::max(max_idx, c.copy_index);
    for (const auto& sh : c.shards) holders.push_back(sh.worker_id);
  }
  PlacementConfig rcfg;
  rcfg.replication = 1;
  rcfg.max_workers_per_copy = 1;
  const std::string tmp_key = key + "\x01rep";
  auto placed = allocator_.allocate_extra_copy(tmp_key, snap.size, rcfg,
                                               max_idx + 1, holders);
  if (!placed.ok()) return placed.error();

  // pull the bytes from the surviving copy into each new shard
  auto pulled = pull_into(placed.value().shards, snap.copies[0].shards);
  if (!pulled.ok()) {
    allocator_.free(tmp_key);
    return pulled.error();
  }

  {
    std::unique_lock lk(objects_mu_);
    auto it = objects_.find(key);
    if (it == objects_.end() || it->second.state != ObjectState::COMMITTED ||
        it->second.copies.size() != snap.copies.size()) {
      lk.unlock();
      allocator_.free(tmp_key);
      return Error{ErrorCode::INVALID_STATE, "object changed during repair"};
    }
    auto mr = allocator_.merge_into(tmp_key, key);
    if (!mr.ok()) {
      lk.unlock();
      allocator_.free(tmp_key);
      return mr.error();
    }
    it->second.copies.push_back(std::move(placed.value()));
    bump_placement_epoch_locked();
    mark_dirty_locked(key, false);
    bump_view();
  }
  ctr_repairs_.fetch_add(1);
  BB_LOG(INFO) << "repaired " << key << " (copies "
               << snap.copies.size() << " → " << snap.copies.size() + 1 << ")";
  return {};
}

void KeystoneService::run_repair_once() {
  std::vector<ObjectKey> degraded;
  {
    std::shared_lock lk(objects_mu_);
    for (const auto& [key, meta] : objects_)
      if (rload(meta.state) == ObjectState::COMMITTED &&
          !meta.copies.empty() && meta.copies.size() < meta.replication)
        degraded.push_back(key);
  }
  if (degraded.empty()) return;
  if (degraded.size() > config_.repair_max_per_cycle)
    degraded.resize(config_.repair_max_per_cycle);
  // fan the re-replication pulls out over a few threads — after a worker
  // death the backlog is bandwidth-bound on the surviving workers, not on
  // keystone
  fan_out(degraded.size(), kMaintenanceThreads, [&](size_t i) {
    auto r = repair_object(degraded[i]);
    if (!r.ok() && r.code() != ErrorCode::NO_SPACE)
      BB_LOG(WARN) << "repair of " << degraded[i]
                   << " failed: " << r.message();
  });
}

// ------------------------------------------------------- object persistence

void KeystoneService::mark_dirty_locked(const ObjectKey& key, bool removed) {
  if (!config_.persist_objects) return;
  std::lock_guard<std::mutex> g(dirty_mu_);
  dirty_[key] = removed;
}

KeystoneService::DirtySet KeystoneService::drain_dirty() {
  DirtySet batch;
  std::lock_guard<std::mutex> g(dirty_mu_);
  batch.swap(dirty_);
  return batch;
}

void KeystoneService::encode_dirty(const DirtySet& batch,
                                   std::vector<coord::KV>& puts,
                                   std::vector<std::string>& dels) {
  const std::string obj_prefix = prefix() + "/objects/";
  // EXCLUSIVE: serde reads every meta field; a concurrent shared-lock
  // commit of the same key must not interleave with the serialization
  std::unique_lock lk(objects_mu_);
  for (const auto& [key, removed] : batch) {
    if (removed) {
      dels.push_back(obj_prefix + key);
      continue;
    }
    auto it = objects_.find(key);
    if (it == objects_.end()) continue;
    puts.push_back(coord::KV{obj_prefix + key, serde::to_bytes(it->second)});
  }
}

// Commit and remove acknowledgements call this before they answer, so an
// acked mutation survives an immediate leader crash; the 100 ms persist_loop
// calls it for the mutations nobody waits for (tiering, repair, scrub).
// Either way: one fenced coordination round trip (put_many) for the whole
// dirty set, put back on failure for the next call to retry.
void KeystoneService::flush_dirty_now() {
  if (!config_.persist_objects || !coord_) return;
  DirtySet batch = drain_dirty();
  if (batch.empty()) return;
  std::vector<coord::KV> puts;
  std::vector<std::string> dels;
  encode_dirty(batch, puts, dels);
  auto r = coord_->put_many(puts, dels);
  if (!r.ok()) {
    BB_LOG(WARN) << "persist failed (" << r.error().message
                 << "); re-queued for the next flush";
    std::lock_guard<std::mutex> g(dirty_mu_);
    for (auto& [key, removed] : batch) dirty_.emplace(key, removed);
  }
}

void KeystoneService::persist_loop() {
  while (running_) {
    {
      std::unique_lock<std::mutex> lk(cv_mu_);
      cv_.wait_for(lk, std::chrono::milliseconds(100),
                   [this] { return !running_.load(); });
    }
    flush_dirty_now();
  }
  flush_dirty_now();  // whatever the shutdown raced in
}

// ------------------------------------------------------------- compaction

Result<uint32_t> KeystoneService::compact_pool(const PoolId& pool_id,
                                               uint32_t max_moves) {
  // find the pool and its class
  StorageClass cls{};
  bool found = false;
  for (const auto& p : allocator_.pools()) {
    if (p.pool_id == pool_id) {
      cls = p.storage_class;
      found = true;
      break;
    }
  }
  if (!found) return Error{ErrorCode::POOL_NOT_FOUND, pool_id};

  // single-copy objects with a shard in this pool, largest offset first —
  // re-allocating them walks data toward the low end and coalesces holes
  std::vector<std::pair<uint64_t, ObjectKey>> cands;
  {
    std::shared_lock lk(objects_mu_);
    for (const auto& [key, meta] : objects_) {
      if (rload(meta.state) != ObjectState::COMMITTED ||
          meta.copies.size() != 1)
        continue;
      for (const auto& sh : meta.copies[0].shards)
        if (sh.pool_id == pool_id) {
          cands.emplace_back(sh.offset, key);
          break;
        }
    }
  }
  std::sort(cands.rbegin(), cands.rend());
  uint32_t moved = 0;
  for (const auto& [off, key] : cands) {
    if (moved >= max_moves) break;
    // migrate within the same tier: the allocator's best-fit will prefer
    // the coalesced low-offset holes
    auto r = migrate_object(key, cls);
    if (r.ok()) ++moved;
  }
  return moved;
}

void KeystoneService::run_compaction_once() {
  const double thr = config_.compact_fragmentation_threshold;
  if (thr <= 0) return;
  for (const auto& p : allocator_.pools()) {
    auto st = allocator_.pool_stats(p.pool_id);
    if (!st.ok() || st.value().used == 0) continue;
    if (st.value().fragmentation <= thr) continue;
    auto moved = compact_pool(p.pool_id, config_.tier_max_moves_per_cycle);
    if (moved.ok() && moved.value() > 0)
      BB_LOG(INFO) << "auto-compacted " << p.pool_id << ": moved "
                   << moved.value() << " objects (frag "
                   << st.value().fragmentation << ")";
  }
}

// ------------------------------------------------------------------ scrub

uint32_t KeystoneService::run_scrub_once(uint32_t max_objects) {
  if (max_objects == 0) max_objects = config_.scrub_batch;
  const uint64_t now = now_ms();
  struct Cand {
    ObjectKey key;
    uint64_t checksum;
    // every copy, striped or not: shard digests recorded at put time make
    // each shard independently verifiable (the round-1 scrubber silently
    // skipped striped copies — exactly the objects with the most failure
    // surface)
    std::vector<std::vector<ShardPlacement>> copies;
  };
  std::vector<Cand> cands;
  {
    std::unique_lock lk(objects_mu_);
    for (auto& [key, meta] : objects_) {
      if (cands.size() >= max_objects) break;
      if (meta.state != ObjectState::COMMITTED || meta.checksum == 0)
        continue;
      if (meta.last_scrub_ms != 0 &&
          now < meta.last_scrub_ms + config_.scrub_interval_ms)
        continue;
      if (meta.copies.empty()) continue;
      meta.last_scrub_ms = now;
      Cand cd;
      cd.key = key;
      cd.checksum = meta.checksum;
      for (const auto& c : meta.copies) cd.copies.push_back(c.shards);
      cands.push_back(std::move(cd));
    }
  }

  uint32_t quarantined = 0;
  for (const auto& cd : cands) {
    for (const auto& shards : cd.copies) {
      // verify every shard of the copy; ONE bad shard quarantines the copy
      bool copy_bad = false;
      bool verified_any = false;
      const ShardPlacement* bad_sh = nullptr;
      uint64_t bad_want = 0, bad_got = 0;
      for (const auto& sh : shards) {
        const uint64_t want =
            sh.digest != 0 ? sh.digest
                           : (shards.size() == 1 ? cd.checksum : 0);
        if (want == 0) continue;  // digest never recorded (e.g. repair copy)
        auto access = allocator_.pool_access(sh.pool_id);
        if (!access.ok()) continue;  // pool gone: dead-worker cleanup owns it
        auto* dc = data_client(access.value().endpoint);
        if (!dc) continue;
        ChecksumReq req{sh.pool_id, sh.offset, sh.length};
        auto resp = dc->call_raw(rpc::methods::DATA_CHECKSUM,
                                 serde::to_bytes(req), 60000);
        if (!resp.ok()) continue;  // transient worker trouble: retry next pass
        U64Msg got;
        if (!serde::from_bytes(resp.value(), got)) continue;
        verified_any = true;
        if (got.v != want) {
          copy_bad = true;
          bad_sh = &sh;
          bad_want = want;
          bad_got = got.v;
          break;
        }
      }
      if (!verified_any || !copy_bad) continue;

      // corrupt copy: quarantine it (re-validate placement under the lock)
      BB_LOG(ERROR) << "scrub: digest mismatch on " << cd.key << " @ "
                    << bad_sh->pool_id << "+" << bad_sh->offset << " (want "
                    << bad_want << " got " << bad_got << ")";
      bool dropped = false;
      bool object_gone = false;
      {
        std::unique_lock lk(objects_mu_);
        auto it = objects_.find(cd.key);
        if (it == objects_.end()) continue;
        auto& copies = it->second.copies;
        for (auto cit = copies.begin(); cit != copies.end(); ++cit) {
          if (cit->shards == shards) {
            copies.erase(cit);
            bump_placement_epoch_locked();
            dropped = true;
            break;
          }
        }
        if (!dropped) continue;  // placement changed under us
        if (copies.empty()) {
          // last copy was corrupt: the object is lost — drop it rather
          // than serve bytes that cannot verify
          BB_LOG(ERROR) << "scrub: all copies of " << cd.key
                        << " corrupt — removing object";
          remove_object_locked(cd.key);
          object_gone = true;
        } else {
          mark_dirty_locked(cd.key, false);
          bump_view();
        }
      }
      if (dropped && !object_gone) allocator_.free_ranges(cd.key, shards);
      ctr_scrubbed_.fetch_add(1);
      ++quarantined;
    }
  }
  return quarantined;
}

}  // namespace blackbird
