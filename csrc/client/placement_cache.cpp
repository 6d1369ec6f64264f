#include "blackbird/client/placement_cache.h"

namespace blackbird {

void PlacementCache::set_enabled(bool on) {
  std::lock_guard<std::mutex> g(mu_);
  on_ = on;
  if (!on) map_.clear();
  ++epoch_;
}

std::optional<PlacementCache::Entry> PlacementCache::find(
    const ObjectKey& key) const {
  std::lock_guard<std::mutex> g(mu_);
  auto it = map_.find(key);
  if (it == map_.end()) return std::nullopt;
  return it->second;
}

PlacementCache::Binding PlacementCache::bind_locked(const KeyList& keys) {
  Binding b;
  b.slots_.reserve(keys.size());
  for (const ObjectKey* k : keys) {
    auto it = map_.find(*k);
    if (it == map_.end()) return {};
    b.slots_.push_back(&it->second);
  }
  b.cache_ = this;
  b.epoch_ = epoch_;
  return b;
}

PlacementCache::Binding PlacementCache::record(const std::vector<Put>& puts,
                                               const KeyList* bind_keys) {
  std::lock_guard<std::mutex> g(mu_);
  if (!on_) return {};
  for (const Put& p : puts) {
    if (p.entry.digest == 0) continue;  // 0 marks "no digest"
    auto [it, inserted] = map_.try_emplace(p.key, p.entry);
    if (inserted) continue;
    Entry& e = it->second;
    if (e.pool_id != p.entry.pool_id || e.offset != p.entry.offset ||
        e.size != p.entry.size || e.shards != p.entry.shards)
      ++epoch_;
    e = p.entry;
  }
  if (map_.size() > kMaxEntries) {
    map_.clear();
    ++epoch_;
  }
  return bind_keys ? bind_locked(*bind_keys) : Binding{};
}

void PlacementCache::erase(const KeyList& keys) {
  std::lock_guard<std::mutex> g(mu_);
  for (const ObjectKey* k : keys) map_.erase(*k);
  ++epoch_;
}

void PlacementCache::clear() {
  std::lock_guard<std::mutex> g(mu_);
  map_.clear();
  ++epoch_;
}

PlacementCache::Lookup PlacementCache::lookup(
    const std::vector<Want>& wants) {
  Lookup lk;
  std::lock_guard<std::mutex> g(mu_);
  for (size_t i = 0; i < wants.size(); ++i) {
    auto it = map_.find(wants[i].key);
    if (it != map_.end() && it->second.size <= wants[i].capacity) {
      lk.hits.emplace_back(static_cast<uint32_t>(i), it->second);
      lk.binding_.slots_.push_back(&it->second);
    } else {
      lk.misses.push_back(static_cast<uint32_t>(i));
    }
  }
  lk.binding_.cache_ = this;
  lk.binding_.epoch_ = epoch_;
  return lk;
}

PlacementCache::Binding PlacementCache::settle(Lookup&& lk,
                                               const KeyList& stale,
                                               bool bind) {
  std::lock_guard<std::mutex> g(mu_);
  if (!stale.empty()) {
    for (const ObjectKey* k : stale) map_.erase(*k);
    ++epoch_;
  }
  if (!bind || !lk.misses.empty() || !live(lk.binding_)) return {};
  return std::move(lk.binding_);
}

bool PlacementCache::read_digests(const Binding& b, uint64_t* out,
                                  size_t n) const {
  std::lock_guard<std::mutex> g(mu_);
  if (!live(b) || n != b.slots_.size()) return false;
  for (size_t j = 0; j < n; ++j) out[j] = b.slots_[j]->digest;
  return true;
}

bool PlacementCache::refresh_digests(const Binding& b, const uint64_t* digests,
                                     size_t stride) {
  std::lock_guard<std::mutex> g(mu_);
  if (!live(b)) return false;
  for (size_t j = 0; j < b.slots_.size(); ++j)
    b.slots_[j]->digest = digests[j * stride];
  return true;
}

}  // namespace blackbird
