// Verified placement cache: {pool, offset, size, digest} of this client's own
// puts, by key — for a striped object the shard list of copy 0 as well — plus
// the session bindings that ride on it.
//
// The class owns the map, its lock, the enabled flag and the invalidation
// epoch. A Binding is a session's hold on the digest slots of an ordered key
// list; it reaches the slots directly (no hashing per step) and is refused
// once anything was erased, moved or cleared since it was taken — every
// such mutation bumps the epoch, and every use of a binding re-checks it
// under the lock. Nothing outside the class sees a pointer, an iterator or
// an epoch value. Host-only: no GPU header is needed here.
#pragma once

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <optional>
#include <unordered_map>
#include <utility>
#include <vector>

#include "blackbird/common/types.h"

namespace blackbird {

class PlacementCache {
 public:
  // past this many entries a put batch empties the cache (bindings die)
  static constexpr size_t kMaxEntries = size_t{1} << 20;

  // One shard of a striped copy: the object's bytes lie in the shards back
  // to back.
  struct Shard {
    PoolId pool_id;
    uint64_t offset = 0;
    uint64_t length = 0;
    bool operator==(const Shard& o) const {
      return pool_id == o.pool_id && offset == o.offset && length == o.length;
    }
  };
  struct Entry {
    PoolId pool_id;
    uint64_t offset = 0;
    uint64_t size = 0;
    uint64_t digest = 0;  // of the whole object, striped or not
    // copy 0 of a striped object; empty = the single range above (a striped
    // entry keeps shard 0's pool and offset there)
    std::vector<Shard> shards;
  };
  // key lists point at strings the caller keeps alive for the call
  using KeyList = std::vector<const ObjectKey*>;

  class Binding {
   public:
    bool bound() const { return cache_ != nullptr; }
    size_t size() const { return slots_.size(); }

   private:
    friend class PlacementCache;
    const PlacementCache* cache_ = nullptr;
    uint64_t epoch_ = 0;
    // mapped values of the cache's map, item order (unordered_map keeps
    // them in place across insert/rehash; erase/clear bump the epoch)
    std::vector<Entry*> slots_;
  };

  // Disabling empties the cache; either way every binding dies.
  void set_enabled(bool on);
  bool enabled() const { std::lock_guard<std::mutex> g(mu_); return on_; }
  bool enabled_and_nonempty() const {
    std::lock_guard<std::mutex> g(mu_);
    return on_ && !map_.empty();
  }

  std::optional<Entry> find(const ObjectKey& key) const;

  // One put batch under one lock: a zero digest is skipped, a new key is
  // inserted, a known key overwritten — and if its pool, offset, size or
  // shard list changed (a re-placed object) every binding dies: sessions hold the old
  // pool addresses. Growing past kMaxEntries empties the cache. With
  // `bind_keys` the result is a binding over those keys in order, unbound
  // if one is absent. A disabled cache records and binds nothing.
  struct Put {
    const ObjectKey& key;
    Entry entry;
  };
  Binding record(const std::vector<Put>& puts,
                 const KeyList* bind_keys = nullptr);

  // Both always kill every binding, even when a named key is absent.
  void erase(const KeyList& keys);
  void clear();

  // One get batch under one lock: an item hits if its key is cached with
  // size <= capacity. The result remembers what settle() needs to tell
  // whether anything was invalidated since.
  struct Want {
    const ObjectKey& key;
    uint64_t capacity;
  };
  class Lookup {
   public:
    std::vector<std::pair<uint32_t, Entry>> hits;  // item index, entry copy
    std::vector<uint32_t> misses;                  // item indices

   private:
    friend class PlacementCache;
    Binding binding_;  // slots parallel to hits
  };
  Lookup lookup(const std::vector<Want>& wants);

  // After the verified read of a lookup's hits, under one lock: erases the
  // `stale` keys (digest mismatches). With `bind`, returns a binding over
  // the lookup's items iff none was stale, every item hit, and nothing was
  // invalidated since the lookup; unbound otherwise.
  Binding settle(Lookup&& lk, const KeyList& stale, bool bind);

  // ---- binding use ----
  bool owns(const Binding& b) const { return b.cache_ == this; }
  // these three refuse (false) a binding that is stale, from a disabled
  // cache or from another cache
  bool valid(const Binding& b) const {
    std::lock_guard<std::mutex> g(mu_);
    return live(b);
  }
  // out[j] = digest of slot j; n must be the binding's size
  bool read_digests(const Binding& b, uint64_t* out, size_t n) const;
  // digest of slot j = digests[j * stride]
  bool refresh_digests(const Binding& b, const uint64_t* digests,
                       size_t stride = 1);

 private:
  bool live(const Binding& b) const {  // under mu_
    return b.cache_ == this && on_ && b.epoch_ == epoch_;
  }
  Binding bind_locked(const KeyList& keys);

  mutable std::mutex mu_;
  bool on_ = false;
  std::unordered_map<ObjectKey, Entry> map_;
  uint64_t epoch_ = 0;  // bumped on every erase, move, clear and on/off
};

}  // namespace blackbird
