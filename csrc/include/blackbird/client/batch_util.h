// Pieces the host Client and GpuClient share in their batch paths: the item
// fan-out, the resolved pool table of a v2 response and the small steps of
// the ranged calls. Host-only (no HIP).
#pragma once

#include <cstdint>
#include <vector>

#include "blackbird/common/fan_out.h"
#include "blackbird/common/types.h"

namespace blackbird {

// One pool-table entry of a v2 response, resolved once per batch.
struct PoolRef {
  PoolId pool_id;
  uint8_t* base = nullptr;  // mapped base, or nullptr: go shard by shard
  AccessInfo access;        // for the per-shard fallback
  ShardPlacement shard(uint64_t offset, uint64_t length) const {
    ShardPlacement sp;
    sp.pool_id = pool_id;
    sp.offset = offset;
    sp.length = length;
    sp.access = access;
    return sp;
  }
};

// base_of(pool_id, &access) → the base this client can address, or nullptr
template <typename BaseOf>
std::vector<PoolRef> resolve_pool_table(const std::vector<PoolId>& ids,
                                        BaseOf&& base_of) {
  std::vector<PoolRef> pools(ids.size());
  for (size_t i = 0; i < ids.size(); ++i) {
    pools[i].pool_id = ids[i];
    pools[i].base = base_of(ids[i], &pools[i].access);
  }
  return pools;
}

// ---- ranged access ----
// a copy's shard lengths, for the planners of gpu/patch_plan.h
inline std::vector<uint64_t> shard_lens_of(const CopyPlacement& copy) {
  std::vector<uint64_t> lens;
  lens.reserve(copy.shards.size());
  for (const auto& s : copy.shards) lens.push_back(s.length);
  return lens;
}

// [offset, offset+length) lies inside an object of `size` bytes
inline bool range_inside(uint64_t offset, uint64_t length, uint64_t size) {
  return offset <= size && length <= size - offset;
}

// [shard_off, shard_off+n) of `s` as a placement of its own, for the shard
// movers
inline ShardPlacement sub_shard(const ShardPlacement& s, uint64_t shard_off,
                                uint64_t n) {
  ShardPlacement sub = s;
  sub.offset = s.offset + shard_off;
  sub.length = n;
  return sub;
}

}  // namespace blackbird
