// Pieces the host Client and GpuClient share in their batch paths: the item
// fan-out and the resolved pool table of a v2 response. Host-only (no HIP).
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

}  // namespace blackbird
