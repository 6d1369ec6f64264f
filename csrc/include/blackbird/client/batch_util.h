// Pieces the host Client and GpuClient share in their batch paths: the item
// fan-out and the resolved pool table of a v2 response. Host-only (no HIP).
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <future>
#include <vector>

#include "blackbird/common/types.h"

namespace blackbird {

// Runs body(t, next) on max(1, min(threads, n)) spawned threads, t being the
// thread's number; next(i) hands each index of [0, n) out once across all of
// them and returns false when none is left. Never runs inline: a batch's
// transfers always execute on spawned threads.
template <typename Body>
void fan_out_threads(size_t n, int threads, Body&& body) {
  std::atomic<size_t> counter{0};
  auto next = [&](size_t& i) { return (i = counter.fetch_add(1)) < n; };
  const int nthreads =
      std::max(1, std::min<int>(threads, static_cast<int>(n)));
  std::vector<std::future<void>> futs;
  for (int t = 0; t < nthreads; ++t)
    futs.push_back(std::async(std::launch::async, [&, t] { body(t, next); }));
  for (auto& f : futs) f.get();
}

// fn(i) for every i in [0, n), spread over the threads above
template <typename Fn>
void fan_out(size_t n, int threads, Fn&& fn) {
  fan_out_threads(n, threads, [&](int, auto& next) {
    for (size_t i; next(i);) fn(i);
  });
}

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
