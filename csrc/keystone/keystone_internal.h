// What keystone_service.cpp, keystone_maintenance.cpp and keystone_rpc.cpp
// share and nobody outside the keystone needs.
#pragma once

#include <atomic>

#include "blackbird/common/result.h"

namespace blackbird {

// Relaxed atomic access to a hot ObjectMeta field. Commits mutate these
// fields under the SHARED objects lock, so every reader and writer that does
// not hold the lock exclusively goes through here.
template <typename T>
inline T rload(const T& f) {
  return std::atomic_ref<T>(const_cast<T&>(f)).load(std::memory_order_relaxed);
}
template <typename T>
inline void rstore(T& f, T v) {
  std::atomic_ref<T>(f).store(v, std::memory_order_relaxed);
}

inline Error not_leader() {
  return Error{ErrorCode::NOT_LEADER, "standby keystone; retry on leader"};
}

}  // namespace blackbird
