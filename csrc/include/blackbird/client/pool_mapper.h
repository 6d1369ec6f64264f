// How a pool's bytes are reached one-sidedly, for the host Client, GpuClient
// and the worker's TransferEngine alike: the same-process registry first,
// then the pool's advertised POSIX-shm segment (host tier) or hipIpc handle
// (GPU tier), both cached per mapper.
#pragma once

#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "blackbird/common/types.h"
#include "blackbird/worker/storage_backend.h"

namespace blackbird {

// A pool as one process can address it.
struct PoolView {
  uint8_t* base = nullptr;  // host or device pointer; nullptr: not
                            // addressable one-sidedly
  uint64_t size = 0;        // mapped size, 0 = unknown (IPC import)
  bool device = false;      // base is a device pointer
  // same-process backend handle; set with base == nullptr for the unmapped
  // direct-IO tier
  StorageBackend* local = nullptr;

  // [offset, offset + length) lies inside the mapping, as far as its size is
  // known
  bool contains(uint64_t offset, uint64_t length) const {
    return size == 0 || (length <= size && offset <= size - length);
  }
};

class PoolMapper {
 public:
  ~PoolMapper();

  // First rung: a pool registered by a worker of this process. Needs no
  // access info, so ask here before fetching any.
  static PoolView local(const PoolId& id);

  // Later rungs, for a pool of another process: its shm segment or its IPC
  // handle, whichever `a` advertises. An empty view sends the caller to TCP.
  PoolView remote(const AccessInfo& a);

  // Device-visible mapping of a HOST pool: pins (hipHostRegister, unless the
  // memory is already page-locked) and maps it into the GPU address space
  // once, cached per pool. Lets the fused copy/digest kernels read and write
  // host tiers (PINNED_CPU, local RAM_CPU/shm) directly at PCIe DMA speed
  // instead of double-copying through a staging bounce. nullptr when the GPU
  // cannot address it (registration failed / no GPU).
  void* host_dev_map(const std::string& pool_key, void* base, uint64_t size);

 private:
  struct Shm {
    void* ptr;
    uint64_t size;
  };

  // Maps the whole segment, cached by name. The size comes from the segment
  // itself; an empty segment is a failure.
  PoolView map_shm(const std::string& name);
  // Imports the handle into this process, cached. Negative cache: a handle
  // that failed to open is not retried (handles are immutable per
  // allocation). Whether there is a GPU at all is asked on a miss only, so a
  // cached import costs no HIP call.
  PoolView open_ipc(const std::string& handle_hex);

  std::mutex mu_;
  std::map<std::string, Shm> shm_;
  std::map<std::string, void*> ipc_;
  std::set<std::string> ipc_failed_;
  std::map<std::string, void*> dev_maps_;  // pool key → device-visible ptr
  std::set<std::string> dev_map_failed_;
  std::vector<void*> registered_;  // bases WE pinned (unregister on teardown)
};

}  // namespace blackbird
