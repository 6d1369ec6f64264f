// Storage tier interface: two-phase shard protocol (reserve → commit/abort),
// free, IO, stats, and the per-pool access advertisement.
// Capability parity with reference StorageBackend (storage_backend.h:46-126)
// + factory (ram_backend.cpp:261-303 — which left NVME/SSD/HDD unwired; this
// factory wires every class). MI355X-first: RAM_GPU is a first-class HBM3E
// backend, RAM_CPU lives in POSIX shared memory so same-host clients get the
// one-sided fast path, PINNED_CPU is page-locked (hipHostMalloc'd) staging.
#pragma once

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <string>

#include "blackbird/allocation/pool_allocator.h"
#include "blackbird/common/result.h"
#include "blackbird/common/types.h"

namespace blackbird {

struct ReservationToken {
  uint64_t token_id = 0;
  uint64_t offset = 0;
  uint64_t size = 0;
  uint64_t expires_ms = 0;
};

struct StorageStats {
  uint64_t capacity = 0;
  uint64_t used = 0;
  uint64_t reserved = 0;
  uint64_t num_shards = 0;
  uint64_t num_reservations = 0;
};

class StorageBackend {
 public:
  virtual ~StorageBackend() = default;

  virtual Result<void> initialize() = 0;
  virtual void shutdown() = 0;
  virtual StorageClass storage_class() const = 0;
  virtual uint64_t capacity() const = 0;
  // Filled after initialize(); the worker stamps the data endpoint in.
  virtual AccessInfo access_info() const = 0;
  // Raw base pointer for local zero-copy (device pointer for HBM; nullptr
  // for file-backed tiers without a mapping).
  virtual void* base_ptr() const = 0;

  // ------------------- two-phase shard protocol -------------------
  // Backend-chosen placement (local allocations: tier migration, tests).
  virtual Result<ReservationToken> reserve(uint64_t size) = 0;
  // Keystone-chosen placement (the cluster allocator owns pool offsets).
  virtual Result<ReservationToken> reserve_at(uint64_t offset, uint64_t size) = 0;
  virtual Result<void> commit(uint64_t token_id) = 0;
  virtual Result<void> abort(uint64_t token_id) = 0;
  virtual Result<void> free(uint64_t offset, uint64_t size) = 0;

  // ------------------------------ IO -------------------------------
  // Host-buffer IO (the TCP data path and tier migration use these; the
  // SHM/HIP-IPC fast paths bypass them entirely).
  virtual Result<void> write(uint64_t offset, const void* src, uint64_t len) = 0;
  virtual Result<void> read(uint64_t offset, void* dst, uint64_t len) = 0;
  // Object digest of a committed range (GPU kernel on the HBM tier).
  virtual Result<uint64_t> checksum(uint64_t offset, uint64_t len) = 0;

  virtual StorageStats stats() const = 0;
};

// Shared bookkeeping: range allocator + reservation/shard tables.
class BackendBase : public StorageBackend {
 public:
  explicit BackendBase(uint64_t capacity, uint64_t reservation_ttl_ms = 600000,
                       uint64_t alignment = 256);

  uint64_t capacity() const override { return capacity_; }
  Result<ReservationToken> reserve(uint64_t size) override;
  Result<ReservationToken> reserve_at(uint64_t offset, uint64_t size) override;
  Result<void> commit(uint64_t token_id) override;
  Result<void> abort(uint64_t token_id) override;
  Result<void> free(uint64_t offset, uint64_t size) override;
  StorageStats stats() const override;

 protected:
  Result<void> check_range(uint64_t offset, uint64_t len) const;
  void expire_reservations_locked(uint64_t now);
  // a fresh token for [offset, +size), not yet in reservations_
  ReservationToken new_token(uint64_t offset, uint64_t size);

  const uint64_t capacity_;
  const uint64_t reservation_ttl_ms_;
  PoolAllocator alloc_;
  mutable std::mutex mu_;
  std::atomic<uint64_t> next_token_{1};
  std::map<uint64_t, ReservationToken> reservations_;
  std::map<uint64_t, uint64_t> shards_;  // offset → size (committed)
};

// Process-local pool registry: worker backends register their base pointers
// so clients living in the SAME process (bench ranks, embedded clusters)
// reach pools by direct pointer instead of hipIpc/SHM re-import
// (hipIpcOpenMemHandle rejects same-process handles).
class LocalPools {
 public:
  struct Entry {
    void* base;  // nullptr for an unmapped tier
    uint64_t size;
    bool is_device;
    int device;
    // same-process backend handle (valid while the pool is registered): lets
    // clients embedded in the worker process reach UNMAPPED tiers (direct-IO
    // NVMe) through the backend's read/write instead of TCP loopback
    StorageBackend* backend;
  };

  static LocalPools& inst();
  void add(const PoolId& id, void* base, uint64_t size, bool is_device,
           int device, StorageBackend* backend = nullptr);
  void remove(const PoolId& id);
  // the pool's entry as registered, read under one lock
  std::optional<Entry> find(const PoolId& id);

 private:
  std::mutex mu_;
  std::map<PoolId, Entry> pools_;
};

// Factory — wires every storage class (the reference's factory returned
// nullptr for NVME/SSD/HDD).
Result<std::unique_ptr<StorageBackend>> create_storage_backend(
    const PoolConfig& cfg, const std::string& worker_id);

}  // namespace blackbird
