// Concrete storage backends for every tier.
// Capability parity with reference RamBackend (ram_backend.cpp),
// MmapDiskBackend (mmap_disk_backend.cpp) and the unimplemented RAM_GPU stub
// (worker_service.cpp:196) — re-designed MI355X-first:
//  * ShmRamBackend (RAM_CPU): POSIX shared memory, so same-host clients map
//    the pool and do one-sided memcpy (the xGMI-node analogue of the
//    reference's UCX one-sided RMA for the host tier).
//  * HbmBackend (RAM_GPU): first-class HBM3E — hipMalloc pool on a chosen
//    device, advertised via hipIpcMemHandle for one-sided hipMemcpy from any
//    process on the node; digests via the MFMA checksum kernel.
//  * PinnedBackend (PINNED_CPU): shm + hipHostRegister — page-locked staging
//    for the GPU→DRAM→NVMe spill path, still SHM-addressable by clients.
//  * MmapDiskBackend (HDD): ftruncate+mmap(MAP_SHARED) backing file.
// The host-mapped tiers share MappedBackend: one mapping and the IO over it.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <random>

#include "blackbird/common/hex.h"
#include "blackbird/common/log.h"
#include "blackbird/gpu/gpu_kernels.h"
#include "blackbird/gpu/hip_check.h"
#include "blackbird/worker/storage_backend.h"

#include <hip/hip_runtime_api.h>

namespace blackbird {

namespace {

// ---------------------------------------------------- host-mapped tiers
// One host mapping of capacity_ bytes and the bounds-checked IO over it. A
// tier supplies how the mapping is made (map) and torn down (unmap), its
// access_info() and its storage_class(); its destructor calls shutdown(),
// which this class cannot do for it once the tier's part is destroyed.
class MappedBackend : public BackendBase {
 public:
  using BackendBase::BackendBase;

  Result<void> initialize() final {
    auto m = map();
    if (!m.ok()) return m.error();
    base_ = m.value();
    return {};
  }

  void shutdown() final {
    if (!base_) return;
    unmap(base_);
    base_ = nullptr;
  }

  void* base_ptr() const final { return base_; }

  Result<void> write(uint64_t offset, const void* src, uint64_t len) final {
    BB_RETURN_IF_ERROR(check_range(offset, len));
    std::memcpy(static_cast<uint8_t*>(base_) + offset, src, len);
    return {};
  }
  Result<void> read(uint64_t offset, void* dst, uint64_t len) final {
    BB_RETURN_IF_ERROR(check_range(offset, len));
    std::memcpy(dst, static_cast<uint8_t*>(base_) + offset, len);
    return {};
  }
  Result<uint64_t> checksum(uint64_t offset, uint64_t len) final {
    BB_RETURN_IF_ERROR(check_range(offset, len));
    return gpu::checksum_cpu(static_cast<uint8_t*>(base_) + offset, len);
  }

 protected:
  virtual Result<void*> map() = 0;
  virtual void unmap(void* base) = 0;

  // MAP_SHARED mapping of the whole pool over `fd`, which is closed either
  // way; nullptr with errno set on failure
  void* map_fd(int fd) const {
    void* p = mmap(nullptr, capacity_, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    ::close(fd);
    return p == MAP_FAILED ? nullptr : p;
  }

  // the advertisement of a mapping that other processes reach as `kind`
  AccessInfo advertise(AccessKind kind) const {
    AccessInfo a;
    a.kind = kind;
    a.base_addr = reinterpret_cast<uint64_t>(base_);
    return a;
  }

 private:
  void* base_ = nullptr;
};

// ------------------------------------------------------------- shm tier
class ShmRamBackend : public MappedBackend {
 public:
  ShmRamBackend(uint64_t cap, std::string shm_name, StorageClass cls)
      : MappedBackend(cap), shm_name_(std::move(shm_name)), class_(cls) {}
  ~ShmRamBackend() override { shutdown(); }

  StorageClass storage_class() const override { return class_; }

  AccessInfo access_info() const override {
    AccessInfo a = advertise(AccessKind::SHM);
    a.shm_name = shm_name_;
    return a;
  }

 protected:
  Result<void*> map() override {
    shm_unlink(shm_name_.c_str());
    int fd = shm_open(shm_name_.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
    if (fd < 0)
      return Error{ErrorCode::BACKEND_INIT_FAILED,
                   "shm_open " + shm_name_ + ": " + strerror(errno)};
    if (ftruncate(fd, static_cast<off_t>(capacity_)) != 0) {
      ::close(fd);
      shm_unlink(shm_name_.c_str());
      return Error{ErrorCode::BACKEND_INIT_FAILED,
                   "ftruncate: " + std::string(strerror(errno))};
    }
    void* base = map_fd(fd);
    if (!base) {
      shm_unlink(shm_name_.c_str());
      return Error{ErrorCode::BACKEND_INIT_FAILED,
                   "mmap: " + std::string(strerror(errno))};
    }
    return base;
  }

  void unmap(void* base) override {
    munmap(base, capacity_);
    shm_unlink(shm_name_.c_str());
  }

 private:
  std::string shm_name_;
  StorageClass class_;
};

// ------------------------------------------------- pinned staging tier
class PinnedBackend : public ShmRamBackend {
 public:
  PinnedBackend(uint64_t cap, std::string shm_name)
      : ShmRamBackend(cap, std::move(shm_name), StorageClass::PINNED_CPU) {}
  ~PinnedBackend() override { shutdown(); }

 protected:
  Result<void*> map() override {
    auto base = ShmRamBackend::map();
    if (base.ok() && gpu::available()) {
      hipError_t e =
          hipHostRegister(base.value(), capacity_, hipHostRegisterDefault);
      if (e == hipSuccess) registered_ = true;
      else BB_LOG(WARN) << "hipHostRegister failed (" << hipGetErrorString(e)
                        << ") — pinned tier degrades to pageable";
    }
    return base;
  }

  void unmap(void* base) override {
    if (registered_) {
      (void)hipHostUnregister(base);
      registered_ = false;
    }
    ShmRamBackend::unmap(base);
  }

 private:
  bool registered_ = false;
};

// ------------------------------------------------------------ CXL.mem tier
// DAX-device (or dax-mounted file) mapping; falls back to anonymous memory
// when no device is present — the behavior the reference's CxlMemoryBackend
// intended (cxl_memory_backend.cpp:73-121) but never shipped compiling (it
// referenced error codes that did not exist).
class CxlMemBackend : public MappedBackend {
 public:
  CxlMemBackend(uint64_t cap, std::string dev_path)
      : MappedBackend(cap), path_(std::move(dev_path)) {}
  ~CxlMemBackend() override { shutdown(); }

  StorageClass storage_class() const override { return StorageClass::CXL_MEM; }
  AccessInfo access_info() const override {
    return advertise(AccessKind::TCP);  // DAX mappings are not name-shareable
  }

 protected:
  Result<void*> map() override {
    if (!path_.empty()) {
      int fd = ::open(path_.c_str(), O_RDWR);
      if (fd >= 0)
        if (void* base = map_fd(fd)) return base;
      BB_LOG(WARN) << "CXL_MEM: cannot map " << path_
                   << " — falling back to anonymous memory";
    }
    void* base = mmap(nullptr, capacity_, PROT_READ | PROT_WRITE,
                      MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (base == MAP_FAILED)
      return Error{ErrorCode::BACKEND_INIT_FAILED, "CXL_MEM mmap failed"};
    return base;
  }

  void unmap(void* base) override { munmap(base, capacity_); }

 private:
  std::string path_;
};

// ------------------------------------------------------------ disk tier
class MmapDiskBackend : public MappedBackend {
 public:
  MmapDiskBackend(uint64_t cap, std::string path, StorageClass cls)
      : MappedBackend(cap), path_(std::move(path)), class_(cls) {}
  ~MmapDiskBackend() override { shutdown(); }

  StorageClass storage_class() const override { return class_; }
  AccessInfo access_info() const override {
    return advertise(AccessKind::TCP);
  }

 protected:
  Result<void*> map() override {
    int fd = ::open(path_.c_str(), O_CREAT | O_RDWR, 0644);
    if (fd < 0)
      return Error{ErrorCode::BACKEND_INIT_FAILED,
                   "open " + path_ + ": " + strerror(errno)};
    if (ftruncate(fd, static_cast<off_t>(capacity_)) != 0) {
      ::close(fd);
      return Error{ErrorCode::BACKEND_INIT_FAILED,
                   "ftruncate " + path_ + ": " + strerror(errno)};
    }
    void* base = map_fd(fd);
    if (!base)
      return Error{ErrorCode::BACKEND_INIT_FAILED,
                   "mmap " + path_ + ": " + strerror(errno)};
    madvise(base, capacity_, MADV_RANDOM);
    return base;
  }

  void unmap(void* base) override {
    msync(base, capacity_, MS_ASYNC);
    munmap(base, capacity_);
  }

 private:
  std::string path_;
  StorageClass class_;
};

// ------------------------------------------------------------ HBM tier
class HbmBackend : public BackendBase {
 public:
  HbmBackend(uint64_t cap, int device) : BackendBase(cap), device_(device) {}
  ~HbmBackend() override { shutdown(); }

  Result<void> initialize() override {
    if (!gpu::available())
      return Error{ErrorCode::NO_GPU,
                   "HBM tier requires an MI355X device (RAM_GPU pool)"};
    BB_HIP_TRY(hipSetDevice(device_));
    BB_HIP_TRY(hipMalloc(&base_, capacity_));
    BB_HIP_TRY(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    hipIpcMemHandle_t handle{};
    hipError_t e = hipIpcGetMemHandle(&handle, base_);
    if (e == hipSuccess) {
      ipc_hex_ = to_hex(&handle, sizeof(handle));
    } else {
      BB_LOG(WARN) << "hipIpcGetMemHandle failed (" << hipGetErrorString(e)
                   << ") — HBM pool reachable via TCP data path only";
    }
    BB_LOG(INFO) << "HBM pool: " << (capacity_ >> 20) << " MiB on device "
                 << device_;
    return {};
  }

  void shutdown() override {
    if (base_) {
      (void)hipSetDevice(device_);
      (void)hipFree(base_);
      base_ = nullptr;
    }
    if (stream_) {
      (void)hipStreamDestroy(stream_);
      stream_ = nullptr;
    }
  }

  StorageClass storage_class() const override { return StorageClass::RAM_GPU; }
  void* base_ptr() const override { return base_; }
  hipStream_t stream() const { return stream_; }
  int device() const { return device_; }

  AccessInfo access_info() const override {
    AccessInfo a;
    a.kind = ipc_hex_.empty() ? AccessKind::TCP : AccessKind::HIP_IPC;
    a.device_id = device_;
    a.ipc_handle_hex = ipc_hex_;
    a.base_addr = reinterpret_cast<uint64_t>(base_);
    return a;
  }

  Result<void> write(uint64_t offset, const void* src, uint64_t len) override {
    BB_RETURN_IF_ERROR(check_range(offset, len));
    BB_HIP_TRY(hipSetDevice(device_));
    BB_HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(base_) + offset, src, len,
                              hipMemcpyHostToDevice, stream_));
    BB_HIP_TRY(hipStreamSynchronize(stream_));
    return {};
  }
  Result<void> read(uint64_t offset, void* dst, uint64_t len) override {
    BB_RETURN_IF_ERROR(check_range(offset, len));
    BB_HIP_TRY(hipSetDevice(device_));
    BB_HIP_TRY(hipMemcpyAsync(dst, static_cast<uint8_t*>(base_) + offset, len,
                              hipMemcpyDeviceToHost, stream_));
    BB_HIP_TRY(hipStreamSynchronize(stream_));
    return {};
  }
  Result<uint64_t> checksum(uint64_t offset, uint64_t len) override {
    BB_RETURN_IF_ERROR(check_range(offset, len));
    return gpu::checksum_sync(static_cast<uint8_t*>(base_) + offset, len,
                              device_, stream_);
  }

 private:
  int device_;
  void* base_ = nullptr;
  hipStream_t stream_ = nullptr;
  std::string ipc_hex_;
};

}  // namespace

std::unique_ptr<StorageBackend> make_direct_file_backend(uint64_t cap,
                                                         const std::string& path,
                                                         StorageClass cls);

Result<std::unique_ptr<StorageBackend>> create_storage_backend(
    const PoolConfig& cfg, const std::string& worker_id) {
  if (cfg.size_bytes == 0)
    return Error{ErrorCode::CONFIG_INVALID, "pool size_bytes is 0"};
  // Per-boot random suffix: a restarted worker must NOT reuse the previous
  // incarnation's shm name — clients cache mappings by name, and a reused
  // name would silently alias the orphaned old segment. The fresh name
  // reaches clients through the pool's AccessInfo advertisement.
  char suffix[12];
  snprintf(suffix, sizeof(suffix), "_%08x",
           static_cast<unsigned>(std::random_device{}()));
  std::string shm = "/bb_" + worker_id + "_" + cfg.pool_id + suffix;
  std::unique_ptr<StorageBackend> b;
  switch (cfg.storage_class) {
    case StorageClass::RAM_CPU:
      b = std::make_unique<ShmRamBackend>(cfg.size_bytes, shm, StorageClass::RAM_CPU);
      break;
    case StorageClass::PINNED_CPU:
      b = std::make_unique<PinnedBackend>(cfg.size_bytes, shm);
      break;
    case StorageClass::RAM_GPU:
      b = std::make_unique<HbmBackend>(cfg.size_bytes, cfg.gpu_device_id);
      break;
    case StorageClass::CXL_MEM:
      // mount_path = the DAX device/file; empty or unmappable → anonymous
      b = std::make_unique<CxlMemBackend>(cfg.size_bytes, cfg.mount_path);
      break;
    case StorageClass::NVME:
    case StorageClass::SSD:
    case StorageClass::HDD: {
      if (cfg.mount_path.empty())
        return Error{ErrorCode::CONFIG_INVALID, "disk pool needs mount_path"};
      std::string path = cfg.mount_path + "/bb_" + worker_id + "_" +
                         cfg.pool_id + ".dat";
      if (cfg.storage_class == StorageClass::HDD)
        b = std::make_unique<MmapDiskBackend>(cfg.size_bytes, path, cfg.storage_class);
      else
        // async direct-IO tier (parity: the reference's io_uring backend used
        // O_DIRECT for NVME/SSD)
        b = make_direct_file_backend(cfg.size_bytes, path, cfg.storage_class);
      break;
    }
  }
  if (!b) return Error{ErrorCode::CONFIG_INVALID, "unknown storage class"};
  return b;
}

}  // namespace blackbird
