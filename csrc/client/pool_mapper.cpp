#include "blackbird/client/pool_mapper.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <hip/hip_runtime_api.h>

#include "blackbird/common/hex.h"
#include "blackbird/gpu/gpu_kernels.h"

namespace blackbird {

PoolMapper::~PoolMapper() {
  for (void* p : registered_) (void)hipHostUnregister(p);
  for (auto& [k, m] : shm_) munmap(m.ptr, m.size);
  for (auto& [k, p] : ipc_) (void)hipIpcCloseMemHandle(p);
}

PoolView PoolMapper::local(const PoolId& id) {
  auto e = LocalPools::inst().find(id);
  if (!e) return {};
  return {static_cast<uint8_t*>(e->base), e->size, e->is_device, e->backend};
}

PoolView PoolMapper::remote(const AccessInfo& a) {
  if (a.kind == AccessKind::SHM && !a.shm_name.empty())
    return map_shm(a.shm_name);
  if (a.kind == AccessKind::HIP_IPC && !a.ipc_handle_hex.empty())
    return open_ipc(a.ipc_handle_hex);
  return {};
}

PoolView PoolMapper::map_shm(const std::string& name) {
  std::lock_guard<std::mutex> g(mu_);
  auto it = shm_.find(name);
  if (it == shm_.end()) {
    int fd = shm_open(name.c_str(), O_RDWR, 0600);
    if (fd < 0) return {};
    struct stat st {};
    if (fstat(fd, &st) != 0 || st.st_size <= 0) {
      ::close(fd);
      return {};
    }
    const uint64_t size = static_cast<uint64_t>(st.st_size);
    void* p = mmap(nullptr, size, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    ::close(fd);
    if (p == MAP_FAILED) return {};
    it = shm_.emplace(name, Shm{p, size}).first;
  }
  return {static_cast<uint8_t*>(it->second.ptr), it->second.size, false,
          nullptr};
}

PoolView PoolMapper::open_ipc(const std::string& handle_hex) {
  std::lock_guard<std::mutex> g(mu_);
  auto it = ipc_.find(handle_hex);
  if (it == ipc_.end()) {
    if (ipc_failed_.count(handle_hex) || !gpu::available()) return {};
    hipIpcMemHandle_t h{};
    if (!from_hex(handle_hex, &h, sizeof(h))) return {};
    void* p = nullptr;
    if (hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess) !=
        hipSuccess) {
      (void)hipGetLastError();  // don't leak the probe error to launch checks
      ipc_failed_.insert(handle_hex);
      return {};
    }
    it = ipc_.emplace(handle_hex, p).first;
  }
  return {static_cast<uint8_t*>(it->second), 0, true, nullptr};
}

void* PoolMapper::host_dev_map(const std::string& pool_key, void* base,
                               uint64_t size) {
  std::lock_guard<std::mutex> g(mu_);
  auto it = dev_maps_.find(pool_key);
  if (it != dev_maps_.end()) return it->second;
  if (dev_map_failed_.count(pool_key)) return nullptr;
  void* dp = nullptr;
  if (hipHostGetDevicePointer(&dp, base, 0) != hipSuccess) {
    // the probe failing is EXPECTED for not-yet-registered memory — clear
    // the sticky thread error so a later launch check doesn't inherit it
    (void)hipGetLastError();
    if (hipHostRegister(base, size, hipHostRegisterDefault) != hipSuccess) {
      (void)hipGetLastError();
      dev_map_failed_.insert(pool_key);
      return nullptr;
    }
    registered_.push_back(base);
    if (hipHostGetDevicePointer(&dp, base, 0) != hipSuccess) {
      (void)hipGetLastError();
      dev_map_failed_.insert(pool_key);
      return nullptr;
    }
  }
  dev_maps_[pool_key] = dp;
  return dp;
}

}  // namespace blackbird
