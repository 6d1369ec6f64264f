#include "blackbird/transport/rccl_engine.h"

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <thread>

#include "blackbird/common/hex.h"
#include "blackbird/common/types.h"
#include "blackbird/common/log.h"
#include "blackbird/gpu/hip_check.h"

namespace blackbird {

namespace {
Error rccl_err(ncclResult_t r, const char* what) {
  return Error{ErrorCode::RCCL_ERROR,
               std::string(what) + ": " + ncclGetErrorString(r)};
}
#define BB_RCCL(expr)                                   \
  do {                                                  \
    ncclResult_t _r = (expr);                           \
    if (_r != ncclSuccess) return rccl_err(_r, #expr);  \
  } while (0)
}  // namespace

RcclEngine::~RcclEngine() { destroy(); }

void RcclEngine::destroy() {
  if (comm_) {
    ncclCommDestroy(comm_);
    comm_ = nullptr;
  }
}

Result<void> RcclEngine::init(std::shared_ptr<coord::CoordService> coord,
                              const std::string& cluster_id,
                              const std::string& tag, int rank, int nranks,
                              int device, int timeout_ms) {
  if (comm_) return Error{ErrorCode::INVALID_STATE, "already initialized"};
  rank_ = rank;
  nranks_ = nranks;
  device_ = device;
  BB_HIP_TRY(hipSetDevice(device));

  const std::string key =
      "/blackbird/clusters/" + cluster_id + "/rccl/" + tag;
  ncclUniqueId id{};
  if (rank == 0) {
    BB_RCCL(ncclGetUniqueId(&id));
    BB_RETURN_IF_ERROR(coord->put(
        key, to_hex(&id, sizeof(id)),
        static_cast<uint64_t>(timeout_ms) * 2));
  } else {
    uint64_t deadline = now_ms() + static_cast<uint64_t>(timeout_ms);
    for (;;) {
      auto v = coord->get(key);
      if (v.ok() && from_hex(v.value(), &id, sizeof(id))) break;
      if (now_ms() > deadline)
        return Error{ErrorCode::TIMEOUT, "rccl uniqueId not published: " + key};
      std::this_thread::sleep_for(std::chrono::milliseconds(20));
    }
  }
  BB_RCCL(ncclCommInitRank(&comm_, nranks, id, rank));
  BB_LOG(INFO) << "rccl communicator up: rank " << rank << "/" << nranks
               << " on device " << device;
  return {};
}

Result<void> RcclEngine::send(const void* dev_ptr, uint64_t nbytes, int peer,
                              hipStream_t stream) {
  BB_RCCL(ncclSend(dev_ptr, nbytes, ncclUint8, peer, comm_, stream));
  return {};
}

Result<void> RcclEngine::recv(void* dev_ptr, uint64_t nbytes, int peer,
                              hipStream_t stream) {
  BB_RCCL(ncclRecv(dev_ptr, nbytes, ncclUint8, peer, comm_, stream));
  return {};
}

Result<void> RcclEngine::group_start() {
  BB_RCCL(ncclGroupStart());
  return {};
}

Result<void> RcclEngine::group_end() {
  BB_RCCL(ncclGroupEnd());
  return {};
}

Result<void> RcclEngine::alltoallv(const std::vector<const void*>& send_ptrs,
                                   const std::vector<uint64_t>& send_bytes,
                                   const std::vector<void*>& recv_ptrs,
                                   const std::vector<uint64_t>& recv_bytes,
                                   hipStream_t stream) {
  if (static_cast<int>(send_ptrs.size()) != nranks_ ||
      static_cast<int>(recv_ptrs.size()) != nranks_)
    return Error{ErrorCode::INVALID_ARGUMENT, "alltoallv needs nranks slots"};
  BB_RCCL(ncclGroupStart());
  for (int peer = 0; peer < nranks_; ++peer) {
    if (peer == rank_) continue;
    if (send_bytes[peer] > 0)
      BB_RCCL(ncclSend(send_ptrs[peer], send_bytes[peer], ncclUint8, peer,
                       comm_, stream));
    if (recv_bytes[peer] > 0)
      BB_RCCL(ncclRecv(recv_ptrs[peer], recv_bytes[peer], ncclUint8, peer,
                       comm_, stream));
  }
  BB_RCCL(ncclGroupEnd());
  // self slot: plain device-local copy on the same stream
  if (send_bytes[rank_] > 0) {
    if (send_bytes[rank_] != recv_bytes[rank_])
      return Error{ErrorCode::SIZE_MISMATCH, "self slot size mismatch"};
    BB_HIP_TRY(hipMemcpyAsync(recv_ptrs[rank_], send_ptrs[rank_],
                              send_bytes[rank_], hipMemcpyDeviceToDevice,
                              stream));
  }
  return {};
}

Result<void> RcclEngine::broadcast(void* dev_ptr, uint64_t nbytes, int root,
                                   hipStream_t stream) {
  BB_RCCL(ncclBroadcast(dev_ptr, dev_ptr, nbytes, ncclUint8, root, comm_, stream));
  return {};
}

}  // namespace blackbird
