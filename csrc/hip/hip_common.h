// Shared helpers for the gfx950 kernel TUs.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "blackbird/common/result.h"
#include "blackbird/gpu/hip_check.h"

namespace blackbird::gpu {

// Directly after a <<<>>> launch of the kernel `name` (a string literal).
#define BB_HIP_LAUNCHED(name)                                     \
  do {                                                            \
    if (hipError_t _le = hipGetLastError(); _le != hipSuccess)    \
      return ::blackbird::gpu::hip_error(_le, name " launch");    \
  } while (0)

// Persistent descriptor staging (pinned + device), grown once and reused:
// per-call hipMallocAsync/hipFreeAsync descriptor churn proved both slow and
// fault-prone. Entry points keep one thread_local instance each. A caller
// that returns BEFORE its stream has run (batched_copy) calls in_flight() so
// that the next acquire() does not overwrite an upload a previous launch
// still reads; callers that synchronize their stream need not.
struct DescStaging {
  void* pinned = nullptr;
  void* device = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;

  Result<void> acquire(size_t bytes) {
    if (ev) BB_HIP_TRY(hipEventSynchronize(ev));  // prior launch done
    if (bytes > cap) {
      if (pinned) BB_HIP_TRY(hipHostFree(pinned));
      if (device) BB_HIP_TRY(hipFree(device));
      cap = std::max<size_t>(bytes * 2, 1 << 16);
      BB_HIP_TRY(hipHostMalloc(&pinned, cap, hipHostMallocDefault));
      BB_HIP_TRY(hipMalloc(&device, cap));
    }
    return {};
  }

  Result<void> in_flight(hipStream_t stream) {
    if (!ev) BB_HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    BB_HIP_TRY(hipEventRecord(ev, stream));
    return {};
  }
};

// One stream of the shared transfer pool (memops.hip), held under its mutex
// until this object goes out of scope.
struct XferStream {
  hipStream_t stream = nullptr;
  std::unique_lock<std::mutex> lock;
};
Result<void> acquire_xfer_stream(XferStream& out);

}  // namespace blackbird::gpu
