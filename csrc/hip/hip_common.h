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

// A stream of the current device that lives as long as the process and is
// never captured (memops.hip): what DescStaging waits on.
Result<hipStream_t> staging_anchor();

// Persistent descriptor staging (pinned + device), grown once and reused:
// per-call hipMallocAsync/hipFreeAsync descriptor churn proved both slow and
// fault-prone. Entry points keep one thread_local instance each. A caller
// that returns BEFORE its stream has run (batched_copy) calls in_flight() so
// that the next acquire() does not overwrite an upload a previous launch
// still reads; callers that synchronize their stream need not.
// The staging outlives the streams it is used with (a thread_local against a
// client's streams), so acquire() must not wait on anything that remembers
// such a stream: an event does, and waiting on one whose stream has since
// been destroyed has the runtime look that stream up again (seen as
// "operation not permitted on an event last recorded in a capturing stream"
// from hipEventSynchronize, with no capture open anywhere). in_flight()
// therefore hands the launch stream's position to the anchor stream while the
// launch stream is certainly alive, and acquire() waits on the anchor.
struct DescStaging {
  void* pinned = nullptr;
  void* device = nullptr;
  size_t cap = 0;
  hipEvent_t hop = nullptr;      // launch stream -> anchor, used at once
  hipStream_t anchor = nullptr;  // set while a launch may be in flight

  Result<void> acquire(size_t bytes) {
    if (anchor) {  // prior launch done
      BB_HIP_TRY(hipStreamSynchronize(anchor));
      anchor = nullptr;
    }
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
    auto a = staging_anchor();
    if (!a.ok()) return a.error();
    if (!hop) BB_HIP_TRY(hipEventCreateWithFlags(&hop, hipEventDisableTiming));
    BB_HIP_TRY(hipEventRecord(hop, stream));
    BB_HIP_TRY(hipStreamWaitEvent(a.value(), hop, 0));
    anchor = a.value();
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
