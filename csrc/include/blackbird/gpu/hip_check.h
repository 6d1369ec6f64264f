// The one HIP error check of the core library and the kernel TUs.
#pragma once

#include <string>

#include <hip/hip_runtime_api.h>

#include "blackbird/common/result.h"

namespace blackbird::gpu {

inline Error hip_error(hipError_t e, const char* what) {
  return Error{ErrorCode::HIP_ERROR,
               std::string(what) + ": " + hipGetErrorString(e)};
}

}  // namespace blackbird::gpu

// Returns `<expr>: <error string>` from the enclosing function when `expr`
// fails.
#define BB_HIP_TRY(expr)                                        \
  do {                                                          \
    hipError_t _e = (expr);                                     \
    if (_e != hipSuccess) {                                     \
      (void)hipGetLastError(); /* consume sticky thread error */ \
      return ::blackbird::gpu::hip_error(_e, #expr);            \
    }                                                           \
  } while (0)
