// Host-side helpers of the C-ABI entry points (capi.hip, train_ops.hip,
// optim.hip, input_stage.hip): the error return and the alignment check.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <string>

#include "../../include/stgcn_hip.h"

namespace stgcn {

void set_last_error(const std::string &msg);  // capi.hip (stgcn_last_error)

inline int fail(int code, const std::string &msg) {
  set_last_error(msg);
  return code;
}

// The alignment contract of stgcn_hip.h (Conventions): the first pointer of the
// list that is off `align` bytes fails the call, by name, before any launch.
// Null pointers pass (optional arguments; the null checks come first).
struct NamedPtr {
  const void *p;
  const char *name;
};
inline int check_aligned(std::initializer_list<NamedPtr> ptrs, unsigned align) {
  for (const NamedPtr &q : ptrs)
    if (((uintptr_t)q.p & (align - 1)) != 0)
      return fail(STGCN_E_INVALID,
                  std::string(q.name) + ": must be " + std::to_string(align) + "-byte aligned");
  return STGCN_OK;
}

}  // namespace stgcn

#define NP(v) stgcn::NamedPtr{v, #v}

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return stgcn::fail(STGCN_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));  \
  } while (0)
