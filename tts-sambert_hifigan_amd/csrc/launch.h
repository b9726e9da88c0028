// launch.h — the one launch path of every kernel that uses dynamic LDS (host only).
// A kernel file keeps its instance table (Instance plus the key fields its lookup needs), its
// shape validation, its LDS formula and its grid; everything after that is launch_instance.
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>

#include "kernels.h"

namespace hfg {

// One kernel instance: the entry point and its template-instance name as rocprofv3 prints it
// (formatted on first use; the longest, a conv1d_bf16x3 instance, is 70 characters).
template <typename... Args>
struct Instance {
  void (*fn)(Args...);
  char name[112];
};
template <typename... Args>
constexpr Instance<Args...> instance_of(void (*fn)(Args...)) {
  return {fn, {0}};
}
template <typename T>
struct KernelArg {  // Args come from the instance alone, the arguments convert to them
  typedef T type;
};

// Launch e.fn(args...) with lds_bytes of dynamic LDS.  format_name(buf, size) writes the
// instance name; it runs once per instance, under setup_mutex().  *name (if asked for) is
// set only when the launch is attempted.
template <typename... Args, typename NameFn>
hipError_t launch_instance(Instance<Args...>& e, NameFn&& format_name, dim3 grid, dim3 block,
                           size_t lds_bytes, hipStream_t stream, const char** name,
                           const typename KernelArg<Args>::type&... args) {
  {
    std::lock_guard<std::mutex> lk(setup_mutex());
    if (!e.name[0]) format_name(e.name, sizeof(e.name));
  }
  if (lds_bytes > kMaxLdsBytes) return hipErrorInvalidValue;
  if (hipError_t err = ensure_max_lds(reinterpret_cast<const void*>(e.fn))) return err;
  if (name) *name = e.name;
  e.fn<<<grid, block, lds_bytes, stream>>>(args...);
  return hipGetLastError();
}

}  // namespace hfg
