// device_guard.h — makes a handle's device current for a scope and restores the caller's;
// shared by the generator's host units (handle.h) and the audio front end's (frontend_host.h).
#pragma once

#include <hip/hip_runtime.h>

namespace hfg_host {

struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (dev < 0) return;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

}  // namespace hfg_host
