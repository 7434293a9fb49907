// Host launch helpers shared by the GEMM files.
#pragma once
#include <hip/hip_runtime.h>

namespace pa {

// Launch of a kernel whose dynamic LDS exceeds the 64 KiB default: the opt-in attribute is set by a function-local
// static initialiser (thread-safe, once per kernel) and a failure of it is returned instead of launching.
// Once per process, not per device: the project runs one process per GPU.
template <auto Kern, class... Args>
int launch_lds(dim3 grid, dim3 block, int smem, hipStream_t st, const Args&... args) {
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
  if (attr != hipSuccess) return (int)attr;
  hipLaunchKernelGGL(Kern, grid, block, smem, st, args...);
  return (int)hipGetLastError();
}

// Compute units of the current device (256 when the query fails): the wave size of the balanced-tail plan.
inline int device_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    return hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
  }();
  return cus;
}

}  // namespace pa
