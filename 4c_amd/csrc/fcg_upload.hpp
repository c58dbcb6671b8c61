// fcg_upload.hpp -- the one allocate-and-copy helper of the contexts' upload stages
// (fcg_context.cpp, fcg_tsi.hip).  Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace fcg {

// *dst = n elements on the current device, counted in `bytes`, holding src[0 .. n) (src == nullptr:
// left uninitialised); n <= 0: *dst = nullptr
template <class T>
hipError_t upload(T** dst, const T* src, int64_t n, int64_t& bytes)
{
  *dst = nullptr;
  if (n <= 0) return hipSuccess;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(dst), sizeof(T) * n);
  if (e != hipSuccess) return e;
  bytes += int64_t(sizeof(T)) * n;
  if (src) return hipMemcpy(*dst, src, sizeof(T) * n, hipMemcpyHostToDevice);
  return hipSuccess;
}

}  // namespace fcg
