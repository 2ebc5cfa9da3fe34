// half_element.h -- the fp32 -> element rule the units that write fp16 share: kernels_features.hip (rene_export_features' fp16 tensors) and
// kernels_exr.hip and kernels_exr_passes.hip (rene_output_exr's and rene_output_exr_passes' HALF channels).  All are built with ROBUSTFLAGS (Makefile).
#pragma once
#include <hip/hip_runtime.h>

namespace rene {

template <class T>
__device__ __forceinline__ T to_element(float v);
template <>
__device__ __forceinline__ float to_element<float>(float v) {
  return v;
}
// clamped to the finite halves, then the conversion of the current rounding mode, which is round-to-nearest-even with fp16 subnormals kept
// (v_cvt_f16_f32; NOT the packed convert, which rounds toward zero).  The comparisons are false for a NaN, which stays one.
template <>
__device__ __forceinline__ _Float16 to_element<_Float16>(float v) {
  v = v > 65504.0f ? 65504.0f : (v < -65504.0f ? -65504.0f : v);
  return (_Float16)v;
}

}  // namespace rene
