// Step and zero point of the MIN_COMBINED quint8 mapping, shared by the CPU
// quantized kernels (kernels/cpu_quantized.cc) and the device code
// (kernels/hip/gemm_i8.hip, kernels/hip/quantized.hip) so both sides derive
// them with the same f32 operations.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define STF_QHD __host__ __device__ inline
#else
#define STF_QHD inline
#endif

namespace stf {

// Float value of one quint8 step of the range [mn, mx].
STF_QHD float QuantStep(float mn, float mx) { return (mx - mn) / 255.f; }

// The quantized value that represents 0.0. Unclamped: negative, or above
// 255, when the range excludes 0.
STF_QHD int32_t QuantZeroPoint(float mn, float mx) {
  float step = QuantStep(mn, mx);
  return (int32_t)lroundf(-mn / (step != 0 ? step : 1.f));
}

// Range of a qint32 product of two quint8 tensors: the int32 extremes in
// units of step_a * step_b.
STF_QHD float QuantProductMin(float step_a, float step_b) {
  return (float)(-2147483648.0 * (step_a * step_b));
}
STF_QHD float QuantProductMax(float step_a, float step_b) {
  return (float)(2147483647.0 * (step_a * step_b));
}

// Upper end of QuantizedBiasAdd's symmetric qint32 output range: 2^17 times
// the largest absolute value among the two input ranges.
STF_QHD float QuantBiasAddMax(float min_x, float max_x, float min_b,
                              float max_b) {
  float m = fabsf(min_x);
  float a = fabsf(max_x);
  m = m < a ? a : m;
  a = fabsf(min_b);
  m = m < a ? a : m;
  a = fabsf(max_b);
  m = m < a ? a : m;
  return m * 131072.f;
}

}  // namespace stf
