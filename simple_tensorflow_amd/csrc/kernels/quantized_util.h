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

// The quint8 that QuantizeV2 assigns to the scalar x under [mn, mx],
// including its mx <= mn rule. No operation here can contract.
STF_QHD uint8_t QuantizeScalarU8(float x, float mn, float mx) {
  if (mx <= mn) mx = mn + 1e-6f;
  float scale = 255.f / (mx - mn);
  float q = roundf((x - mn) * scale);
  float lo = 0.f < q ? q : 0.f;       // std::max(0.f, q)
  float v = lo < 255.f ? lo : 255.f;  // std::min(255.f, .)
  return (uint8_t)v;
}

// QuantizedRelu6's clamp values. Unlike QuantizedRelu, which lets a zero
// point above 255 wrap into the byte, the floor is clamped to 0..255; the
// ceiling is the quint8 of 6.0.
STF_QHD int32_t QuantRelu6Floor(float mn, float mx) {
  int32_t z = QuantZeroPoint(mn, mx);
  return z < 0 ? 0 : (z > 255 ? 255 : z);
}
STF_QHD int32_t QuantRelu6Ceil(float mn, float mx) {
  return QuantizeScalarU8(6.0f, mn, mx);
}

// QuantizedConcat: the quint8 q of [mn_in, mx_in] expressed in
// [mn_out, mx_out]: Dequantize's f32 value, then QuantizeV2's formula. The
// multiply and the add stay two roundings on both devices.
STF_QHD uint8_t RequantizeU8(uint32_t q, float mn_in, float mx_in,
                             float mn_out, float mx_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float f = mn_in + (float)q * QuantStep(mn_in, mx_in);
  return QuantizeScalarU8(f, mn_out, mx_out);
}

// QuantizedConcat's output range, folded input by input in input order:
// min(0, min_i mn_i) and max_i mx_i. first starts the fold.
STF_QHD void QuantConcatRangeFold(float mn, float mx, bool first, float* lo,
                                  float* hi) {
  float l = first ? 0.f : *lo;
  *lo = mn < l ? mn : l;
  *hi = first ? mx : (*hi < mx ? mx : *hi);
}

}  // namespace stf
