// The per-element formulas of the quantized ops: step and zero point of the
// MIN_COMBINED quint8 mapping, the qint32 unit, and every float <-> quint8 /
// qint32 conversion. This is their one definition: the CPU kernels
// (kernels/cpu_quantized.cc) and the device code (kernels/hip/gemm_i8.hip,
// kernels/hip/quantized.hip) both call it, so the two sides run the same IEEE
// operations in the same order and precision (f32 for the quint8 paths, f64
// for the qint32 paths). A function in which a multiply feeds an add or a
// subtract turns contraction off in its own body: a pragma in the including
// file does not reach in here, and device code is contracted by default.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define STF_QHD __host__ __device__ inline
#else
#define STF_QHD inline
#endif

#if defined(__clang__)
#define STF_FP_CONTRACT_OFF _Pragma("clang fp contract(off)")
#else
#define STF_FP_CONTRACT_OFF
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

// Float value of one qint32 step of the range [mn, mx], in f64.
STF_QHD double QuantUnitI32(float mn, float mx) {
  return ((double)mx - mn) / 4294967295.0;
}

// QuantizeV2's quint8 of x with scale = 255 / (mx - mn). The clamps are
// std::min(255.f, std::max(0.f, q)) spelled as compares, NaN included. No
// operation here can contract.
STF_QHD uint8_t QuantizeU8(float x, float mn, float scale) {
  float q = roundf((x - mn) * scale);
  float lo = 0.f < q ? q : 0.f;       // std::max(0.f, q)
  float v = lo < 255.f ? lo : 255.f;  // std::min(255.f, .)
  return (uint8_t)v;
}

// The quint8 that QuantizeV2 assigns to the scalar x under [mn, mx],
// including its mx <= mn rule.
STF_QHD uint8_t QuantizeScalarU8(float x, float mn, float mx) {
  if (mx <= mn) mx = mn + 1e-6f;
  return QuantizeU8(x, mn, 255.f / (mx - mn));
}

// Dequantize of the quint8 q with step = QuantStep(mn, mx): two roundings.
STF_QHD float DequantizeU8(uint32_t q, float mn, float step) {
  STF_FP_CONTRACT_OFF
  return mn + (float)q * step;
}

// Dequantize of the qint32 p with scale = QuantUnitI32(mn, mx): the int32
// range maps onto [mn, mx].
STF_QHD float DequantizeI32(int32_t p, double scale, float mn) {
  STF_FP_CONTRACT_OFF
  return (float)(((double)p + 2147483648.0) * scale + mn);
}

// QuantizeDownAndShrinkRange's and Requantize's quint8 of the qint32 p: its
// f64 value p * unit under the range that starts at lo, with
// scale = 255 / (hi - lo).
STF_QHD uint8_t QuantizeDownI32(int32_t p, double unit, double lo,
                                double scale) {
  STF_FP_CONTRACT_OFF
  double v = round((p * unit - lo) * scale);
  double m = 0.0 < v ? v : 0.0;  // std::max(0.0, v)
  m = m < 255.0 ? m : 255.0;     // std::min(255.0, .)
  return (uint8_t)m;
}

// The range of a QuantizedBiasAdd result (symmetric, +-max_out) and the
// qint32 unit of that range, next to the two input mappings.
struct QuantBiasAddScale {
  float min_x, step_x, min_b, step_b, max_out;
  double unit;
};

STF_QHD QuantBiasAddScale MakeQuantBiasAddScale(float min_x, float max_x,
                                                float min_b, float max_b) {
  QuantBiasAddScale s;
  s.min_x = min_x;
  s.min_b = min_b;
  s.step_x = QuantStep(min_x, max_x);
  s.step_b = QuantStep(min_b, max_b);
  s.max_out = QuantBiasAddMax(min_x, max_x, min_b, max_b);
  s.unit = QuantUnitI32(-s.max_out, s.max_out);
  return s;
}

// round((fx + fb) / unit) with fx, fb the f32 values Dequantize gives. The
// f64 divide is part of the definition: a reciprocal multiply rounds
// differently.
STF_QHD int32_t QuantBiasAddI32(uint32_t x, uint32_t b,
                                const QuantBiasAddScale& s) {
  float fx = DequantizeU8(x, s.min_x, s.step_x);
  float fb = DequantizeU8(b, s.min_b, s.step_b);
  if (s.unit == 0) return 0;
  return (int32_t)round(((double)fx + (double)fb) / s.unit);
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
// [mn_out, mx_out]: Dequantize's f32 value, then QuantizeV2's formula.
STF_QHD uint8_t RequantizeU8(uint32_t q, float mn_in, float mx_in,
                             float mn_out, float mx_out) {
  float f = DequantizeU8(q, mn_in, QuantStep(mn_in, mx_in));
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
