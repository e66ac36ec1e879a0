// Elementwise and range kernels of the quantized ops: QuantizeV2,
// Dequantize, QuantizedRelu, RequantizationRange, QuantizeDownAndShrinkRange,
// Requantize, QuantizedBiasAdd, QuantizedMaxPool, QuantizedAvgPool,
// QuantizedRelu6, QuantizedConcat.
//
// Every output is bit-equal to kernels/cpu_quantized.cc. The per-element
// formulas are not written here: both sides call the one definition in
// kernels/quantized_util.h, which keeps its own multiplies and adds from
// contracting; contraction is off in this file as well, for the range
// arithmetic that stays here. The ranges are device scalars, read through
// pointers and written by the kernels, so a chain of quantized layers never
// synchronises with the host.
#include "hip_common.h"
#include "kernels/quantized_util.h"
#include "stf_kernels.h"

#pragma clang fp contract(off)

namespace {

// The calling thread's first index and step in a grid-stride loop.
struct GridThread {
  int64_t tid, stride;
};

// The block size comes from the builtin: blockDim.x, read outside a
// __global__ function, compiles to the lookup that allows for a partial last
// block, which costs every kernel a global load in its prologue.
__device__ __forceinline__ GridThread ThisThread() {
  uint32_t block = __builtin_amdgcn_workgroup_size_x();
  return {(int64_t)blockIdx.x * block + threadIdx.x,
          (int64_t)gridDim.x * block};
}

// Thread 0 of the grid writes the op's two output range scalars.
__device__ __forceinline__ void WriteRanges(const GridThread& t,
                                            float* out_mn, float* out_mx,
                                            float mn, float mx) {
  if (t.tid == 0) {
    out_mn[0] = mn;
    out_mx[0] = mx;
  }
}

__global__ void QuantizeV2Kernel(const float* __restrict__ x,
                                 const float* __restrict__ mnp,
                                 const float* __restrict__ mxp,
                                 uint8_t* __restrict__ y,
                                 float* __restrict__ out_mn,
                                 float* __restrict__ out_mx, int64_t n) {
  float mn = mnp[0], mx = mxp[0];
  if (mx <= mn) mx = mn + 1e-6f;
  float scale = 255.f / (mx - mn);
  GridThread t = ThisThread();
  WriteRanges(t, out_mn, out_mx, mn, mx);
  int64_t n4 = n / 4;
  for (int64_t i = t.tid; i < n4; i += t.stride) {
    float4 v = ((const float4*)x)[i];
    uint32_t w = (uint32_t)stf::QuantizeU8(v.x, mn, scale) |
                 (uint32_t)stf::QuantizeU8(v.y, mn, scale) << 8 |
                 (uint32_t)stf::QuantizeU8(v.z, mn, scale) << 16 |
                 (uint32_t)stf::QuantizeU8(v.w, mn, scale) << 24;
    ((uint32_t*)y)[i] = w;
  }
  for (int64_t i = n4 * 4 + t.tid; i < n; i += t.stride)
    y[i] = stf::QuantizeU8(x[i], mn, scale);
}

__global__ void DequantizeU8Kernel(const uint8_t* __restrict__ x,
                                   const float* __restrict__ mnp,
                                   const float* __restrict__ mxp,
                                   float* __restrict__ y, int64_t n) {
  float mn = mnp[0];
  float step = stf::QuantStep(mn, mxp[0]);
  GridThread t = ThisThread();
  int64_t n4 = n / 4;
  for (int64_t i = t.tid; i < n4; i += t.stride) {
    uint32_t w = ((const uint32_t*)x)[i];
    float4 o;
    o.x = stf::DequantizeU8(w & 0xff, mn, step);
    o.y = stf::DequantizeU8((w >> 8) & 0xff, mn, step);
    o.z = stf::DequantizeU8((w >> 16) & 0xff, mn, step);
    o.w = stf::DequantizeU8(w >> 24, mn, step);
    ((float4*)y)[i] = o;
  }
  for (int64_t i = n4 * 4 + t.tid; i < n; i += t.stride)
    y[i] = stf::DequantizeU8(x[i], mn, step);
}

__global__ void DequantizeI32Kernel(const int32_t* __restrict__ x,
                                    const float* __restrict__ mnp,
                                    const float* __restrict__ mxp,
                                    float* __restrict__ y, int64_t n) {
  float mn = mnp[0];
  double scale = stf::QuantUnitI32(mn, mxp[0]);
  GridThread t = ThisThread();
  int64_t n4 = n / 4;
  for (int64_t i = t.tid; i < n4; i += t.stride) {
    int4 v = ((const int4*)x)[i];
    float4 o;
    o.x = stf::DequantizeI32(v.x, scale, mn);
    o.y = stf::DequantizeI32(v.y, scale, mn);
    o.z = stf::DequantizeI32(v.z, scale, mn);
    o.w = stf::DequantizeI32(v.w, scale, mn);
    ((float4*)y)[i] = o;
  }
  for (int64_t i = n4 * 4 + t.tid; i < n; i += t.stride)
    y[i] = stf::DequantizeI32(x[i], scale, mn);
}

// max per byte of the four u8 lanes of a word against one floor value
__device__ __forceinline__ uint32_t MaxU8x4(uint32_t w, int32_t floor_q) {
  uint32_t o = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    int32_t p = (int32_t)((w >> (8 * b)) & 0xff);
    o |= (uint32_t)(uint8_t)(p > floor_q ? p : floor_q) << (8 * b);
  }
  return o;
}

__global__ void QuantizedReluKernel(const uint8_t* __restrict__ x,
                                    const float* __restrict__ mnp,
                                    const float* __restrict__ mxp,
                                    uint8_t* __restrict__ y,
                                    float* __restrict__ out_mn,
                                    float* __restrict__ out_mx, int64_t n) {
  float mn = mnp[0], mx = mxp[0];
  int32_t zero_q = stf::QuantZeroPoint(mn, mx);
  int32_t floor_q = zero_q > 0 ? zero_q : 0;
  GridThread t = ThisThread();
  WriteRanges(t, out_mn, out_mx, mn, mx);
  int64_t n16 = n / 16;
  for (int64_t i = t.tid; i < n16; i += t.stride) {
    uint4 v = ((const uint4*)x)[i];
    v.x = MaxU8x4(v.x, floor_q);
    v.y = MaxU8x4(v.y, floor_q);
    v.z = MaxU8x4(v.z, floor_q);
    v.w = MaxU8x4(v.w, floor_q);
    ((uint4*)y)[i] = v;
  }
  for (int64_t i = n16 * 16 + t.tid; i < n; i += t.stride) {
    int32_t p = x[i];
    y[i] = (uint8_t)(p > floor_q ? p : floor_q);
  }
}

// lohi[0] = min(lohi[0], min x), lohi[1] = max(lohi[1], max x); the caller
// zeroes lohi on the stream first, which is the CPU loops' starting value.
__global__ void MinMaxI32Kernel(const int32_t* __restrict__ x,
                                int32_t* __restrict__ lohi, int64_t n) {
  __shared__ int32_t slo[4], shi[4];
  GridThread t = ThisThread();
  int32_t lo = 0, hi = 0;
  int64_t n4 = n / 4;
  for (int64_t i = t.tid; i < n4; i += t.stride) {
    int4 v = ((const int4*)x)[i];
    lo = min(lo, min(min(v.x, v.y), min(v.z, v.w)));
    hi = max(hi, max(max(v.x, v.y), max(v.z, v.w)));
  }
  for (int64_t i = n4 * 4 + t.tid; i < n; i += t.stride) {
    lo = min(lo, x[i]);
    hi = max(hi, x[i]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = min(lo, __shfl_xor(lo, off));
    hi = max(hi, __shfl_xor(hi, off));
  }
  int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    slo[wid] = lo;
    shi[wid] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    lo = min(min(slo[0], slo[1]), min(slo[2], slo[3]));
    hi = max(max(shi[0], shi[1]), max(shi[2], shi[3]));
    if (lo < 0) atomicMin(&lohi[0], lo);
    if (hi > 0) atomicMax(&lohi[1], hi);
  }
}

__global__ void RequantRangeKernel(const int32_t* __restrict__ lohi,
                                   const float* __restrict__ mnp,
                                   const float* __restrict__ mxp,
                                   float* __restrict__ out_mn,
                                   float* __restrict__ out_mx) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double unit = stf::QuantUnitI32(mnp[0], mxp[0]);
  out_mn[0] = (float)(lohi[0] * unit);
  out_mx[0] = (float)(lohi[1] * unit);
}

// The CPU code takes min/max over x[i] * unit starting from 0.0. x -> x *
// unit is monotone (either way, by the sign of unit), so the extremes are
// reached at the integer extremes.
__device__ __forceinline__ void ShrunkRange(const int32_t* lohi, double unit,
                                            double* lo, double* hi) {
  double a = lohi[0] * unit, b = lohi[1] * unit;
  double l = 0, h = 0;
  l = a < l ? a : l;
  l = b < l ? b : l;
  h = h < a ? a : h;
  h = h < b ? b : h;
  if (h <= l) h = l + 1e-6;
  *lo = l;
  *hi = h;
}

__device__ __forceinline__ uint32_t QuantizeDownFour(int4 v, double unit,
                                                     double lo,
                                                     double scale) {
  return (uint32_t)stf::QuantizeDownI32(v.x, unit, lo, scale) |
         (uint32_t)stf::QuantizeDownI32(v.y, unit, lo, scale) << 8 |
         (uint32_t)stf::QuantizeDownI32(v.z, unit, lo, scale) << 16 |
         (uint32_t)stf::QuantizeDownI32(v.w, unit, lo, scale) << 24;
}

__global__ void QuantizeDownKernel(const int32_t* __restrict__ x,
                                   const int32_t* __restrict__ lohi,
                                   const float* __restrict__ mnp,
                                   const float* __restrict__ mxp,
                                   uint8_t* __restrict__ y,
                                   float* __restrict__ out_mn,
                                   float* __restrict__ out_mx, int64_t n) {
  double unit = stf::QuantUnitI32(mnp[0], mxp[0]);
  double lo, hi;
  ShrunkRange(lohi, unit, &lo, &hi);
  double scale = 255.0 / (hi - lo);
  GridThread t = ThisThread();
  WriteRanges(t, out_mn, out_mx, (float)lo, (float)hi);
  int64_t n4 = n / 4;
  for (int64_t i = t.tid; i < n4; i += t.stride)
    ((uint32_t*)y)[i] =
        QuantizeDownFour(((const int4*)x)[i], unit, lo, scale);
  for (int64_t i = n4 * 4 + t.tid; i < n; i += t.stride)
    y[i] = stf::QuantizeDownI32(x[i], unit, lo, scale);
}

// QuantizeDownKernel with the range given: no reduction in front of it. A
// thread takes 16 consecutive elements, four 16-byte loads and one 16-byte
// store.
__global__ void RequantizeKernel(const int32_t* __restrict__ x,
                                 const float* __restrict__ mnp,
                                 const float* __restrict__ mxp,
                                 const float* __restrict__ req_mn,
                                 const float* __restrict__ req_mx,
                                 uint8_t* __restrict__ y,
                                 float* __restrict__ out_mn,
                                 float* __restrict__ out_mx, int64_t n) {
  double unit = stf::QuantUnitI32(mnp[0], mxp[0]);
  double lo = (double)req_mn[0], hi = (double)req_mx[0];
  if (hi <= lo) hi = lo + 1e-6;
  double scale = 255.0 / (hi - lo);
  GridThread t = ThisThread();
  WriteRanges(t, out_mn, out_mx, (float)lo, (float)hi);
  int64_t n16 = n / 16;
  for (int64_t i = t.tid; i < n16; i += t.stride) {
    const int4* src = (const int4*)x + i * 4;
    int4 a = src[0], b = src[1], c = src[2], d = src[3];
    uint4 o;
    o.x = QuantizeDownFour(a, unit, lo, scale);
    o.y = QuantizeDownFour(b, unit, lo, scale);
    o.z = QuantizeDownFour(c, unit, lo, scale);
    o.w = QuantizeDownFour(d, unit, lo, scale);
    ((uint4*)y)[i] = o;
  }
  for (int64_t i = n16 * 16 + t.tid; i < n; i += t.stride)
    y[i] = stf::QuantizeDownI32(x[i], unit, lo, scale);
}

// x viewed as [rows, C]. VEC: C % 4 == 0 and a thread takes 4 consecutive
// channels (n4 = rows * C / 4 groups); otherwise one element per thread.
template <bool VEC>
__global__ void QuantizedBiasAddKernel(const uint8_t* __restrict__ x,
                                       const uint8_t* __restrict__ bias,
                                       const float* __restrict__ min_x,
                                       const float* __restrict__ max_x,
                                       const float* __restrict__ min_b,
                                       const float* __restrict__ max_b,
                                       int32_t* __restrict__ y,
                                       float* __restrict__ out_mn,
                                       float* __restrict__ out_mx,
                                       int64_t total, int64_t C) {
  stf::QuantBiasAddScale s =
      stf::MakeQuantBiasAddScale(min_x[0], max_x[0], min_b[0], max_b[0]);
  GridThread t = ThisThread();
  WriteRanges(t, out_mn, out_mx, -s.max_out, s.max_out);
  if (VEC) {
    int64_t c4 = C / 4;
    for (int64_t i = t.tid; i < total; i += t.stride) {
      uint32_t xv = ((const uint32_t*)x)[i];
      uint32_t bv = ((const uint32_t*)bias)[i % c4];
      int4 o;
      o.x = stf::QuantBiasAddI32(xv & 0xff, bv & 0xff, s);
      o.y = stf::QuantBiasAddI32((xv >> 8) & 0xff, (bv >> 8) & 0xff, s);
      o.z = stf::QuantBiasAddI32((xv >> 16) & 0xff, (bv >> 16) & 0xff, s);
      o.w = stf::QuantBiasAddI32(xv >> 24, bv >> 24, s);
      ((int4*)y)[i] = o;
    }
  } else {
    for (int64_t i = t.tid; i < total; i += t.stride)
      y[i] = stf::QuantBiasAddI32(x[i], bias[i % C], s);
  }
}

using u16x2 = __attribute__((ext_vector_type(2))) unsigned short;

// max of the two u16 halves of a word
__device__ __forceinline__ uint32_t PkMaxU16(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(
      uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a),
                                          __builtin_bit_cast(u16x2, b)));
}

// Byte-wise running maximum of 4 u8 lanes, kept as the even and the odd
// bytes widened to u16 pairs so that each tap costs two packed maxima.
struct MaxU8x4Acc {
  uint32_t even = 0, odd = 0;
  __device__ __forceinline__ void Take(uint32_t w) {
    even = PkMaxU16(even, w & 0x00ff00ffu);
    odd = PkMaxU16(odd, (w >> 8) & 0x00ff00ffu);
  }
  __device__ __forceinline__ uint32_t Word() const {
    return even | odd << 8;
  }
};

__device__ __forceinline__ void PoolWindow(const StfPoolGeom& g, int p, int q,
                                           int* h0, int* h1, int* w0,
                                           int* w1) {
  *h0 = max(p * g.sh - g.ph, 0);
  *h1 = min(p * g.sh - g.ph + g.kh, g.H);
  *w0 = max(q * g.sw - g.pw, 0);
  *w1 = min(q * g.sw - g.pw + g.kw, g.W);
}

// Sums of the four u8 lanes of a word, in 32 bits: 255 * taps overflows 16
// bits once a window has more than 257 taps, and 32 bits hold any window.
__device__ __forceinline__ void AddU8x4(uint32_t w, uint32_t* acc) {
#pragma unroll
  for (int b = 0; b < 4; ++b) acc[b] += (w >> (8 * b)) & 0xff;
}

__device__ __forceinline__ void AddU8x16(uint4 v, uint32_t* acc) {
  AddU8x4(v.x, acc);
  AddU8x4(v.y, acc + 4);
  AddU8x4(v.z, acc + 8);
  AddU8x4(v.w, acc + 12);
}

// The integer division is the CPU kernel's: a float reciprocal turns
// 255 * cnt / cnt into 254 for some counts.
__device__ __forceinline__ uint32_t DivU8x4(const uint32_t* acc,
                                            uint32_t cnt) {
  uint32_t o = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) o |= (acc[b] / cnt) << (8 * b);
  return o;
}

// Taps of the clipped window; never 0 for a valid geometry, and 1 keeps the
// division defined where it would be.
__device__ __forceinline__ uint32_t PoolTaps(int h0, int h1, int w0, int w1) {
  int cnt = max(h1 - h0, 0) * max(w1 - w0, 0);
  return cnt > 0 ? (uint32_t)cnt : 1u;
}

// The reducers of QuantizedPoolKernel, for G = 16 or 1 channels per thread.
// State starts zeroed. Row() takes the taps w0..w1-1 of the image row whose
// first pixel is pixel `pix` of x, at the thread's channel offset c; Store()
// writes the G results of output group i, given the window's tap count. The
// functions are static and the kernel holds the State as a plain local: as
// members of a reducer object, PoolAvg<16>'s sums are split up differently by
// the compiler, and the kernel needs 72 VGPRs or more where it has 63.
template <int G>
struct PoolMax;

template <>
struct PoolMax<16> {
  using State = MaxU8x4Acc[4];
  static __device__ __forceinline__ void Row(State& a, const uint8_t* x,
                                             int64_t pix, int64_t c, int w0,
                                             int w1, int C) {
    for (int iw = w0; iw < w1; ++iw) {
      uint4 v = *(const uint4*)(x + (pix + iw) * C + c);
      a[0].Take(v.x);
      a[1].Take(v.y);
      a[2].Take(v.z);
      a[3].Take(v.w);
    }
  }
  static __device__ __forceinline__ void Store(const State& a, uint8_t* y,
                                               int64_t i, uint32_t) {
    ((uint4*)y)[i] = uint4{a[0].Word(), a[1].Word(), a[2].Word(), a[3].Word()};
  }
};

template <>
struct PoolMax<1> {
  using State = uint32_t;
  static __device__ __forceinline__ void Row(State& best, const uint8_t* x,
                                             int64_t pix, int64_t c, int w0,
                                             int w1, int C) {
    for (int iw = w0; iw < w1; ++iw) {
      uint32_t v = x[(pix + iw) * C + c];
      best = best < v ? v : best;
    }
  }
  static __device__ __forceinline__ void Store(const State& best, uint8_t* y,
                                               int64_t i, uint32_t) {
    y[i] = (uint8_t)best;
  }
};

template <int G>
struct PoolAvg;

template <>
struct PoolAvg<16> {
  using State = uint32_t[16];
  // Four taps of a row at a time, their loads issued before the first sum so
  // that they are in flight together: a global-pool head (8x8 on 2048
  // channels) has few threads with 64 taps each and is bound by the latency
  // of a tap's load.
  static __device__ __forceinline__ void Row(State& acc, const uint8_t* x,
                                             int64_t pix, int64_t c, int w0,
                                             int w1, int C) {
    const uint8_t* row = x + pix * C + c;
    int iw = w0;
    for (; iw + 4 <= w1; iw += 4) {
      const uint8_t* t = row + (int64_t)iw * C;
      uint4 v0 = *(const uint4*)t;
      uint4 v1 = *(const uint4*)(t + C);
      uint4 v2 = *(const uint4*)(t + 2 * (int64_t)C);
      uint4 v3 = *(const uint4*)(t + 3 * (int64_t)C);
      AddU8x16(v0, acc);
      AddU8x16(v1, acc);
      AddU8x16(v2, acc);
      AddU8x16(v3, acc);
    }
    for (; iw < w1; ++iw)
      AddU8x16(*(const uint4*)(row + (int64_t)iw * C), acc);
  }
  static __device__ __forceinline__ void Store(const State& acc, uint8_t* y,
                                               int64_t i, uint32_t taps) {
    ((uint4*)y)[i] = uint4{DivU8x4(acc, taps), DivU8x4(acc + 4, taps),
                           DivU8x4(acc + 8, taps), DivU8x4(acc + 12, taps)};
  }
};

template <>
struct PoolAvg<1> {
  using State = uint32_t;
  static __device__ __forceinline__ void Row(State& sum, const uint8_t* x,
                                             int64_t pix, int64_t c, int w0,
                                             int w1, int C) {
    for (int iw = w0; iw < w1; ++iw) sum += x[(pix + iw) * C + c];
  }
  static __device__ __forceinline__ void Store(const State& sum, uint8_t* y,
                                               int64_t i, uint32_t taps) {
    y[i] = (uint8_t)(sum / taps);
  }
};

// The NHWC quint8 pools. A thread owns G channels of one output pixel: 16
// when C % 16 == 0, else 1; `total` counts those groups. The window is
// clipped to the image, so every tap that is read lies inside it. Both pools
// pass their ranges through.
template <template <int> class Reducer, int G>
__global__ void QuantizedPoolKernel(const uint8_t* __restrict__ x,
                                    const float* __restrict__ mnp,
                                    const float* __restrict__ mxp,
                                    uint8_t* __restrict__ y,
                                    float* __restrict__ out_mn,
                                    float* __restrict__ out_mx,
                                    StfPoolGeom g, int64_t total) {
  GridThread t = ThisThread();
  WriteRanges(t, out_mn, out_mx, mnp[0], mxp[0]);
  int64_t groups = g.C / G;
  for (int64_t i = t.tid; i < total; i += t.stride) {
    int64_t rem = i;
    int64_t c = rem % groups; rem /= groups;
    int q = (int)(rem % g.Q); rem /= g.Q;
    int p = (int)(rem % g.P); rem /= g.P;
    int64_t n = rem;
    int h0, h1, w0, w1;
    PoolWindow(g, p, q, &h0, &h1, &w0, &w1);
    typename Reducer<G>::State r{};
    for (int ih = h0; ih < h1; ++ih)
      Reducer<G>::Row(r, x, (n * g.H + ih) * g.W, c * G, w0, w1, g.C);
    // ((n * P + p) * Q + q) * C + c * G == i * G
    Reducer<G>::Store(r, y, i, PoolTaps(h0, h1, w0, w1));
  }
}

__device__ __forceinline__ uint32_t PkMinU16(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(
      uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a),
                                          __builtin_bit_cast(u16x2, b)));
}

// min(max(., lo), hi) per byte of a word; lo2 and hi2 hold the clamp value
// in both u16 halves, and the even and the odd bytes go through as u16
// pairs (MaxU8x4Acc's scheme).
__device__ __forceinline__ uint32_t ClampU8x4(uint32_t w, uint32_t lo2,
                                              uint32_t hi2) {
  uint32_t even = PkMinU16(PkMaxU16(w & 0x00ff00ffu, lo2), hi2);
  uint32_t odd = PkMinU16(PkMaxU16((w >> 8) & 0x00ff00ffu, lo2), hi2);
  return even | odd << 8;
}

// QuantizedReluKernel's scheme with a ceiling as well as a floor. Both clamp
// values lie in 0..255 (kernels/quantized_util.h): QuantizedRelu wraps a
// zero point above 255 into the byte, Relu6 clamps it.
__global__ void QuantizedRelu6Kernel(const uint8_t* __restrict__ x,
                                     const float* __restrict__ mnp,
                                     const float* __restrict__ mxp,
                                     uint8_t* __restrict__ y,
                                     float* __restrict__ out_mn,
                                     float* __restrict__ out_mx, int64_t n) {
  float mn = mnp[0], mx = mxp[0];
  int32_t lo = stf::QuantRelu6Floor(mn, mx);
  int32_t hi = stf::QuantRelu6Ceil(mn, mx);
  uint32_t lo2 = (uint32_t)lo | (uint32_t)lo << 16;
  uint32_t hi2 = (uint32_t)hi | (uint32_t)hi << 16;
  GridThread t = ThisThread();
  WriteRanges(t, out_mn, out_mx, mn, mx);
  int64_t n16 = n / 16;
  for (int64_t i = t.tid; i < n16; i += t.stride) {
    uint4 v = ((const uint4*)x)[i];
    v.x = ClampU8x4(v.x, lo2, hi2);
    v.y = ClampU8x4(v.y, lo2, hi2);
    v.z = ClampU8x4(v.z, lo2, hi2);
    v.w = ClampU8x4(v.w, lo2, hi2);
    ((uint4*)y)[i] = v;
  }
  for (int64_t i = n16 * 16 + t.tid; i < n; i += t.stride) {
    int32_t p = x[i];
    p = p > lo ? p : lo;
    y[i] = (uint8_t)(p < hi ? p : hi);
  }
}

// One thread folds a chunk's ranges into the two output scalars, in input
// order, as the CPU kernel does.
__global__ void QuantizedConcatRangeKernel(StfQuantConcatArgs a, int first,
                                           float* __restrict__ out_mn,
                                           float* __restrict__ out_mx) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float lo = 0.f, hi = 0.f;
  if (!first) {
    lo = out_mn[0];
    hi = out_mx[0];
  }
  for (int k = 0; k < a.n; ++k)
    stf::QuantConcatRangeFold(a.mn[k][0], a.mx[k][0], first && k == 0, &lo,
                              &hi);
  out_mn[0] = lo;
  out_mx[0] = hi;
}

__device__ __forceinline__ uint32_t LutU8x4(const uint8_t* lut, uint32_t w) {
  return (uint32_t)lut[w & 0xff] | (uint32_t)lut[(w >> 8) & 0xff] << 8 |
         (uint32_t)lut[(w >> 16) & 0xff] << 16 |
         (uint32_t)lut[w >> 24] << 24;
}

// blockIdx.y picks the input of the chunk, blockIdx.x strides over its
// [outer, inner] bytes; the block must have 256 threads. Each block first
// builds its input's 256-entry table in LDS with the helper the CPU kernel
// uses (RequantizeU8), one entry per thread, so the f32 work is done 256
// times per block instead of once per byte and bit-equality with the CPU
// needs no care in the copy loop. The table is one 256-byte LDS bank row: two
// lookups conflict only on the same dword, which broadcasts. An input whose
// range equals the output range (f32 == on both ends) is copied as it is,
// which is the specified result and not the table's: requantizing under the
// degenerate range (0, 0) would map every byte to 0.
// VEC: every inner, column offset and pointer is a multiple of 16, and a
// thread moves 16 bytes; otherwise one byte.
template <bool VEC>
__global__ void __launch_bounds__(256)
QuantizedConcatCopyKernel(StfQuantConcatArgs a,
                          const float* __restrict__ out_mn,
                          const float* __restrict__ out_mx,
                          uint8_t* __restrict__ y, int64_t outer,
                          int64_t out_row) {
  __shared__ __attribute__((aligned(256))) uint8_t lut[256];
  int k = blockIdx.y;
  int64_t width = VEC ? a.inner[k] / 16 : a.inner[k];
  int64_t units = outer * width;
  // uniform over the block: no thread of it has work
  if ((int64_t)blockIdx.x * blockDim.x >= units) return;
  float mn = a.mn[k][0], mx = a.mx[k][0];
  float lo = out_mn[0], hi = out_mx[0];
  bool copy = mn == lo && mx == hi;
  lut[threadIdx.x] = stf::RequantizeU8(threadIdx.x, mn, mx, lo, hi);
  __syncthreads();
  const uint8_t* __restrict__ src = a.src[k];
  uint8_t* __restrict__ dst = y + a.off[k];
  GridThread t = ThisThread();
  for (int64_t i = t.tid; i < units; i += t.stride) {
    int64_t row = i / width, col = i - row * width;
    if (VEC) {
      uint4 v = ((const uint4*)src)[i];
      if (!copy) {
        v.x = LutU8x4(lut, v.x);
        v.y = LutU8x4(lut, v.y);
        v.z = LutU8x4(lut, v.z);
        v.w = LutU8x4(lut, v.w);
      }
      *(uint4*)(dst + row * out_row + col * 16) = v;
    } else {
      uint8_t v = src[i];
      dst[row * out_row + col] = copy ? v : lut[v];
    }
  }
}

hipError_t MinMaxI32(const int32_t* x, int32_t* lohi, int64_t n,
                     hipStream_t stream) {
  hipError_t e = hipMemsetAsync(lohi, 0, 2 * sizeof(int32_t), stream);
  if (e != hipSuccess) return e;
  if (n > 0)
    hipLaunchKernelGGL(MinMaxI32Kernel, ElemwiseGrid(n), dim3(256), 0, stream,
                       x, lohi, n);
  return hipGetLastError();
}

template <template <int> class Reducer>
hipError_t QuantizedPool(const uint8_t* x, const float* mn, const float* mx,
                         uint8_t* y, float* out_mn, float* out_mx,
                         const StfPoolGeom* gp, hipStream_t stream) {
  const StfPoolGeom g = *gp;
  int64_t total = (int64_t)g.N * g.P * g.Q * g.C;
  if (g.C > 0 && g.C % 16 == 0)
    hipLaunchKernelGGL((QuantizedPoolKernel<Reducer, 16>),
                       ElemwiseGrid(total / 16, 256, 1), dim3(256), 0, stream,
                       x, mn, mx, y, out_mn, out_mx, g, total / 16);
  else
    hipLaunchKernelGGL((QuantizedPoolKernel<Reducer, 1>),
                       ElemwiseGrid(total, 256, 1), dim3(256), 0, stream, x,
                       mn, mx, y, out_mn, out_mx, g, total);
  return hipGetLastError();
}

}  // namespace

extern "C" hipError_t stf_quantize_v2(const float* x, const float* mn,
                                      const float* mx, uint8_t* y,
                                      float* out_mn, float* out_mx, int64_t n,
                                      hipStream_t stream) {
  hipLaunchKernelGGL(QuantizeV2Kernel, ElemwiseGrid(n), dim3(256), 0, stream,
                     x, mn, mx, y, out_mn, out_mx, n);
  return hipGetLastError();
}

extern "C" hipError_t stf_dequantize(int in_i32, const void* x,
                                     const float* mn, const float* mx,
                                     float* y, int64_t n,
                                     hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (in_i32)
    hipLaunchKernelGGL(DequantizeI32Kernel, ElemwiseGrid(n), dim3(256), 0,
                       stream, (const int32_t*)x, mn, mx, y, n);
  else
    hipLaunchKernelGGL(DequantizeU8Kernel, ElemwiseGrid(n), dim3(256), 0,
                       stream, (const uint8_t*)x, mn, mx, y, n);
  return hipGetLastError();
}

extern "C" hipError_t stf_quantized_relu(const uint8_t* x, const float* mn,
                                         const float* mx, uint8_t* y,
                                         float* out_mn, float* out_mx,
                                         int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(QuantizedReluKernel, ElemwiseGrid(n, 256, 16), dim3(256),
                     0, stream, x, mn, mx, y, out_mn, out_mx, n);
  return hipGetLastError();
}

extern "C" hipError_t stf_requantization_range(
    const int32_t* x, const float* mn, const float* mx, int32_t* lohi,
    float* out_mn, float* out_mx, int64_t n, hipStream_t stream) {
  hipError_t e = MinMaxI32(x, lohi, n, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(RequantRangeKernel, dim3(1), dim3(64), 0, stream, lohi,
                     mn, mx, out_mn, out_mx);
  return hipGetLastError();
}

extern "C" hipError_t stf_quantize_down(const int32_t* x, const float* mn,
                                        const float* mx, int32_t* lohi,
                                        uint8_t* y, float* out_mn,
                                        float* out_mx, int64_t n,
                                        hipStream_t stream) {
  hipError_t e = MinMaxI32(x, lohi, n, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(QuantizeDownKernel, ElemwiseGrid(n), dim3(256), 0,
                     stream, x, lohi, mn, mx, y, out_mn, out_mx, n);
  return hipGetLastError();
}

// The three entries below launch for an empty tensor too: thread 0 writes
// the output ranges.
extern "C" hipError_t stf_requantize(const int32_t* x, const float* mn,
                                     const float* mx, const float* req_mn,
                                     const float* req_mx, uint8_t* y,
                                     float* out_mn, float* out_mx, int64_t n,
                                     hipStream_t stream) {
  hipLaunchKernelGGL(RequantizeKernel, ElemwiseGrid(n, 256, 16), dim3(256), 0,
                     stream, x, mn, mx, req_mn, req_mx, y, out_mn, out_mx, n);
  return hipGetLastError();
}

extern "C" hipError_t stf_quantized_bias_add(
    const uint8_t* x, const uint8_t* bias, const float* min_x,
    const float* max_x, const float* min_b, const float* max_b, int32_t* y,
    float* out_mn, float* out_mx, int64_t rows, int64_t C,
    hipStream_t stream) {
  int64_t n = rows * C;
  if (C > 0 && C % 4 == 0)
    hipLaunchKernelGGL(QuantizedBiasAddKernel<true>,
                       ElemwiseGrid(n / 4, 256, 1),
                       dim3(256), 0, stream, x, bias, min_x, max_x, min_b,
                       max_b, y, out_mn, out_mx, n / 4, C);
  else
    hipLaunchKernelGGL(QuantizedBiasAddKernel<false>, ElemwiseGrid(n),
                       dim3(256), 0, stream, x, bias, min_x, max_x, min_b,
                       max_b, y, out_mn, out_mx, n, C);
  return hipGetLastError();
}

extern "C" hipError_t stf_quantized_max_pool(const uint8_t* x,
                                             const float* mn, const float* mx,
                                             uint8_t* y, float* out_mn,
                                             float* out_mx,
                                             const StfPoolGeom* gp,
                                             hipStream_t stream) {
  return QuantizedPool<PoolMax>(x, mn, mx, y, out_mn, out_mx, gp, stream);
}

extern "C" hipError_t stf_quantized_avg_pool(const uint8_t* x,
                                             const float* mn, const float* mx,
                                             uint8_t* y, float* out_mn,
                                             float* out_mx,
                                             const StfPoolGeom* gp,
                                             hipStream_t stream) {
  return QuantizedPool<PoolAvg>(x, mn, mx, y, out_mn, out_mx, gp, stream);
}

extern "C" hipError_t stf_quantized_relu6(const uint8_t* x, const float* mn,
                                          const float* mx, uint8_t* y,
                                          float* out_mn, float* out_mx,
                                          int64_t n, hipStream_t stream) {
  // Two 16-byte groups per thread: a thread's prologue has one f32 divide
  // more than QuantizedRelu's (profiles/quantized_inception.md).
  hipLaunchKernelGGL(QuantizedRelu6Kernel, ElemwiseGrid(n, 256, 32),
                     dim3(256), 0, stream, x, mn, mx, y, out_mn, out_mx, n);
  return hipGetLastError();
}

extern "C" hipError_t stf_quantized_concat_range(const StfQuantConcatArgs* a,
                                                 int first, float* out_mn,
                                                 float* out_mx,
                                                 hipStream_t stream) {
  if (a->n < 1 || a->n > kStfQuantConcatMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(QuantizedConcatRangeKernel, dim3(1), dim3(64), 0, stream,
                     *a, first, out_mn, out_mx);
  return hipGetLastError();
}

extern "C" hipError_t stf_quantized_concat_copy(const StfQuantConcatArgs* a,
                                                const float* out_mn,
                                                const float* out_mx,
                                                uint8_t* y, int64_t outer,
                                                int64_t out_row,
                                                hipStream_t stream) {
  if (a->n < 1 || a->n > kStfQuantConcatMax) return hipErrorInvalidValue;
  bool vec = ((uintptr_t)y & 15) == 0 && out_row % 16 == 0;
  int64_t widest = 0;
  for (int k = 0; k < a->n; ++k) {
    vec = vec && a->inner[k] % 16 == 0 && a->off[k] % 16 == 0 &&
          ((uintptr_t)a->src[k] & 15) == 0;
    widest = a->inner[k] > widest ? a->inner[k] : widest;
  }
  int64_t units = outer * (vec ? widest / 16 : widest);
  if (units <= 0) return hipSuccess;
  dim3 grid(ElemwiseGrid(units, 256, 4).x, (uint32_t)a->n);
  if (vec)
    hipLaunchKernelGGL(QuantizedConcatCopyKernel<true>, grid, dim3(256), 0,
                       stream, *a, out_mn, out_mx, y, outer, out_row);
  else
    hipLaunchKernelGGL(QuantizedConcatCopyKernel<false>, grid, dim3(256), 0,
                       stream, *a, out_mn, out_mx, y, outer, out_row);
  return hipGetLastError();
}
