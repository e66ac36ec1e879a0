// Quantized (quint8 x quint8 -> qint32) GEMM and Conv2D for gfx950 on
// v_mfma_i32_16x16x64_i8.
//
// The MFMA is signed, so both operands are flipped into the s8 domain
// (a' = a - 128 = a ^ 0x80). With ca = 128 - z_a, cb = 128 - z_b and V the
// set of contraction indices that contribute (all of K for a matmul, the
// in-image taps for a conv):
//
//   sum_V (a - z_a)(b - z_b)
//     = sum_V a'b' + cb * sum_V a' + ca * sum_V b' + |V| * ca * cb
//
// Term 1 is the MFMA accumulation. Padding and K tails are staged as a' = 0,
// so term 2 is the row sum of the staged A tile (one more MFMA against an
// all-ones fragment, which lands in the C/D layout). Term 3 comes from the
// column (per-tap) sums the B packer emits; term 4 is a scalar. Everything
// after the MFMA is wrapping uint32 arithmetic, so the result equals the
// CPU kernels' (int32_t)int64 sum bit for bit for any zero point.
//
// The ranges arrive as device pointers; zero points are derived here with
// the helpers the CPU kernels use (kernels/quantized_util.h).
//
// Structure follows gemm_bf16.hip: 4 waves, 128x128 (or 128x64) C tile,
// K step 64 bytes, double-buffered XOR-swizzled LDS, one ds_read_b128 per
// fragment. Both operands are staged through registers (the flip and the
// masks happen there). Every lane group reads the same 16-byte chunk index
// of A and of B, so the result does not depend on how the instruction
// orders k inside a fragment.
#include "hip_common.h"
#include "kernels/quantized_util.h"
#include "stf_kernels.h"

#include <algorithm>

namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;

constexpr uint32_t kFlip = 0x80808080u;

__device__ __forceinline__ uint4 Flip4(uint4 v, uint32_t flip) {
  v.x ^= flip; v.y ^= flip; v.z ^= flip; v.w ^= flip;
  return v;
}

// A-operand chunk loaders: load(row, k) returns the 16 s8 values
// A'[row][k .. k+16), k a multiple of 16; the caller checks row.
struct LinearA8 {
  const uint8_t* base;
  int64_t ld;
  int64_t kend;   // chunks at k >= kend are zero
  uint32_t flip;  // kFlip for a raw u8 matrix, 0 for a packed s8 one
  __device__ __forceinline__ uint4 load(int64_t row, int64_t k) const {
    if (k >= kend) return uint4{0, 0, 0, 0};
    return Flip4(*(const uint4*)(base + row * ld + k), flip);
  }
};

// Implicit conv: row = output pixel, k = (r, s, c) with c % 16 == 0, so a
// chunk lies inside one tap. Out-of-image taps are 0 after the flip.
struct ConvA8 {
  const uint8_t* x;
  U32Div div_pq, div_q, div_c, div_s;
  int H, W, C;
  int sh, sw, ph, pw;
  int64_t rsc;
  __device__ __forceinline__ uint4 load(int64_t row, int64_t k) const {
    if (k >= rsc) return uint4{0, 0, 0, 0};
    uint32_t row32 = (uint32_t)row, k32 = (uint32_t)k;
    uint32_t n = div_pq.div(row32);
    uint32_t pq = div_pq.mod(row32, n);
    uint32_t p = div_q.div(pq);
    uint32_t q = div_q.mod(pq, p);
    uint32_t rs = div_c.div(k32);
    uint32_t c = div_c.mod(k32, rs);
    uint32_t r = div_s.div(rs);
    uint32_t s_ = div_s.mod(rs, r);
    int h = (int)p * sh - ph + (int)r;
    int w = (int)q * sw - pw + (int)s_;
    if (h < 0 || h >= H || w < 0 || w >= W) return uint4{0, 0, 0, 0};
    return Flip4(
        *(const uint4*)(x + ((((int64_t)n * H + h) * W + w) * C + c)), kFlip);
  }
};

// Which taps of an output pixel lie inside the image (a rectangle), for the
// epilogue's sum over V. A matmul is the 1x1 conv over a 1x1 image with
// cper = K: one tap, always valid.
struct I8Epilogue {
  U32Div div_pq, div_q;
  int H, W, R, S;
  int sh, sw, ph, pw;
  int cper;  // contraction elements per tap
};

// 16-byte slot of (row, chunk) in a [rows][4 chunks] tile; the XOR keeps
// the 16 rows a ds_read_b128 quarter-wave touches on distinct banks.
__device__ __forceinline__ int Slot(int r, int c) {
  return r * 4 + (c ^ ((r >> 2) & 3));
}

template <int WN, class AG>
__launch_bounds__(256) __global__ void GemmI8(
    AG ag, const uint8_t* __restrict__ Bp,  // packed s8 [N][Kp]
    const int32_t* __restrict__ bsums,      // [1 or 1 + taps][N]
    const float* __restrict__ min_a, const float* __restrict__ max_a,
    const float* __restrict__ min_b, const float* __restrict__ max_b,
    int32_t* __restrict__ C, float* __restrict__ min_out,
    float* __restrict__ max_out, int64_t M, int64_t N, int64_t Kp,
    I8Epilogue ep) {
  constexpr int WM = 4;
  constexpr int BM = 2 * WM * 16;  // 128
  constexpr int BN = 2 * WN * 16;  // 128 or 64
  constexpr int PA = BM * 4 / 256; // 16B chunks per thread
  constexpr int PB = BN * 4 / 256;

  __shared__ __attribute__((aligned(16))) uint4 lds[2 * (BM + BN) * 4];
  auto a_tile = [&](int buf) { return lds + buf * BM * 4; };
  auto b_tile = [&](int buf) { return lds + 2 * BM * 4 + buf * BN * 4; };

  // an empty C still gets one block, which writes the ranges
  int nbn = max(1, (int)((N + BN - 1) / BN));
  int nbm = max(1, (int)((M + BM - 1) / BM));
  int bid = XcdSwizzle(blockIdx.x, nbm * nbn);
  int64_t m0 = (int64_t)(bid / nbn) * BM, n0 = (int64_t)(bid % nbn) * BN;

  int tid = threadIdx.x;
  int lane = tid & 63;
  int wid = tid >> 6;
  int wr = wid >> 1, wc = wid & 1;

  if (blockIdx.x == 0 && tid == 0) {
    float sa = stf::QuantStep(min_a[0], max_a[0]);
    float sb = stf::QuantStep(min_b[0], max_b[0]);
    min_out[0] = stf::QuantProductMin(sa, sb);
    max_out[0] = stf::QuantProductMax(sa, sb);
  }

  uint4 ra[PA], rb[PB];
  auto load = [&](int64_t k0) {
#pragma unroll
    for (int p = 0; p < PA; ++p) {
      int s = p * 256 + tid;
      int64_t row = m0 + (s >> 2);
      ra[p] = row < M ? ag.load(row, k0 + (s & 3) * 16) : uint4{0, 0, 0, 0};
    }
#pragma unroll
    for (int p = 0; p < PB; ++p) {
      int s = p * 256 + tid;
      int64_t row = n0 + (s >> 2);
      rb[p] = row < N ? *(const uint4*)(Bp + row * Kp + k0 + (s & 3) * 16)
                      : uint4{0, 0, 0, 0};
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int p = 0; p < PA; ++p) {
      int s = p * 256 + tid;
      a_tile(buf)[Slot(s >> 2, s & 3)] = ra[p];
    }
#pragma unroll
    for (int p = 0; p < PB; ++p) {
      int s = p * 256 + tid;
      b_tile(buf)[Slot(s >> 2, s & 3)] = rb[p];
    }
  };

  i32x4 acc[WM][WN], rs[WM];
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    rs[i] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < WN; ++j) acc[i][j] = {0, 0, 0, 0};
  }
  const i32x4 ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};

  int kt_count = (int)(Kp / 64);
  if (kt_count > 0) {
    load(0);
    store(0);
  }
  __syncthreads();
  int cur = 0;
  for (int kt = 0; kt < kt_count; ++kt) {
    bool more = kt + 1 < kt_count;
    if (more) load((int64_t)(kt + 1) * 64);
    const uint4* at = a_tile(cur);
    const uint4* bt = b_tile(cur);
    i32x4 afrag[WM], bfrag[WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
      afrag[i] = *(const i32x4*)(
          at + Slot(wr * WM * 16 + i * 16 + (lane & 15), lane >> 4));
#pragma unroll
    for (int j = 0; j < WN; ++j)
      bfrag[j] = *(const i32x4*)(
          bt + Slot(wc * WN * 16 + j * 16 + (lane & 15), lane >> 4));
#pragma unroll
    for (int i = 0; i < WM; ++i) {
#pragma unroll
      for (int j = 0; j < WN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(
            afrag[i], bfrag[j], acc[i][j], 0, 0, 0);
      rs[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(afrag[i], ones, rs[i], 0,
                                                     0, 0);
    }
    // The other buffer was last read before the previous barrier.
    if (more) store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue: C/D map col = lane & 15, row = (lane >> 4) * 4 + reg ----
  uint32_t ca = 128u - (uint32_t)stf::QuantZeroPoint(min_a[0], max_a[0]);
  uint32_t cb = 128u - (uint32_t)stf::QuantZeroPoint(min_b[0], max_b[0]);
  uint32_t cab = ca * cb;
  int taps = ep.R * ep.S;
#pragma unroll
  for (int i = 0; i < WM; ++i) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      int64_t row = m0 + wr * WM * 16 + i * 16 + (lane >> 4) * 4 + reg;
      if (row >= M) continue;
      uint32_t row32 = (uint32_t)row;
      uint32_t n = ep.div_pq.div(row32);
      uint32_t pq = ep.div_pq.mod(row32, n);
      int p = (int)ep.div_q.div(pq);
      int q = (int)ep.div_q.mod(pq, (uint32_t)p);
      int r_lo = max(0, ep.ph - p * ep.sh);
      int r_hi = min(ep.R, ep.H + ep.ph - p * ep.sh);
      int s_lo = max(0, ep.pw - q * ep.sw);
      int s_hi = min(ep.S, ep.W + ep.pw - q * ep.sw);
      int nvalid = max(0, r_hi - r_lo) * max(0, s_hi - s_lo);
      uint32_t base = cb * (uint32_t)rs[i][reg] +
                      (uint32_t)nvalid * (uint32_t)ep.cper * cab;
#pragma unroll
      for (int j = 0; j < WN; ++j) {
        int64_t col = n0 + wc * WN * 16 + j * 16 + (lane & 15);
        if (col >= N) continue;
        uint32_t sb;
        if (nvalid == taps) {
          sb = (uint32_t)bsums[col];  // row 0: the sum over every tap
        } else {
          sb = 0;
          for (int r = r_lo; r < r_hi; ++r)
            for (int s = s_lo; s < s_hi; ++s)
              sb += (uint32_t)bsums[(int64_t)(1 + r * ep.S + s) * N + col];
        }
        C[row * N + col] =
            (int32_t)((uint32_t)acc[i][j][reg] + base + ca * sb);
      }
    }
  }
}

// src u8, element (row, k) at src[row * sr + k * sk] -> dst s8 [rows][Kp],
// flipped, K tail zero. One thread per 64-byte block of a dst row. sums
// (optional, zeroed): [0][row] += sum_k dst; with taps > 1 also
// [1 + k / cper][row] += the part of it in that tap.
__global__ void PackI8(const uint8_t* __restrict__ src, int64_t sr,
                       int64_t sk, int64_t rows, int64_t K, int64_t Kp,
                       uint8_t* __restrict__ dst, int32_t* __restrict__ sums,
                       int taps, int64_t cper) {
  int64_t nblk = Kp / 64;
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * nblk) return;
  // k-major sources (sr == 1) are read coalesced across rows
  int64_t row = sr == 1 ? idx % rows : idx / nblk;
  int64_t blk = sr == 1 ? idx / rows : idx % nblk;
  int64_t k0 = blk * 64;
  if (k0 >= K) {  // only when K == 0
    for (int v = 0; v < 4; ++v)
      *(uint4*)(dst + row * Kp + k0 + v * 16) = uint4{0, 0, 0, 0};
    return;
  }
  int64_t tap = taps > 1 ? k0 / cper : 0;
  int64_t c = taps > 1 ? k0 - tap * cper : 0;
  int32_t total = 0, run = 0;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      int64_t k = k0 + v * 16 + e;
      if (k < K) {
        uint8_t b = src[row * sr + k * sk] ^ 0x80;
        w[e >> 2] |= (uint32_t)b << ((e & 3) * 8);
        total += (int8_t)b;
        if (taps > 1) {
          run += (int8_t)b;
          if (++c == cper) {
            if (sums) atomicAdd(&sums[(1 + tap) * rows + row], run);
            run = 0;
            c = 0;
            ++tap;
          }
        }
      }
    }
    *(uint4*)(dst + row * Kp + k0 + v * 16) = uint4{w[0], w[1], w[2], w[3]};
  }
  if (!sums) return;
  if (taps > 1 && c != 0) atomicAdd(&sums[(1 + tap) * rows + row], run);
  atomicAdd(&sums[row], total);
}

// u8 NHWC image -> s8 column matrix [n*p*q][kp], flipped; out-of-image taps
// and the K tail are 0. One thread per 16-byte chunk.
__global__ void Im2ColI8(const uint8_t* __restrict__ x,
                         uint8_t* __restrict__ col, StfConvGeom g,
                         int64_t kp) {
  int64_t nch = kp / 16;
  int64_t M = (int64_t)g.n * g.p * g.q;
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= M * nch) return;
  int64_t row = idx / nch;
  int64_t k0 = (idx % nch) * 16;
  int q = (int)(row % g.q);
  int p = (int)((row / g.q) % g.p);
  int64_t n = row / ((int64_t)g.p * g.q);
  int64_t rsc = (int64_t)g.r * g.s * g.c;
  uint32_t w[4] = {0, 0, 0, 0};
  for (int e = 0; e < 16; ++e) {
    int64_t k = k0 + e;
    if (k >= rsc) break;
    int c = (int)(k % g.c);
    int rs = (int)(k / g.c);
    int s = rs % g.s, r = rs / g.s;
    int h = p * g.sh - g.ph + r;
    int wi = q * g.sw - g.pw + s;
    if (h < 0 || h >= g.h || wi < 0 || wi >= g.w) continue;
    uint8_t b = x[((n * g.h + h) * g.w + wi) * g.c + c] ^ 0x80;
    w[e >> 2] |= (uint32_t)b << ((e & 3) * 8);
  }
  *(uint4*)(col + row * kp + k0) = uint4{w[0], w[1], w[2], w[3]};
}

template <class AG>
hipError_t LaunchI8(const AG& ag, const void* Bp, const int32_t* bsums,
                    const float* min_a, const float* max_a,
                    const float* min_b, const float* max_b, int32_t* C,
                    float* min_out, float* max_out, int64_t M, int64_t N,
                    int64_t Kp, const I8Epilogue& ep, hipStream_t stream) {
  int64_t nbm = std::max<int64_t>(1, (M + 127) / 128);
  if (N <= 64) {
    hipLaunchKernelGGL((GemmI8<2, AG>), dim3((uint32_t)nbm), dim3(256), 0,
                       stream, ag, (const uint8_t*)Bp, bsums, min_a, max_a,
                       min_b, max_b, C, min_out, max_out, M, N, Kp, ep);
  } else {
    int64_t nbn = std::max<int64_t>(1, (N + 127) / 128);
    hipLaunchKernelGGL((GemmI8<4, AG>), dim3((uint32_t)(nbm * nbn)),
                       dim3(256), 0, stream, ag, (const uint8_t*)Bp, bsums,
                       min_a, max_a, min_b, max_b, C, min_out, max_out, M, N,
                       Kp, ep);
  }
  return hipGetLastError();
}

I8Epilogue ConvEpilogue(const StfConvGeom& g) {
  I8Epilogue ep;
  ep.div_pq.init((uint32_t)(g.p * g.q));
  ep.div_q.init((uint32_t)g.q);
  ep.H = g.h; ep.W = g.w; ep.R = g.r; ep.S = g.s;
  ep.sh = g.sh; ep.sw = g.sw; ep.ph = g.ph; ep.pw = g.pw;
  ep.cper = g.c;
  return ep;
}

}  // namespace

extern "C" hipError_t stf_pack_i8(const void* src_u8, int64_t row_stride,
                                  int64_t k_stride, int64_t rows, int64_t K,
                                  void* dst_s8, int32_t* sums, int taps,
                                  hipStream_t stream) {
  int64_t Kp = (K + 63) & ~int64_t(63);
  int64_t threads = rows * (Kp / 64);
  if (threads <= 0) return hipSuccess;
  if (taps < 1 || K % taps != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(PackI8, dim3((uint32_t)((threads + 255) / 256)),
                     dim3(256), 0, stream, (const uint8_t*)src_u8, row_stride,
                     k_stride, rows, K, Kp, (uint8_t*)dst_s8, sums, taps,
                     K / taps);
  return hipGetLastError();
}

extern "C" hipError_t stf_im2col_i8(const void* x_u8, void* col_s8,
                                    const StfConvGeom* g, int64_t kp,
                                    hipStream_t stream) {
  int64_t threads = (int64_t)g->n * g->p * g->q * (kp / 16);
  if (threads <= 0) return hipSuccess;
  hipLaunchKernelGGL(Im2ColI8, dim3((uint32_t)((threads + 255) / 256)),
                     dim3(256), 0, stream, (const uint8_t*)x_u8,
                     (uint8_t*)col_s8, *g, kp);
  return hipGetLastError();
}

extern "C" hipError_t stf_gemm_i8(const void* A, int a_packed,
                                  const void* Bp, const int32_t* bsums,
                                  const float* min_a, const float* max_a,
                                  const float* min_b, const float* max_b,
                                  int32_t* C, float* min_out, float* max_out,
                                  int64_t M, int64_t N, int64_t K,
                                  hipStream_t stream) {
  int64_t Kp = (K + 63) & ~int64_t(63);
  if (!a_packed && (K & 15) != 0) return hipErrorInvalidValue;
  LinearA8 ag{(const uint8_t*)A, a_packed ? Kp : K, a_packed ? Kp : K,
              a_packed ? 0u : kFlip};
  // the 1x1 conv over a 1x1 image: one tap of K elements, always valid
  StfConvGeom g1{(int)M, 1, 1, (int)K, 1, 1, 1, 1, 0, 0, 1, 1, N};
  return LaunchI8(ag, Bp, bsums, min_a, max_a, min_b, max_b, C, min_out,
                  max_out, M, N, Kp, ConvEpilogue(g1), stream);
}

extern "C" hipError_t stf_conv2d_i8(const void* x_or_col, int implicit,
                                    const void* wp, const int32_t* wsums,
                                    const float* min_x, const float* max_x,
                                    const float* min_w, const float* max_w,
                                    int32_t* y, float* min_out,
                                    float* max_out, const StfConvGeom* g,
                                    hipStream_t stream) {
  int64_t M = (int64_t)g->n * g->p * g->q;
  int64_t rsc = (int64_t)g->r * g->s * g->c;
  int64_t Kp = (rsc + 63) & ~int64_t(63);
  I8Epilogue ep = ConvEpilogue(*g);
  if (!implicit) {
    LinearA8 ag{(const uint8_t*)x_or_col, Kp, Kp, 0u};
    return LaunchI8(ag, wp, wsums, min_x, max_x, min_w, max_w, y, min_out,
                    max_out, M, g->cout, Kp, ep, stream);
  }
  if ((g->c & 15) != 0) return hipErrorInvalidValue;
  ConvA8 ag;
  ag.x = (const uint8_t*)x_or_col;
  ag.div_pq.init((uint32_t)(g->p * g->q));
  ag.div_q.init((uint32_t)g->q);
  ag.div_c.init((uint32_t)g->c);
  ag.div_s.init((uint32_t)g->s);
  ag.H = g->h; ag.W = g->w; ag.C = g->c;
  ag.sh = g->sh; ag.sw = g->sw; ag.ph = g->ph; ag.pw = g->pw;
  ag.rsc = rsc;
  return LaunchI8(ag, wp, wsums, min_x, max_x, min_w, max_w, y, min_out,
                  max_out, M, g->cout, Kp, ep, stream);
}
