// What gemm_i8.hip (qint32 out) and gemm_i8_fused.hip (fused epilogue, quint8
// out) share: the A-operand loaders, the staging and MFMA loop over K as one
// device function template, the tap geometry of the epilogues, and the host
// code that picks a loader. gemm_i8.hip's header comment has the arithmetic.
// Only those two files include this.
#pragma once

#include "hip_common.h"
#include "kernels/quantized_util.h"
#include "stf_kernels.h"

#include <algorithm>

namespace i8 {

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

constexpr int kWM = 4;           // 16-row MFMA tiles per wave along M
constexpr int kBM = 2 * kWM * 16;  // 128
// LDS of a block, in 16-byte units: two buffers of an A and a B tile.
constexpr int LdsChunks(int WN) { return 2 * (kBM + 2 * WN * 16) * 4; }

// The block's tile origin (m0, n0). An empty C still gets one block, which
// writes the ranges.
template <int WN>
__device__ __forceinline__ void BlockOrigin(int64_t M, int64_t N, int64_t* m0,
                                            int64_t* n0) {
  constexpr int BN = 2 * WN * 16;
  int nbn = max(1, (int)((N + BN - 1) / BN));
  int nbm = max(1, (int)((M + kBM - 1) / kBM));
  int bid = XcdSwizzle(blockIdx.x, nbm * nbn);
  *m0 = (int64_t)(bid / nbn) * kBM;
  *n0 = (int64_t)(bid % nbn) * BN;
}

// The K loop of both kernels: stages the block's A and B tiles through lds
// and leaves the products in acc and the A row sums in rs. SWAP issues each
// MFMA with its operands exchanged, which transposes what a lane holds:
//   !SWAP  acc[i][j][reg]: row = (lane >> 4) * 4 + reg, col = lane & 15;
//          rs[i][reg]: the sum of that row
//    SWAP  acc[i][j][reg]: row = lane & 15, col = (lane >> 4) * 4 + reg;
//          rs[i][0]: the sum of row lane & 15
// (row, col inside the 16x16 tile i, j of the wave). The sums are integer
// and exact, so both forms hold the same numbers. Ends behind a barrier:
// lds is free.
template <int WN, bool SWAP, class AG>
__device__ __forceinline__ void I8MainLoop(
    const AG& ag, const uint8_t* __restrict__ Bp, int64_t M, int64_t N,
    int64_t Kp, int64_t m0, int64_t n0, uint4* lds, i32x4 (&acc)[kWM][WN],
    i32x4 (&rs)[kWM]) {
  constexpr int WM = kWM;
  constexpr int BM = kBM;
  constexpr int BN = 2 * WN * 16;  // 128 or 64
  constexpr int PA = BM * 4 / 256; // 16B chunks per thread
  constexpr int PB = BN * 4 / 256;

  auto a_tile = [&](int buf) { return lds + buf * BM * 4; };
  auto b_tile = [&](int buf) { return lds + 2 * BM * 4 + buf * BN * 4; };

  int tid = threadIdx.x;
  int lane = tid & 63;
  int wid = tid >> 6;
  int wr = wid >> 1, wc = wid & 1;

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
        acc[i][j] = SWAP ? __builtin_amdgcn_mfma_i32_16x16x64_i8(
                               bfrag[j], afrag[i], acc[i][j], 0, 0, 0)
                         : __builtin_amdgcn_mfma_i32_16x16x64_i8(
                               afrag[i], bfrag[j], acc[i][j], 0, 0, 0);
      rs[i] = SWAP ? __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, afrag[i],
                                                           rs[i], 0, 0, 0)
                   : __builtin_amdgcn_mfma_i32_16x16x64_i8(afrag[i], ones,
                                                           rs[i], 0, 0, 0);
    }
    // The other buffer was last read before the previous barrier.
    if (more) store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
}

// The in-image taps of output pixel `row` (a rectangle of the filter).
struct I8Taps {
  int r_lo, r_hi, s_lo, s_hi, nvalid;
};
__device__ __forceinline__ I8Taps TapsOf(const I8Epilogue& ep, int64_t row) {
  uint32_t row32 = (uint32_t)row;
  uint32_t n = ep.div_pq.div(row32);
  uint32_t pq = ep.div_pq.mod(row32, n);
  int p = (int)ep.div_q.div(pq);
  int q = (int)ep.div_q.mod(pq, (uint32_t)p);
  I8Taps t;
  t.r_lo = max(0, ep.ph - p * ep.sh);
  t.r_hi = min(ep.R, ep.H + ep.ph - p * ep.sh);
  t.s_lo = max(0, ep.pw - q * ep.sw);
  t.s_hi = min(ep.S, ep.W + ep.pw - q * ep.sw);
  t.nvalid = max(0, t.r_hi - t.r_lo) * max(0, t.s_hi - t.s_lo);
  return t;
}

// Sum over the taps t of column col's packed filter values: bsums is
// [1 + taps][N], row 0 the sum over every tap, row 1 + r * S + s that of one
// tap. Only a border pixel walks the rows.
__device__ __forceinline__ uint32_t TapSum(const int32_t* __restrict__ bsums,
                                           const I8Epilogue& ep,
                                           const I8Taps& t, int64_t N,
                                           int64_t col) {
  if (t.nvalid == ep.R * ep.S) return (uint32_t)bsums[col];
  uint32_t sb = 0;
  for (int r = t.r_lo; r < t.r_hi; ++r)
    for (int s = t.s_lo; s < t.s_hi; ++s)
      sb += (uint32_t)bsums[(int64_t)(1 + r * ep.S + s) * N + col];
  return sb;
}

inline I8Epilogue ConvEpilogue(const StfConvGeom& g) {
  I8Epilogue ep;
  ep.div_pq.init((uint32_t)(g.p * g.q));
  ep.div_q.init((uint32_t)g.q);
  ep.H = g.h; ep.W = g.w; ep.R = g.r; ep.S = g.s;
  ep.sh = g.sh; ep.sw = g.sw; ep.ph = g.ph; ep.pw = g.pw;
  ep.cper = g.c;
  return ep;
}

// The A loader and epilogue geometry of a matmul, handed to
// launch(ag, M, N, Kp, ep): GemmI8's launcher or the fused kernel's.
template <class Launch>
hipError_t GemmWith(const void* A, int a_packed, int64_t M, int64_t N,
                    int64_t K, Launch launch) {
  int64_t Kp = (K + 63) & ~int64_t(63);
  if (!a_packed && (K & 15) != 0) return hipErrorInvalidValue;
  LinearA8 ag{(const uint8_t*)A, a_packed ? Kp : K, a_packed ? Kp : K,
              a_packed ? 0u : kFlip};
  // the 1x1 conv over a 1x1 image: one tap of K elements, always valid
  StfConvGeom g1{(int)M, 1, 1, (int)K, 1, 1, 1, 1, 0, 0, 1, 1, N};
  return launch(ag, M, N, Kp, ConvEpilogue(g1));
}

// The same for a conv: the implicit loader, or the column matrix's.
template <class Launch>
hipError_t ConvWith(const void* x_or_col, int implicit, const StfConvGeom* g,
                    Launch launch) {
  int64_t M = (int64_t)g->n * g->p * g->q;
  int64_t rsc = (int64_t)g->r * g->s * g->c;
  int64_t Kp = (rsc + 63) & ~int64_t(63);
  I8Epilogue ep = ConvEpilogue(*g);
  if (!implicit) {
    LinearA8 ag{(const uint8_t*)x_or_col, Kp, Kp, 0u};
    return launch(ag, M, g->cout, Kp, ep);
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
  return launch(ag, M, g->cout, Kp, ep);
}

}  // namespace i8
