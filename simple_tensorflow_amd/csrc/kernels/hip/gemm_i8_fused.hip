// Quantized quint8 x quint8 -> quint8 GEMM and Conv2D with the bias, the
// activation and the requantization (and, for the conv, a residual sum)
// fused in, for gfx950 on
// v_mfma_i32_16x16x64_i8. gemm_i8.hip's header comment has the integer
// arithmetic; the accumulator this kernel requantizes is the value that
// GemmI8 stores.
//
// GemmI8Fused is GemmI8's K loop (I8MainLoop in gemm_i8_core.h, one device
// function template) in front of a fused bias + activation + requantize
// epilogue that writes quint8 (stf::QuantFusedU8 in
// kernels/quantized_util.h, which the CPU kernels call too):
//
//  * Swapped MFMA operands: the MFMA is issued as (weights, pixels), so in
//    the C/D map a lane holds four consecutive output channels
//    (quad * 4 + reg, quad = lane >> 4) of one pixel (lane & 15). Its four
//    quint8 pack into one dword with no cross-lane traffic. The A row sum is
//    mfma(ones, pixels): the same value in every register, register 0 is
//    used.
//  * bias[col] and ca * bsums[col] of the lane's 4 * WN channels are loaded
//    once, ahead of the element loop; the per-pixel part (row sum, tap count,
//    and the per-tap sums for border pixels only) is computed once per pixel
//    as in GemmI8. The activation is a template parameter.
//  * Output through LDS: behind the K loop's last barrier the A/B tiles are
//    dead, and the packed dwords go into a [128 pixels][BN channels] u8 tile
//    there (16 KB of the 32 KB for BN = 128, 8 KB of the 24 KB for BN = 64).
//    The tile is addressed in 16-byte chunks, NCH = BN / 16 per row, chunk c
//    of row r at slot r * NCH + (c ^ ((r / (16 / NCH)) & (NCH - 1))).
//    16 / NCH rows cover the 64 banks once and the XOR shifts each further
//    group of rows by one chunk, so the dword writes of a wave (16 pixels x 4
//    quads, one chunk column) fall on 64 distinct banks, and so do the
//    16-byte reads of a quarter-wave (consecutive chunks of 16 / NCH rows).
//    Consecutive threads then store consecutive 16-byte chunks of a pixel's
//    channels. When N % 16 != 0 the same chunks go out as byte stores, cut
//    at N; rows >= M are not stored.
//
// GemmI8FusedSum is the same block function with a residual sum in front of
// the activation (QuantizedConv2DWithBiasSumAndRequantize,
// stf::QuantFusedSumU8): a quint8 summand of C's shape.
//  * Its [128 pixels][BN channels] tile has an LDS region of its own behind
//    the A/B tiles (BM * NCH chunks: 32 KB in all for BN = 64, 48 KB for
//    BN = 128; at the kernel's register-limited 3 and 2 blocks per CU that
//    stays inside the CU's LDS), in the output tile's layout.
//  * It is filled in front of the K loop (FillSummandTile), so the loads
//    overlap the loop and nothing of the summand is live in registers across
//    it. One s_waitcnt vmcnt(0) and a barrier stand in front of the
//    epilogue's first read.
//  * The epilogue works in place: a lane reads the dword of its four
//    channels' summands at the address where GemmI8Fused writes its packed
//    result, and writes the result there. Same lane, same dword: no hazard,
//    and the bank-conflict argument above carries over unchanged. The
//    tile -> C pass then stores from this region.
// profiles/quantized_fused_sum.md has the timings and the resource table.
//
// This file is built without the packed f32 VALU operations
// (v_pk_add/mul/fma_f32; the Makefile turns the target feature off for it, as
// for conv_dw_tall.hip): the epilogue is the only f32 arithmetic here, and
// its two roundings per element are kept as separate scalar instructions.
// That also costs fewer registers: GemmI8Fused<2> needs 83-84 VGPRs with the
// feature off and 100-101 with it on, GemmI8Fused<4> 130-131 against
// 146-147 (plus 48 and 80 AGPRs). gemm_i8.hip is built as before.
#include "gemm_i8_core.h"

namespace {

using namespace i8;

// 16-byte slot of (pixel row r, 16-channel chunk c) in the fused kernel's
// [128 rows][NCH chunks] u8 output tile. A row is NCH * 16 bytes, so
// 16 / NCH rows span the 64 banks once; the XOR moves the chunk by one
// 16-byte column per such group of rows.
template <int NCH>
__device__ __forceinline__ int OutSlot(int r, int c) {
  return r * NCH + (c ^ ((r / (16 / NCH)) & (NCH - 1)));
}

// What the summand variant takes beyond the fused kernel's arguments.
struct I8Summand {
  const uint8_t* q;  // [M][N] quint8, 16-byte aligned
  const float* mn;   // its range
  const float* mx;
};

// The block's [BM][BN] tile of the summand into `region`, in the output
// tile's layout: chunk (r, c) at slot OutSlot<NCH>(r, c). Issued in front of
// the K loop. With N % 16 == 0 each thread issues BM * NCH / 256 16-byte
// global_load_lds and keeps nothing in registers. The instruction writes the
// lanes of a wave to consecutive slots behind a wave-uniform base, so the
// swizzle is applied on the global side: the thread of linear slot s fetches
// the chunk (r, c) with OutSlot<NCH>(r, c) == s (the XOR is its own inverse).
// Lanes whose chunk lies at row >= M or col >= N are masked off; their slots
// are never read for a stored element. Otherwise the 16-byte chunks are
// misaligned: plain byte loads, cut at N, and a ds_write. Nobody waits here:
// the K loop's own waits hold with these older loads outstanding (loads
// retire in order), and the epilogue waits for all of them.
template <int WN>
__device__ __forceinline__ void FillSummandTile(
    const uint8_t* __restrict__ S, int64_t M, int64_t N, int64_t m0,
    int64_t n0, uint4* region) {
  constexpr int NCH = 2 * WN;
  int tid = threadIdx.x;
  bool vec = (N & 15) == 0;
#pragma unroll
  for (int pass = 0; pass < kBM * NCH / 256; ++pass) {
    int s = pass * 256 + tid;
    int r = s / NCH;
    int c = (s % NCH) ^ ((r / (16 / NCH)) & (NCH - 1));
    int64_t row = m0 + r, col = n0 + c * 16;
    if (row >= M || col >= N) continue;
    const uint8_t* g = S + row * N + col;
    if (vec) {
      // the wave's base: lane i lands at slot base + i, which is s
      uint4* base = region + pass * 256 + (tid & ~63);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) uint32_t*)g,
          (__attribute__((address_space(3))) uint32_t*)base, 16, 0, 0);
    } else {
      int nb = (int)min((int64_t)16, N - col);
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int b = 0; b < 16; ++b)
        if (b < nb) w[b >> 2] |= (uint32_t)g[b] << (8 * (b & 3));
      region[s] = uint4{w[0], w[1], w[2], w[3]};
    }
  }
}

// One block of the fused form: quint8 out = requantize(activation(acc * m +
// bias[col] [+ the dequantized summand])), stf::QuantFusedU8 or, with SUM,
// stf::QuantFusedSumU8, on the accumulators of the swapped main loop. See the
// header comment for the epilogue's layout. lds holds LdsChunks(WN) chunks
// and, with SUM, the summand's BM * NCH behind them.
template <int WN, int ACT, bool SUM, class AG>
__device__ __forceinline__ void I8FusedBlock(
    AG ag, const uint8_t* __restrict__ Bp,
    const int32_t* __restrict__ bsums, const float* __restrict__ bias,
    const I8Summand& sm, const float* __restrict__ min_a,
    const float* __restrict__ max_a, const float* __restrict__ min_b,
    const float* __restrict__ max_b, const float* __restrict__ req_min,
    const float* __restrict__ req_max, uint8_t* __restrict__ C,
    float* __restrict__ min_out, float* __restrict__ max_out, int64_t M,
    int64_t N, int64_t Kp, I8Epilogue ep, uint4* lds) {
  constexpr int WM = kWM;
  constexpr int BM = kBM;
  constexpr int BN = 2 * WN * 16;
  constexpr int NCH = BN / 16;  // 16-byte chunks per tile row
  static_assert(BM * NCH <= LdsChunks(WN), "the output tile reuses the LDS");
  // the output tile: the dead A/B tiles, or in place over the summand's
  uint4* out = SUM ? lds + LdsChunks(WN) : lds;
  int64_t m0, n0;
  BlockOrigin<WN>(M, N, &m0, &n0);

  int tid = threadIdx.x;
  int lane = tid & 63;
  int wid = tid >> 6;
  int wr = wid >> 1, wc = wid & 1;
  int quad = lane >> 4;  // which 4 channels of a 16-channel chunk

  if constexpr (SUM) FillSummandTile<WN>(sm.q, M, N, m0, n0, out);

  i32x4 acc[WM][WN], rs[WM];
  I8MainLoop<WN, true>(ag, Bp, M, N, Kp, m0, n0, lds, acc, rs);

  // behind the K loop, so that nothing of it is live across the loop
  const stf::QuantFusedScale sc = stf::MakeQuantFusedScale(
      min_a[0], max_a[0], min_b[0], max_b[0], req_min[0], req_max[0]);
  if (blockIdx.x == 0 && tid == 0) {
    min_out[0] = sc.mn;
    max_out[0] = sc.mx;
  }
  float s_min = 0.f, s_step = 0.f;
  if constexpr (SUM) {
    s_min = sm.mn[0];
    s_step = stf::QuantStep(s_min, sm.mx[0]);
    // every load of the summand tile has landed, in every wave
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- epilogue: C/D map row (pixel) = lane & 15, col (channel) =
  // quad * 4 + reg ----
  uint32_t ca = 128u - (uint32_t)stf::QuantZeroPoint(min_a[0], max_a[0]);
  uint32_t cb = 128u - (uint32_t)stf::QuantZeroPoint(min_b[0], max_b[0]);
  uint32_t cab = ca * cb;
  int taps = ep.R * ep.S;

  // per-channel values of the lane's 4 * WN channels, loaded once
  float bv[WN][4];
  uint32_t cs[WN][4];  // ca * (the filter column's sum over every tap)
#pragma unroll
  for (int j = 0; j < WN; ++j) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      int64_t col = n0 + wc * WN * 16 + j * 16 + quad * 4 + reg;
      bool in = col < N;
      bv[j][reg] = in ? bias[col] : 0.f;
      cs[j][reg] = in ? ca * (uint32_t)bsums[col] : 0u;
    }
  }

  uint32_t* tile = (uint32_t*)out;
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    int rt = wr * WM * 16 + i * 16 + (lane & 15);
    int64_t row = m0 + rt;
    if (row >= M) continue;  // its tile row is never read
    I8Taps t = TapsOf(ep, row);
    uint32_t base = cb * (uint32_t)rs[i][0] +
                    (uint32_t)t.nvalid * (uint32_t)ep.cper * cab;
    bool border = t.nvalid != taps;
#pragma unroll
    for (int j = 0; j < WN; ++j) {
      // the lane's dword: with SUM it holds the four summands, and the
      // result replaces them (same lane, same address: no hazard)
      int dw = OutSlot<NCH>(rt, wc * WN + j) * 4 + quad;
      uint32_t sq = 0;
      if constexpr (SUM) sq = tile[dw];
      uint32_t packed = 0;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        uint32_t s = cs[j][reg];
        if (border) {  // the sums of the in-image taps only
          int64_t col = n0 + wc * WN * 16 + j * 16 + quad * 4 + reg;
          s = col < N ? ca * TapSum(bsums, ep, t, N, col) : 0u;
        }
        int32_t a = (int32_t)((uint32_t)acc[i][j][reg] + base + s);
        if constexpr (SUM)
          packed |= (uint32_t)stf::QuantFusedSumU8<ACT>(
                        a, bv[j][reg], (sq >> (8 * reg)) & 255u, s_min,
                        s_step, sc)
                    << (8 * reg);
        else
          packed |= (uint32_t)stf::QuantFusedU8<ACT>(a, bv[j][reg], sc)
                    << (8 * reg);
      }
      tile[dw] = packed;
    }
  }
  __syncthreads();

  // ---- tile -> C: consecutive threads take consecutive 16-byte chunks of
  // a pixel's channels ----
  bool vec = (N & 15) == 0;
#pragma unroll
  for (int pass = 0; pass < BM * NCH / 256; ++pass) {
    int s = pass * 256 + tid;
    int rt = s / NCH, ch = s % NCH;
    int64_t row = m0 + rt, col = n0 + ch * 16;
    if (row >= M || col >= N) continue;
    uint4 v = out[OutSlot<NCH>(rt, ch)];
    uint8_t* dst = C + row * N + col;
    if (vec) {
      *(uint4*)dst = v;
    } else {
      int nb = (int)min((int64_t)16, N - col);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int b = 0; b < 16; ++b)
        if (b < nb) dst[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
    }
  }
}

template <int WN, int ACT, class AG>
__launch_bounds__(256) __global__ void GemmI8Fused(
    AG ag, const uint8_t* __restrict__ Bp,  // packed s8 [N][Kp]
    const int32_t* __restrict__ bsums,      // [1 or 1 + taps][N]
    const float* __restrict__ bias,         // [N]
    const float* __restrict__ min_a, const float* __restrict__ max_a,
    const float* __restrict__ min_b, const float* __restrict__ max_b,
    const float* __restrict__ req_min, const float* __restrict__ req_max,
    uint8_t* __restrict__ C, float* __restrict__ min_out,
    float* __restrict__ max_out, int64_t M, int64_t N, int64_t Kp,
    I8Epilogue ep) {
  __shared__ __attribute__((aligned(16))) uint4 lds[LdsChunks(WN)];
  I8FusedBlock<WN, ACT, false>(ag, Bp, bsums, bias, I8Summand{}, min_a, max_a,
                               min_b, max_b, req_min, req_max, C, min_out,
                               max_out, M, N, Kp, ep, lds);
}

// GemmI8Fused with the residual sum: the summand tile has an LDS region of
// its own behind the K loop's, BM * NCH chunks (32 KB in all for WN = 2,
// 48 KB for WN = 4).
template <int WN, int ACT, class AG>
__launch_bounds__(256) __global__ void GemmI8FusedSum(
    AG ag, const uint8_t* __restrict__ Bp, const int32_t* __restrict__ bsums,
    const float* __restrict__ bias, I8Summand sm,
    const float* __restrict__ min_a, const float* __restrict__ max_a,
    const float* __restrict__ min_b, const float* __restrict__ max_b,
    const float* __restrict__ req_min, const float* __restrict__ req_max,
    uint8_t* __restrict__ C, float* __restrict__ min_out,
    float* __restrict__ max_out, int64_t M, int64_t N, int64_t Kp,
    I8Epilogue ep) {
  __shared__ __attribute__((aligned(16)))
  uint4 lds[LdsChunks(WN) + kBM * 2 * WN];
  I8FusedBlock<WN, ACT, true>(ag, Bp, bsums, bias, sm, min_a, max_a, min_b,
                              max_b, req_min, req_max, C, min_out, max_out, M,
                              N, Kp, ep, lds);
}

// What the fused kernels take beyond GemmI8's arguments; sum.q is null
// without a summand.
struct I8FusedArgs {
  const float* bias;
  const float* req_min;
  const float* req_max;
  int activation;  // stf::QuantActivation
  I8Summand sum;
};

template <int WN, int ACT, bool SUM, class AG>
void LaunchI8FusedTile(uint32_t blocks, const AG& ag, const void* Bp,
                       const int32_t* bsums, const I8FusedArgs& f,
                       const float* min_a, const float* max_a,
                       const float* min_b, const float* max_b, uint8_t* C,
                       float* min_out, float* max_out, int64_t M, int64_t N,
                       int64_t Kp, const I8Epilogue& ep, hipStream_t stream) {
  if constexpr (SUM)
    hipLaunchKernelGGL((GemmI8FusedSum<WN, ACT, AG>), dim3(blocks), dim3(256),
                       0, stream, ag, (const uint8_t*)Bp, bsums, f.bias, f.sum,
                       min_a, max_a, min_b, max_b, f.req_min, f.req_max, C,
                       min_out, max_out, M, N, Kp, ep);
  else
    hipLaunchKernelGGL((GemmI8Fused<WN, ACT, AG>), dim3(blocks), dim3(256), 0,
                       stream, ag, (const uint8_t*)Bp, bsums, f.bias, min_a,
                       max_a, min_b, max_b, f.req_min, f.req_max, C, min_out,
                       max_out, M, N, Kp, ep);
}

template <int ACT, bool SUM, class AG>
hipError_t LaunchI8FusedAct(const AG& ag, const void* Bp,
                            const int32_t* bsums, const I8FusedArgs& f,
                            const float* min_a, const float* max_a,
                            const float* min_b, const float* max_b,
                            uint8_t* C, float* min_out, float* max_out,
                            int64_t M, int64_t N, int64_t Kp,
                            const I8Epilogue& ep, hipStream_t stream) {
  int64_t nbm = std::max<int64_t>(1, (M + 127) / 128);
  if (N <= 64) {
    LaunchI8FusedTile<2, ACT, SUM>((uint32_t)nbm, ag, Bp, bsums, f, min_a,
                                   max_a, min_b, max_b, C, min_out, max_out,
                                   M, N, Kp, ep, stream);
  } else {
    int64_t nbn = std::max<int64_t>(1, (N + 127) / 128);
    LaunchI8FusedTile<4, ACT, SUM>((uint32_t)(nbm * nbn), ag, Bp, bsums, f,
                                   min_a, max_a, min_b, max_b, C, min_out,
                                   max_out, M, N, Kp, ep, stream);
  }
  return hipGetLastError();
}

// The fused kernel of f.activation, with or without the summand.
template <bool SUM, class AG>
hipError_t LaunchI8Fused(const AG& ag, const void* Bp, const int32_t* bsums,
                         const I8FusedArgs& f, const float* min_a,
                         const float* max_a, const float* min_b,
                         const float* max_b, uint8_t* C, float* min_out,
                         float* max_out, int64_t M, int64_t N, int64_t Kp,
                         const I8Epilogue& ep, hipStream_t stream) {
  switch (f.activation) {
    case stf::kQuantActNone:
      return LaunchI8FusedAct<stf::kQuantActNone, SUM>(
          ag, Bp, bsums, f, min_a, max_a, min_b, max_b, C, min_out, max_out,
          M, N, Kp, ep, stream);
    case stf::kQuantActRelu:
      return LaunchI8FusedAct<stf::kQuantActRelu, SUM>(
          ag, Bp, bsums, f, min_a, max_a, min_b, max_b, C, min_out, max_out,
          M, N, Kp, ep, stream);
    case stf::kQuantActRelu6:
      return LaunchI8FusedAct<stf::kQuantActRelu6, SUM>(
          ag, Bp, bsums, f, min_a, max_a, min_b, max_b, C, min_out, max_out,
          M, N, Kp, ep, stream);
  }
  return hipErrorInvalidValue;
}

}  // namespace

extern "C" hipError_t stf_gemm_i8_fused(
    const void* A, int a_packed, const void* Bp, const int32_t* bsums,
    const float* bias, const float* min_a, const float* max_a,
    const float* min_b, const float* max_b, const float* req_min,
    const float* req_max, int activation, uint8_t* C, float* min_out,
    float* max_out, int64_t M, int64_t N, int64_t K, hipStream_t stream) {
  I8FusedArgs f{bias, req_min, req_max, activation, {}};
  return GemmWith(A, a_packed, M, N, K,
                  [&](const auto& ag, int64_t m, int64_t n, int64_t Kp,
                      const I8Epilogue& ep) {
                    return LaunchI8Fused<false>(ag, Bp, bsums, f, min_a, max_a, min_b,
                                         max_b, C, min_out, max_out, m, n, Kp,
                                         ep, stream);
                  });
}

extern "C" hipError_t stf_conv2d_i8_fused(
    const void* x_or_col, int implicit, const void* wp, const int32_t* wsums,
    const float* bias, const float* min_x, const float* max_x,
    const float* min_w, const float* max_w, const float* req_min,
    const float* req_max, int activation, uint8_t* y, float* min_out,
    float* max_out, const StfConvGeom* g, hipStream_t stream) {
  I8FusedArgs f{bias, req_min, req_max, activation, {}};
  return ConvWith(x_or_col, implicit, g,
                  [&](const auto& ag, int64_t m, int64_t n, int64_t Kp,
                      const I8Epilogue& ep) {
                    return LaunchI8Fused<false>(ag, wp, wsums, f, min_x, max_x, min_w,
                                         max_w, y, min_out, max_out, m, n, Kp,
                                         ep, stream);
                  });
}

extern "C" hipError_t stf_conv2d_i8_fused_sum(
    const void* x_or_col, int implicit, const void* wp, const int32_t* wsums,
    const float* bias, const uint8_t* summand, const float* min_x,
    const float* max_x, const float* min_w, const float* max_w,
    const float* min_s, const float* max_s, const float* req_min,
    const float* req_max, int activation, uint8_t* y, float* min_out,
    float* max_out, const StfConvGeom* g, hipStream_t stream) {
  I8FusedArgs f{bias, req_min, req_max, activation, {summand, min_s, max_s}};
  return ConvWith(x_or_col, implicit, g,
                  [&](const auto& ag, int64_t m, int64_t n, int64_t Kp,
                      const I8Epilogue& ep) {
                    return LaunchI8Fused<true>(ag, wp, wsums, f, min_x, max_x,
                                               min_w, max_w, y, min_out,
                                               max_out, m, n, Kp, ep, stream);
                  });
}
