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
//
// The loaders and the K loop are in gemm_i8_core.h, shared with
// gemm_i8_fused.hip, which puts a bias + activation + requantize epilogue
// behind the same loop.
#include "gemm_i8_core.h"

namespace {

using namespace i8;

template <int WN, class AG>
__launch_bounds__(256) __global__ void GemmI8(
    AG ag, const uint8_t* __restrict__ Bp,  // packed s8 [N][Kp]
    const int32_t* __restrict__ bsums,      // [1 or 1 + taps][N]
    const float* __restrict__ min_a, const float* __restrict__ max_a,
    const float* __restrict__ min_b, const float* __restrict__ max_b,
    int32_t* __restrict__ C, float* __restrict__ min_out,
    float* __restrict__ max_out, int64_t M, int64_t N, int64_t Kp,
    I8Epilogue ep) {
  constexpr int WM = kWM;
  __shared__ __attribute__((aligned(16))) uint4 lds[LdsChunks(WN)];
  int64_t m0, n0;
  BlockOrigin<WN>(M, N, &m0, &n0);

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

  i32x4 acc[WM][WN], rs[WM];
  I8MainLoop<WN, false>(ag, Bp, M, N, Kp, m0, n0, lds, acc, rs);

  // ---- epilogue: C/D map col = lane & 15, row = (lane >> 4) * 4 + reg ----
  uint32_t ca = 128u - (uint32_t)stf::QuantZeroPoint(min_a[0], max_a[0]);
  uint32_t cb = 128u - (uint32_t)stf::QuantZeroPoint(min_b[0], max_b[0]);
  uint32_t cab = ca * cb;
#pragma unroll
  for (int i = 0; i < WM; ++i) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      int64_t row = m0 + wr * WM * 16 + i * 16 + (lane >> 4) * 4 + reg;
      if (row >= M) continue;
      I8Taps t = TapsOf(ep, row);
      uint32_t base = cb * (uint32_t)rs[i][reg] +
                      (uint32_t)t.nvalid * (uint32_t)ep.cper * cab;
#pragma unroll
      for (int j = 0; j < WN; ++j) {
        int64_t col = n0 + wc * WN * 16 + j * 16 + (lane & 15);
        if (col >= N) continue;
        uint32_t sb = TapSum(bsums, ep, t, N, col);
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
  return GemmWith(A, a_packed, M, N, K,
                  [&](const auto& ag, int64_t m, int64_t n, int64_t Kp,
                      const I8Epilogue& ep) {
                    return LaunchI8(ag, Bp, bsums, min_a, max_a, min_b, max_b,
                                    C, min_out, max_out, m, n, Kp, ep, stream);
                  });
}

extern "C" hipError_t stf_conv2d_i8(const void* x_or_col, int implicit,
                                    const void* wp, const int32_t* wsums,
                                    const float* min_x, const float* max_x,
                                    const float* min_w, const float* max_w,
                                    int32_t* y, float* min_out,
                                    float* max_out, const StfConvGeom* g,
                                    hipStream_t stream) {
  return ConvWith(x_or_col, implicit, g,
                  [&](const auto& ag, int64_t m, int64_t n, int64_t Kp,
                      const I8Epilogue& ep) {
                    return LaunchI8(ag, wp, wsums, min_x, max_x, min_w, max_w,
                                    y, min_out, max_out, m, n, Kp, ep, stream);
                  });
}
