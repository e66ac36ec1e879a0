// float32 Conv2D, backprop-input and backprop-filter as one implicit-GEMM
// kernel on v_mfma_f32_16x16x4_f32: native f32 in and out, f32 accumulation,
// no bf16 round trip. NHWC x and dy, [r][s][c][cout] filter.
//
// All three are C[M][N] = sum_k A[m][k] * B[k][n] with gathered operands:
//
//   FWD  m = (n,p,q)  k = (r,s,c)   n = ko   A = x at (n, p*sh-ph+r, q*sw-pw+s, c)
//                                            B = w[k][ko]           (as stored)
//   DX   m = (n,h,w)  k = (r,s,ko)  n = c    A = dy at (n, (h+ph-r)/sh,
//                                                (w+pw-s)/sw, ko), exact
//                                                divisions inside [0,p)x[0,q)
//                                            B = w[r][s][c][ko]  (+ side)
//   DW   m = (r,s,c)  k = (n,p,q)   n = ko   A = x at (n, p*sh-ph+r, q*sw-pw+s, c)
//                                            B = dy[k][ko]          (as stored)
//
// Whatever falls outside the image, the matrix or the block's k range is 0.
// The one DX gather form serves every stride: no col2im, no column buffer.
//
// Tile. 256 threads (4 waves) own a 128 x 64 tile of C and walk k in steps of
// 16. The waves sit 2 x 2, each with 4 x 2 MFMA tiles of 16x16 = 32
// accumulator registers; one k step is 4 MFMA sub-steps of k = 4, each reading
// 4 A and 2 B fragments (one f32 per lane each) for 8 MFMAs. A wider wave
// tile would cut LDS reads per MFMA further, but the tutorial convnets this
// kernel is for have cout 32 and 64: with BN = 64 no column of the tile is
// wasted there, and BM = 128 keeps M = n*p*q grids above 256 blocks at batch
// 128.
//
// LDS. Both tiles are k-major, As[k][128 + 16] and Bs[k][64 + 16], twice
// (28 KiB): step i+1 is gathered into registers before the MFMAs of step i
// and stored to the other buffer after them, one barrier per step. A
// fragment read takes 16 consecutive floats from each of 4 consecutive k
// rows; the row strides 144 and 80 are 16 mod 64, so the four rows fall on
// four disjoint groups of 16 banks.
//
// Staging goes through registers because every gather zero-fills, and it has
// two granularities per operand, template arguments EA and EB: 4 (one
// 16-byte load) when the operand's contiguous extent (c for x, cout for dy
// and w) is a multiple of 4 and its base is 16-byte aligned, else 1. A run of
// 4 then never crosses a tap or an image edge. Two thread layouts:
//   k-contiguous operands (FWD A, DX A and B): a thread owns one tile row
//     and 8 (A) or 4 (B) consecutive k; lanes run along the rows, so the LDS
//     stores of a wave hit consecutive banks.
//   row-contiguous operands (FWD B, DW A and B): a thread owns E consecutive
//     rows at a few k, 256*E/rows apart; a 4-run is one 16-byte LDS store.
// No divisions in the loop: the row's (n,p,q) / (n,h,w) / (r,s,c) is decoded
// once into a base offset and an origin, and the contraction index is kept as
// three counters advanced by pre-decomposed steps (Advance). DX's division
// by the stride is the multiply-shift of U32Div, skipped at stride 1.
//
// DW splits the pixel range over gridDim.z in slices that are multiples of
// 16; with more than one slice the blocks atomicAdd into the zeroed output
// (the op's own f32 tensor), with one they store. Offsets are 32-bit:
// stf_conv2d_f32_ok says whether a geometry fits.
//
// Resources (gfx950 cross-compile, all 12 instantiations): 37 to 44 VGPRs
// plus the 32 accumulator AGPRs, no scratch, 28 KiB LDS, 5 waves per SIMD.
// The file is built without packed f32 VALU ops like the other conv kernels
// of this directory (Makefile); it has none to form, and the counts are the
// same with and without the flag.
#include <climits>

#include "hip_common.h"
#include "stf_kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int BM = 128, BN = 64, BK = 16;
constexpr int LDA = BM + 16, LDB = BN + 16;

enum Mode { FWD = 0, DX = 1, DW = 2 };

struct Params {
  const float* a;     // FWD x, DX dy, DW x
  const float* b;     // FWD w, DX w, DW dy
  const float* side;  // DX: optional [M][N] added in the epilogue
  float* out;         // [M][N]
  int n, h, w, c, r, s, sh, sw, ph, pw, p, q, cout;
  int M, N, K;
  int kslice;  // k extent of one gridDim.z slice, a multiple of BK
  int d1, d2;  // the two inner extents of the contraction index
  U32Div div_sh, div_sw;  // DX only
};

// The contraction index as (i0, i1, i2) over extents (., d1, d2), i2 fastest.
struct Ctr {
  int i0, i1, i2;
};

__device__ __forceinline__ Ctr MakeCtr(int k, int d1, int d2) {
  Ctr c;
  int hi = k / d2;
  c.i2 = k - hi * d2;
  c.i0 = hi / d1;
  c.i1 = hi - c.i0 * d1;
  return c;
}

// c += step, where step = MakeCtr(distance): at most one carry per level.
__device__ __forceinline__ void Advance(Ctr& c, const Ctr& step, int d1,
                                        int d2) {
  c.i2 += step.i2;
  if (c.i2 >= d2) { c.i2 -= d2; ++c.i1; }
  c.i1 += step.i1;
  if (c.i1 >= d1) { c.i1 -= d1; ++c.i0; }
  c.i0 += step.i0;
}

// A tile row decoded once: element offset of its fixed part and the origin
// its taps are measured from.
struct Row {
  int base, o0, o1;
  bool ok;
};

// Element offset of A[row][k], or -1 where the operand is 0.
template <int MODE>
__device__ __forceinline__ int OffsetA(const Params& p, const Row& rw,
                                       const Ctr& k) {
  if (MODE == FWD) {  // k = (r, s, c)
    int h = rw.o0 + k.i0, w = rw.o1 + k.i1;
    if ((unsigned)h >= (unsigned)p.h || (unsigned)w >= (unsigned)p.w)
      return -1;
    return rw.base + (h * p.w + w) * p.c + k.i2;
  }
  if (MODE == DX) {  // k = (r, s, ko)
    int th = rw.o0 - k.i0, tw = rw.o1 - k.i1;
    if (th < 0 || tw < 0) return -1;
    int yp = (int)p.div_sh.div((uint32_t)th);
    int yq = (int)p.div_sw.div((uint32_t)tw);
    if (yp * p.sh != th || yq * p.sw != tw || yp >= p.p || yq >= p.q)
      return -1;
    return rw.base + (yp * p.q + yq) * p.cout + k.i2;
  }
  // DW: k = (n, p, q); the row is (r - ph, s - pw, c)
  int h = k.i1 * p.sh + rw.o0, w = k.i2 * p.sw + rw.o1;
  if ((unsigned)h >= (unsigned)p.h || (unsigned)w >= (unsigned)p.w) return -1;
  return ((k.i0 * p.h + h) * p.w + w) * p.c + rw.base;
}

template <int E>
__device__ __forceinline__ void Load(const float* __restrict__ base, int off,
                                     float* v) {
  if (E == 4) {
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    if (off >= 0) t = *reinterpret_cast<const f32x4*>(base + off);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else {
    v[0] = off >= 0 ? base[off] : 0.f;
  }
}

template <int E>
__device__ __forceinline__ void StoreRun(float* dst, const float* v) {
  if (E == 4) {
    f32x4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(dst) = t;
  } else {
    dst[0] = v[0];
  }
}

template <int MODE, int EA, int EB>
__launch_bounds__(kThreads) __global__ void ConvF32(const Params p) {
  __shared__ __attribute__((aligned(16))) float As[2][BK][LDA];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK][LDB];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int kbeg = blockIdx.z * p.kslice;
  const int kend = min(p.K, kbeg + p.kslice);
  const int nsteps = (kend - kbeg + BK - 1) / BK;

  // ---- which part of the two tiles this thread stages ----
  constexpr bool kAKc = MODE != DW;  // A contiguous along k (else along rows)
  constexpr bool kBKc = MODE == DX;
  constexpr int kAUnits = kAKc ? BM : BM / EA;  // threads along the rows
  constexpr int kBUnits = kBKc ? BN : BN / EB;
  constexpr int kALoads = 8 / EA, kBLoads = 4 / EB;  // per thread and step
  // k distance between two loads of a thread
  constexpr int kAStride = kAKc ? EA : kThreads / kAUnits;
  constexpr int kBStride = kBKc ? EB : kThreads / kBUnits;
  const int a_row = kAKc ? t % BM : (t % kAUnits) * EA;
  const int a_k = kAKc ? (t / BM) * 8 : t / kAUnits;
  const int b_row = kBKc ? t % BN : (t % kBUnits) * EB;
  const int b_k = kBKc ? (t / BN) * 4 : t / kBUnits;

  // ---- rows, decoded once ----
  Row ar;
  {
    int m = m0 + a_row;
    ar.ok = m < p.M;
    m = min(m, p.M - 1);
    if (MODE == FWD) {  // (n, p, q)
      int img = m / (p.p * p.q), pq = m - img * (p.p * p.q);
      int yp = pq / p.q, yq = pq - yp * p.q;
      ar.base = img * p.h * p.w * p.c;
      ar.o0 = yp * p.sh - p.ph;
      ar.o1 = yq * p.sw - p.pw;
    } else if (MODE == DX) {  // (n, h, w)
      int img = m / (p.h * p.w), hw = m - img * (p.h * p.w);
      int xh = hw / p.w, xw = hw - xh * p.w;
      ar.base = img * p.p * p.q * p.cout;
      ar.o0 = xh + p.ph;
      ar.o1 = xw + p.pw;
    } else {  // (r, s, c)
      int fr = m / (p.s * p.c), sc = m - fr * (p.s * p.c);
      int fs = sc / p.c;
      ar.base = sc - fs * p.c;
      ar.o0 = fr - p.ph;
      ar.o1 = fs - p.pw;
    }
  }
  // DX's B row is the input channel n0 + b_row of w[r][s][c][ko]
  const int b_col = n0 + b_row;
  const bool b_ok = b_col < p.N;
  const int b_base = kBKc ? min(b_col, p.N - 1) * p.cout : b_col;

  // ---- contraction counters ----
  const int d1 = p.d1, d2 = p.d2;
  int ak = kbeg + a_k, bk = kbeg + b_k;
  Ctr ac = MakeCtr(ak, d1, d2), bc = MakeCtr(bk, d1, d2);
  const Ctr step_bk = MakeCtr(BK, d1, d2);
  const Ctr step_a = MakeCtr(kAStride, d1, d2);
  const Ctr step_b = MakeCtr(kBStride, d1, d2);

  float ra[8], rb[4];
  auto gather = [&]() {
    Ctr cur = ac;
#pragma unroll
    for (int j = 0; j < kALoads; ++j) {
      int off = -1;
      if (ar.ok && ak + j * kAStride < kend) off = OffsetA<MODE>(p, ar, cur);
      Load<EA>(p.a, off, ra + j * EA);
      Advance(cur, step_a, d1, d2);
    }
    Advance(ac, step_bk, d1, d2);
    ak += BK;
    if (kBKc) {  // w[(r*s + s)*c + col][ko]
      cur = bc;
#pragma unroll
      for (int j = 0; j < kBLoads; ++j) {
        int off = -1;
        if (b_ok && bk + j * kBStride < kend)
          off = (cur.i0 * p.s + cur.i1) * p.c * p.cout + b_base + cur.i2;
        Load<EB>(p.b, off, rb + j * EB);
        Advance(cur, step_b, d1, d2);
      }
      Advance(bc, step_bk, d1, d2);
    } else {  // B[k][col], rows of N
#pragma unroll
      for (int j = 0; j < kBLoads; ++j) {
        int k = bk + j * kBStride;
        Load<EB>(p.b, b_ok && k < kend ? k * p.N + b_base : -1, rb + j * EB);
      }
    }
    bk += BK;
  };
  auto stage = [&](int buf) {
    if (kAKc) {
#pragma unroll
      for (int i = 0; i < 8; ++i) As[buf][a_k + i][a_row] = ra[i];
    } else {
#pragma unroll
      for (int j = 0; j < kALoads; ++j)
        StoreRun<EA>(&As[buf][a_k + j * kAStride][a_row], ra + j * EA);
    }
    if (kBKc) {
#pragma unroll
      for (int i = 0; i < 4; ++i) Bs[buf][b_k + i][b_row] = rb[i];
    } else {
#pragma unroll
      for (int j = 0; j < kBLoads; ++j)
        StoreRun<EB>(&Bs[buf][b_k + j * kBStride][b_row], rb + j * EB);
    }
  };

  // ---- main loop ----
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 32;
  const int lr = lane & 15, lk = lane >> 4;
  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (nsteps > 0) {
    gather();
    stage(0);
  }
  __syncthreads();
  for (int it = 0; it < nsteps; ++it) {
    const int buf = it & 1;
    const bool more = it + 1 < nsteps;
    if (more) gather();
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      float a[4], b[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[buf][kk + lk][wm + i * 16 + lr];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = Bs[buf][kk + lk][wn + j * 16 + lr];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j],
                                                           acc[i][j], 0, 0, 0);
    }
    if (more) stage(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue: lane holds rows 4*(lane/16) + 0..3 of column lane%16 ----
  const bool atomic = MODE == DW && gridDim.z > 1;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int col = n0 + wn + j * 16 + lr;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int row = m0 + wm + i * 16 + lk * 4 + e;
        if (row >= p.M || col >= p.N) continue;
        int idx = row * p.N + col;
        float v = acc[i][j][e];
        if (MODE == DX && p.side) v += p.side[idx];
        if (atomic) atomicAdd(p.out + idx, v);
        else p.out[idx] = v;
      }
    }
}

bool Aligned16(const void* ptr) { return ((uintptr_t)ptr & 15) == 0; }

Params MakeParams(const StfConvGeom& g) {
  Params p = {};
  p.n = g.n; p.h = g.h; p.w = g.w; p.c = g.c; p.r = g.r; p.s = g.s;
  p.sh = g.sh; p.sw = g.sw; p.ph = g.ph; p.pw = g.pw; p.p = g.p; p.q = g.q;
  p.cout = (int)g.cout;
  p.div_sh.init((uint32_t)g.sh);
  p.div_sw.init((uint32_t)g.sw);
  return p;
}

template <int MODE>
hipError_t Launch(Params p, bool vec_a, bool vec_b, int splits,
                  hipStream_t stream) {
  if (p.M == 0 || p.N == 0) return hipSuccess;
  // an empty contraction still writes its zeros; the extents only have to
  // be divisible by
  p.d1 = p.d1 > 0 ? p.d1 : 1;
  p.d2 = p.d2 > 0 ? p.d2 : 1;
  int ksteps = (p.K + BK - 1) / BK;
  if (ksteps < 1) ksteps = 1;
  if (splits < 1) splits = 1;
  if (splits > ksteps) splits = ksteps;
  p.kslice = (ksteps + splits - 1) / splits * BK;
  int slices = (ksteps * BK + p.kslice - 1) / p.kslice;
  dim3 grid((uint32_t)((p.M + BM - 1) / BM), (uint32_t)((p.N + BN - 1) / BN),
            (uint32_t)slices);
  DispatchBool(vec_a, [&](auto va) {
    DispatchBool(vec_b, [&](auto vb) {
      constexpr int EA = decltype(va)::value ? 4 : 1;
      constexpr int EB = decltype(vb)::value ? 4 : 1;
      hipLaunchKernelGGL((ConvF32<MODE, EA, EB>), grid, dim3(kThreads), 0,
                         stream, p);
    });
  });
  return hipGetLastError();
}

}  // namespace

extern "C" int stf_conv2d_f32_ok(const StfConvGeom* g) {
  if (g->cout < 0 || g->cout > INT_MAX) return 0;
  // every element offset, and a tile or a k step past the end, in an int
  const int64_t lim = INT_MAX - 4 * BM;
  int64_t x = (int64_t)g->n * g->h * g->w;
  int64_t y = (int64_t)g->n * g->p * g->q;
  int64_t f = (int64_t)g->r * g->s;
  if (x > lim || y > lim || f > lim) return 0;  // before the products below
  if (x * g->c > lim || y * g->cout > lim) return 0;
  if (f * g->c > lim || f * g->cout > lim) return 0;
  if (f * g->c * g->cout > lim) return 0;
  if ((int64_t)g->h + g->r + g->ph > lim || (int64_t)g->w + g->s + g->pw > lim)
    return 0;
  int64_t wide = g->cout > g->c ? g->cout : g->c;
  return (wide + BN - 1) / BN <= 65535;  // gridDim.y
}

extern "C" hipError_t stf_conv2d_f32_fwd(const void* x, const void* w, void* y,
                                         const StfConvGeom* g,
                                         hipStream_t stream) {
  if (!stf_conv2d_f32_ok(g)) return hipErrorInvalidValue;
  Params p = MakeParams(*g);
  p.a = (const float*)x;
  p.b = (const float*)w;
  p.out = (float*)y;
  p.M = g->n * g->p * g->q;
  p.N = p.cout;
  p.K = g->r * g->s * g->c;
  p.d1 = g->s;
  p.d2 = g->c;
  return Launch<FWD>(p, g->c % 4 == 0 && Aligned16(x),
                     p.cout % 4 == 0 && Aligned16(w), 1, stream);
}

extern "C" hipError_t stf_conv2d_f32_dx(const void* dy, const void* w,
                                        const void* side_or_null, void* dx,
                                        const StfConvGeom* g,
                                        hipStream_t stream) {
  if (!stf_conv2d_f32_ok(g)) return hipErrorInvalidValue;
  Params p = MakeParams(*g);
  p.a = (const float*)dy;
  p.b = (const float*)w;
  p.side = (const float*)side_or_null;
  p.out = (float*)dx;
  p.M = g->n * g->h * g->w;
  p.N = g->c;
  p.K = g->r * g->s * p.cout;
  p.d1 = g->s;
  p.d2 = p.cout;
  bool vec = p.cout % 4 == 0;
  return Launch<DX>(p, vec && Aligned16(dy), vec && Aligned16(w), 1, stream);
}

extern "C" hipError_t stf_conv2d_f32_dw(const void* x, const void* dy,
                                        void* dw, const StfConvGeom* g,
                                        int splits, hipStream_t stream) {
  if (!stf_conv2d_f32_ok(g)) return hipErrorInvalidValue;
  Params p = MakeParams(*g);
  p.a = (const float*)x;
  p.b = (const float*)dy;
  p.out = (float*)dw;
  p.M = g->r * g->s * g->c;
  p.N = p.cout;
  p.K = g->n * g->p * g->q;
  p.d1 = g->p;
  p.d2 = g->q;
  return Launch<DW>(p, g->c % 4 == 0 && Aligned16(x),
                    p.cout % 4 == 0 && Aligned16(dy), splits, stream);
}
