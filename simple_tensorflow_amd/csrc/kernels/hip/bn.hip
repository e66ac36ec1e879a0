// Batch norm forward/backward over x[rows, C] (NHWC flattened), f32 math and
// f32 statistics. (Replaces reference fused_batch_norm_op — redesigned for
// wave64 + LDS per the CDNA4 guide, not translated.)
//
// Two kernel families, chosen by UseV9() below and nowhere else:
//   V9      bf16 with C % 8 == 0: 16B loads/stores, fixed channel window.
//   scalar  everything else: f32 for any C, bf16 with C % 8 != 0.
#include "hip_common.h"
#include "stf_kernels.h"

namespace {

// ---------------- scalar kernels ----------------
// pass 1: per-channel sum and sumsq into f32 accumulators [2C] (zeroed).
// All 256 threads stream elements, accumulating via LDS atomics —
// wave64-coalesced regardless of C.
template <typename T>
__global__ void BnStatsKernel(const T* __restrict__ x, float* __restrict__ acc,
                              int64_t rows, int c) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s1 = (float*)smem;        // [c]
  float* s2 = s1 + c;              // [c]
  for (int i = threadIdx.x; i < c; i += blockDim.x) {
    s1[i] = 0.f;
    s2[i] = 0.f;
  }
  __syncthreads();
  int64_t n = rows * c;
  int64_t gstride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gstride) {
    float f = (float)x[i];
    int ch = (int)(i % c);
    atomicAdd(&s1[ch], f);
    atomicAdd(&s2[ch], f * f);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < c; i += blockDim.x) {
    atomicAdd(&acc[i], s1[i]);
    atomicAdd(&acc[c + i], s2[i]);
  }
}

// pass 2: finalize mean/var; write mean, var, inv_std (both families)
__global__ void BnFinalizeKernel(const float* __restrict__ acc,
                                 float* __restrict__ mean,
                                 float* __restrict__ var,
                                 float* __restrict__ inv_std, int64_t rows,
                                 int c, float eps) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c) return;
  float m = acc[i] / rows;
  float v = acc[c + i] / rows - m * m;
  v = v > 0.f ? v : 0.f;
  mean[i] = m;
  var[i] = v;
  inv_std[i] = rsqrtf(v + eps);
}

// pass 3: normalize (+ optional relu)
template <typename T, bool RELU>
__global__ void BnNormKernel(const T* __restrict__ x,
                             const float* __restrict__ mean,
                             const float* __restrict__ inv_std,
                             const float* __restrict__ scale,
                             const float* __restrict__ offset,
                             T* __restrict__ y, int64_t n, int c) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int ch = (int)(i % c);
    float v = ((float)x[i] - mean[ch]) * inv_std[ch] * scale[ch] + offset[ch];
    if (RELU) v = v > 0.f ? v : 0.f;
    y[i] = (T)v;
  }
}

// bwd pass 1: per-channel sum(dy), sum(dy * xhat) (both zeroed).
// RELU: the forward was BN+ReLU fused; dy is masked by y>0 on the fly so no
// separate relu-grad elementwise pass (or its memory traffic) is needed.
template <typename T, bool RELU>
__global__ void BnGradStatsKernel(const T* __restrict__ dy,
                                  const T* __restrict__ x,
                                  const T* __restrict__ yr,
                                  const float* __restrict__ mean,
                                  const float* __restrict__ inv_std,
                                  float* __restrict__ sum_dy,
                                  float* __restrict__ sum_dy_xhat,
                                  int64_t rows, int c) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s1 = (float*)smem;
  float* s2 = s1 + c;
  for (int i = threadIdx.x; i < c; i += blockDim.x) {
    s1[i] = 0.f;
    s2[i] = 0.f;
  }
  __syncthreads();
  int64_t n = rows * c;
  int64_t gstride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gstride) {
    int ch = (int)(i % c);
    float gf = (float)dy[i];
    if (RELU && (float)yr[i] <= 0.f) gf = 0.f;
    float xhat = ((float)x[i] - mean[ch]) * inv_std[ch];
    atomicAdd(&s1[ch], gf);
    atomicAdd(&s2[ch], gf * xhat);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < c; i += blockDim.x) {
    atomicAdd(&sum_dy[i], s1[i]);
    atomicAdd(&sum_dy_xhat[i], s2[i]);
  }
}

// bwd pass 2: dx = scale*inv_std*(dy - sum_dy/rows - xhat*sum_dy_xhat/rows)
// DSIDE (with RELU, the BN+add+ReLU tail): dy and yr are in registers here, so
// the residual branch's gradient dside = yr > 0 ? dy : 0 is one more store
// instead of a separate pass. A NaN in yr gives 0, as the relu-grad op does.
template <typename T, bool RELU, bool DSIDE>
__global__ void BnGradKernel(const T* __restrict__ dy, const T* __restrict__ x,
                             const T* __restrict__ yr,
                             const float* __restrict__ mean,
                             const float* __restrict__ inv_std,
                             const float* __restrict__ scale,
                             const float* __restrict__ sum_dy,
                             const float* __restrict__ sum_dy_xhat,
                             T* __restrict__ dx, T* __restrict__ dside,
                             int64_t n, int64_t rows, int c) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  float inv_rows = 1.f / (float)rows;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int ch = (int)(i % c);
    float xhat = ((float)x[i] - mean[ch]) * inv_std[ch];
    float g = (float)dy[i];
    if (RELU && (float)yr[i] <= 0.f) g = 0.f;
    dx[i] = (T)(scale[ch] * inv_std[ch] *
                (g - sum_dy[ch] * inv_rows -
                 xhat * sum_dy_xhat[ch] * inv_rows));
    if (DSIDE) dside[i] = (T)((float)yr[i] > 0.f ? (float)dy[i] : 0.f);
  }
}

// ---------------- V9: fixed-channel-window kernels (bf16, C % 8 == 0) ------
// Each thread owns ONE 8-channel window for its whole lifetime and strides
// over rows: no per-iteration modulo (64-bit int div/mod stalls wave issue),
// per-channel parameters hoisted into registers once, and for the reduction
// kernels the private partials flush to LDS exactly once.
struct BnIdx {
  int nw;          // channel windows (c/8)
  int w;           // this thread's window
  int64_t chunk;   // row-chunk id
  int64_t chunks;  // number of row chunks
  bool active;
};

__device__ __forceinline__ BnIdx BnThreadIndex(int c, int64_t rows) {
  BnIdx ix;
  ix.nw = c >> 3;
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  ix.chunks = nthreads / ix.nw;
  if (ix.chunks > rows) ix.chunks = rows;
  if (ix.chunks < 1) ix.chunks = 1;
  ix.w = (int)(tid % ix.nw);
  ix.chunk = tid / ix.nw;
  ix.active = ix.chunk < ix.chunks;
  return ix;
}

inline int BnGridV9(int c, int64_t rows) {
  int nw = c >> 3;
  // ~131k threads / 512 blocks measured FASTER than 1.5k blocks (the
  // per-block LDS zero/flush overhead beats the extra latency hiding).
  int64_t chunks = (131072 + nw - 1) / nw;
  if (chunks > rows) chunks = rows;
  if (chunks < 1) chunks = 1;
  return (int)((nw * chunks + 255) / 256) + 1;
}

// 8 bf16 = one 16B access; p must be 16B-aligned.
__device__ __forceinline__ void Load8(__bf16 (&v)[8], const __bf16* p) {
  *(ulong2*)v = *(const ulong2*)p;
}
__device__ __forceinline__ void Store8(__bf16* p, __bf16 (&v)[8]) {
  *(ulong2*)p = *(ulong2*)v;
}

__global__ void BnStatsKernelV9(const __bf16* __restrict__ x,
                                float* __restrict__ acc, int64_t rows,
                                int c) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s1 = (float*)smem;
  float* s2 = s1 + c;
  for (int i = threadIdx.x; i < c; i += blockDim.x) {
    s1[i] = 0.f;
    s2[i] = 0.f;
  }
  __syncthreads();
  BnIdx ix = BnThreadIndex(c, rows);
  float p1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float p2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (ix.active) {
    const __bf16* base = x + (int64_t)ix.w * 8;
    for (int64_t r = ix.chunk; r < rows; r += ix.chunks) {
      __bf16 v[8];
      Load8(v, base + r * c);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float f = (float)v[e];
        p1[e] += f;
        p2[e] += f * f;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      atomicAdd(&s1[ix.w * 8 + e], p1[e]);
      atomicAdd(&s2[ix.w * 8 + e], p2[e]);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < c; i += blockDim.x)
    if (s1[i] != 0.f || s2[i] != 0.f) {
      atomicAdd(&acc[i], s1[i]);
      atomicAdd(&acc[c + i], s2[i]);
    }
}

template <bool RELU>
__global__ void BnNormKernelV9(const __bf16* __restrict__ x,
                               const float* __restrict__ mean,
                               const float* __restrict__ inv_std,
                               const float* __restrict__ scale,
                               const float* __restrict__ offset,
                               __bf16* __restrict__ y, int64_t rows, int c) {
  BnIdx ix = BnThreadIndex(c, rows);
  if (!ix.active) return;
  int cb = ix.w * 8;
  float m[8], is[8], sc[8], of[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    m[e] = mean[cb + e];
    is[e] = inv_std[cb + e] * scale[cb + e];
    sc[e] = is[e];
    of[e] = offset[cb + e] - m[e] * is[e];
  }
  for (int64_t r = ix.chunk; r < rows; r += ix.chunks) {
    __bf16 v[8], o[8];
    Load8(v, x + r * c + cb);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float f = (float)v[e] * sc[e] + of[e];
      if (RELU) f = f > 0.f ? f : 0.f;
      o[e] = (__bf16)f;
    }
    Store8(y + r * c + cb, o);
  }
}

// BN + residual add + relu in one pass (the bottleneck tail:
// relu(bn(conv_out) + shortcut)) — saves two full elementwise passes.
__global__ void BnNormAddReluKernelV9(const __bf16* __restrict__ x,
                                      const __bf16* __restrict__ side,
                                      const float* __restrict__ mean,
                                      const float* __restrict__ inv_std,
                                      const float* __restrict__ scale,
                                      const float* __restrict__ offset,
                                      __bf16* __restrict__ y, int64_t rows,
                                      int c) {
  BnIdx ix = BnThreadIndex(c, rows);
  if (!ix.active) return;
  int cb = ix.w * 8;
  float sc[8], of[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sc[e] = inv_std[cb + e] * scale[cb + e];
    of[e] = offset[cb + e] - mean[cb + e] * sc[e];
  }
  for (int64_t r = ix.chunk; r < rows; r += ix.chunks) {
    __bf16 v[8], sd[8], o[8];
    Load8(v, x + r * c + cb);
    Load8(sd, side + r * c + cb);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float f = (float)v[e] * sc[e] + of[e] + (float)sd[e];
      o[e] = (__bf16)(f > 0.f ? f : 0.f);
    }
    Store8(y + r * c + cb, o);
  }
}

template <bool RELU>
__global__ void BnGradStatsKernelV9(const __bf16* __restrict__ dy,
                                    const __bf16* __restrict__ x,
                                    const __bf16* __restrict__ yr,
                                    const float* __restrict__ mean,
                                    const float* __restrict__ inv_std,
                                    float* __restrict__ sum_dy,
                                    float* __restrict__ sum_dy_xhat,
                                    int64_t rows, int c) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s1 = (float*)smem;
  float* s2 = s1 + c;
  for (int i = threadIdx.x; i < c; i += blockDim.x) {
    s1[i] = 0.f;
    s2[i] = 0.f;
  }
  __syncthreads();
  BnIdx ix = BnThreadIndex(c, rows);
  float p1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float p2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (ix.active) {
    int cb = ix.w * 8;
    float mloc[8], iloc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      mloc[e] = mean[cb + e];
      iloc[e] = inv_std[cb + e];
    }
    int64_t off = (int64_t)cb;
    for (int64_t r = ix.chunk; r < rows; r += ix.chunks) {
      __bf16 g[8], xv[8], yv[8];
      Load8(g, dy + r * c + off);
      Load8(xv, x + r * c + off);
      if (RELU) Load8(yv, yr + r * c + off);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float gf = (float)g[e];
        if (RELU && (float)yv[e] <= 0.f) gf = 0.f;
        float xhat = ((float)xv[e] - mloc[e]) * iloc[e];
        p1[e] += gf;
        p2[e] += gf * xhat;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      atomicAdd(&s1[cb + e], p1[e]);
      atomicAdd(&s2[cb + e], p2[e]);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < c; i += blockDim.x)
    if (s1[i] != 0.f || s2[i] != 0.f) {
      atomicAdd(&sum_dy[i], s1[i]);
      atomicAdd(&sum_dy_xhat[i], s2[i]);
    }
}

template <bool RELU, bool DSIDE>
__global__ void BnGradKernelV9(const __bf16* __restrict__ dy,
                               const __bf16* __restrict__ x,
                               const __bf16* __restrict__ yr,
                               const float* __restrict__ mean,
                               const float* __restrict__ inv_std,
                               const float* __restrict__ scale,
                               const float* __restrict__ sum_dy,
                               const float* __restrict__ sum_dy_xhat,
                               __bf16* __restrict__ dx,
                               __bf16* __restrict__ dside, int64_t rows,
                               int c) {
  BnIdx ix = BnThreadIndex(c, rows);
  if (!ix.active) return;
  int cb = ix.w * 8;
  float inv_rows = 1.f / (float)rows;
  float m[8], is[8], k[8], a[8], b[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    m[e] = mean[cb + e];
    is[e] = inv_std[cb + e];
    k[e] = scale[cb + e] * is[e];
    a[e] = sum_dy[cb + e] * inv_rows;
    b[e] = sum_dy_xhat[cb + e] * inv_rows;
  }
  for (int64_t r = ix.chunk; r < rows; r += ix.chunks) {
    __bf16 g8[8], x8[8], y8[8], o[8], ds[8];
    Load8(g8, dy + r * c + cb);
    Load8(x8, x + r * c + cb);
    if (RELU) Load8(y8, yr + r * c + cb);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float xhat = ((float)x8[e] - m[e]) * is[e];
      float g = (float)g8[e];
      if (RELU && (float)y8[e] <= 0.f) g = 0.f;
      o[e] = (__bf16)(k[e] * (g - a[e] - xhat * b[e]));
      if (DSIDE) ds[e] = (__bf16)((float)y8[e] > 0.f ? (float)g8[e] : 0.f);
    }
    Store8(dx + r * c + cb, o);
    if (DSIDE) Store8(dside + r * c + cb, ds);
  }
}

// ---------------- column sums of per-tile partials ----------------
// acc[j] += sum_t partial[t][j] for the [tiles][cols] f32 partials that the
// 8-phase GEMM's STATS epilogue leaves. A block owns a 64-column strip
// (blockIdx.x) and every gridDim.y-th group of 4 rows (blockIdx.y), so a
// narrow matrix (the stem: 128 columns x 12544 tiles) still fills the GPU.
// The four row lanes combine in LDS; one f32 atomic per block and column
// then goes into the zeroed acc, a few KB in all.
__global__ void BnPartialSumsKernel(const float* __restrict__ partial,
                                    float* __restrict__ acc, int64_t tiles,
                                    int cols) {
  __shared__ float red[4][64];
  int lane_c = threadIdx.x & 63, lane_r = threadIdx.x >> 6;
  int col = blockIdx.x * 64 + lane_c;
  float sum = 0.f;
  if (col < cols)
    for (int64_t t = (int64_t)blockIdx.y * 4 + lane_r; t < tiles;
         t += (int64_t)gridDim.y * 4)
      sum += partial[t * cols + col];
  red[lane_r][lane_c] = sum;
  __syncthreads();
  if (lane_r == 0 && col < cols)
    atomicAdd(&acc[col], (red[0][lane_c] + red[1][lane_c]) +
                             (red[2][lane_c] + red[3][lane_c]));
}

// ---------------- dispatch ----------------
// The one rule: bf16 with C % 8 == 0 runs the V9 kernels; f32 for any C and
// bf16 with C % 8 != 0 run the scalar kernels.
inline bool UseV9(int dtype, int c) { return dtype != 0 && c % 8 == 0; }

// Both reduction families keep two f32 arrays [c] in LDS.
inline size_t BnLdsBytes(int c) { return (size_t)c * 2 * sizeof(float); }

// Forward pass 1: column sums and sums of squares of x into acc.
void LaunchBnSums(int dtype, const void* x, float* acc, int64_t rows, int c,
                  hipStream_t stream) {
  if (UseV9(dtype, c)) {
    hipLaunchKernelGGL(BnStatsKernelV9, dim3(BnGridV9(c, rows)), dim3(256),
                       BnLdsBytes(c), stream, (const __bf16*)x, acc, rows, c);
  } else {
    DispatchDtype(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      hipLaunchKernelGGL((BnStatsKernel<T>), dim3(512), dim3(256),
                         BnLdsBytes(c), stream, (const T*)x, acc, rows, c);
    });
  }
}

// Forward pass 2: acc -> mean/var/inv_std.
void LaunchBnFinalize(const float* acc, float* mean, float* var,
                      float* inv_std, int64_t rows, int c, float eps,
                      hipStream_t stream) {
  hipLaunchKernelGGL(BnFinalizeKernel, dim3((c + 255) / 256), dim3(256), 0,
                     stream, acc, mean, var, inv_std, rows, c, eps);
}

// Forward passes 1 + 2: batch statistics of x into mean/var/inv_std.
void LaunchBnStats(int dtype, const void* x, float* acc, float* mean,
                   float* var, float* inv_std, int64_t rows, int c, float eps,
                   hipStream_t stream) {
  LaunchBnSums(dtype, x, acc, rows, c, stream);
  LaunchBnFinalize(acc, mean, var, inv_std, rows, c, eps, stream);
}

// Forward pass 3: normalize (+ optional relu).
void LaunchBnNorm(int dtype, const void* x, const void* scale,
                  const void* offset, const float* mean, const float* inv_std,
                  void* y, int64_t rows, int c, int fuse_relu,
                  hipStream_t stream) {
  DispatchBool(fuse_relu, [&](auto relu) {
    constexpr bool RELU = decltype(relu)::value;
    if (UseV9(dtype, c)) {
      hipLaunchKernelGGL((BnNormKernelV9<RELU>), dim3(BnGridV9(c, rows)),
                         dim3(256), 0, stream, (const __bf16*)x, mean,
                         inv_std, (const float*)scale, (const float*)offset,
                         (__bf16*)y, rows, c);
      return;
    }
    DispatchDtype(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      int64_t n = rows * c;
      hipLaunchKernelGGL((BnNormKernel<T, RELU>), ElemwiseGrid(n, 256, 4),
                         dim3(256), 0, stream, (const T*)x, mean, inv_std,
                         (const float*)scale, (const float*)offset, (T*)y, n,
                         c);
    });
  });
}

}  // namespace

extern "C" {

hipError_t stf_bn_stats_only(int dtype, const void* x, float* acc, float* mean,
                             float* var, float* inv_std, int64_t rows, int c,
                             float eps, hipStream_t stream) {
  LaunchBnStats(dtype, x, acc, mean, var, inv_std, rows, c, eps, stream);
  return hipGetLastError();
}

hipError_t stf_bn_fwd(int dtype, const void* x, const void* scale,
                      const void* offset, float* acc, float* mean, float* var,
                      float* inv_std, void* y, int64_t rows, int c, float eps,
                      int fuse_relu, hipStream_t stream) {
  LaunchBnStats(dtype, x, acc, mean, var, inv_std, rows, c, eps, stream);
  LaunchBnNorm(dtype, x, scale, offset, mean, inv_std, y, rows, c, fuse_relu,
               stream);
  return hipGetLastError();
}

hipError_t stf_bn_fwd_acc(int dtype, const void* x, const void* scale,
                          const void* offset, const float* acc, float* mean,
                          float* var, float* inv_std, void* y, int64_t rows,
                          int c, float eps, int fuse_relu,
                          hipStream_t stream) {
  LaunchBnFinalize(acc, mean, var, inv_std, rows, c, eps, stream);
  LaunchBnNorm(dtype, x, scale, offset, mean, inv_std, y, rows, c, fuse_relu,
               stream);
  return hipGetLastError();
}

hipError_t stf_bn_sums(int dtype, const void* x, float* acc, int64_t rows,
                       int c, hipStream_t stream) {
  LaunchBnSums(dtype, x, acc, rows, c, stream);
  return hipGetLastError();
}

hipError_t stf_bn_partial_sums(const float* partial, float* acc,
                               int64_t tiles, int cols, hipStream_t stream) {
  if (tiles < 1 || cols < 1) return hipErrorInvalidValue;
  // About 1024 blocks, and no more row splits than leave a thread 4 rows.
  int strips = (cols + 63) / 64;
  int64_t splits = (tiles + 15) / 16;
  int64_t cap = strips >= 1024 ? 1 : 1024 / strips;
  if (splits > cap) splits = cap;
  hipLaunchKernelGGL(BnPartialSumsKernel, dim3(strips, (uint32_t)splits),
                     dim3(256), 0, stream, partial, acc, tiles, cols);
  return hipGetLastError();
}

hipError_t stf_bn_add_relu(const void* x, const void* side, const float* mean,
                           const float* inv_std, const void* scale,
                           const void* offset, void* y, int64_t rows, int c,
                           hipStream_t stream) {
  if (c % 8 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(BnNormAddReluKernelV9, dim3(BnGridV9(c, rows)),
                     dim3(256), 0, stream, (const __bf16*)x,
                     (const __bf16*)side, mean, inv_std, (const float*)scale,
                     (const float*)offset, (__bf16*)y, rows, c);
  return hipGetLastError();
}

hipError_t stf_bn_add_relu_acc(const void* x, const void* side,
                               const float* acc, float* mean, float* var,
                               float* inv_std, const void* scale,
                               const void* offset, void* y, int64_t rows,
                               int c, float eps, hipStream_t stream) {
  if (c % 8 != 0) return hipErrorInvalidValue;
  LaunchBnFinalize(acc, mean, var, inv_std, rows, c, eps, stream);
  return stf_bn_add_relu(x, side, mean, inv_std, scale, offset, y, rows, c,
                         stream);
}

hipError_t stf_bn_bwd(int dtype, const void* dy, const void* x,
                      const void* y_relu, const float* mean,
                      const float* inv_std, const void* scale,
                      float* sum_dy, float* sum_dy_xhat, void* dx,
                      void* dside, int64_t rows, int c, int fuse_relu,
                      hipStream_t stream) {
  if (dside && !fuse_relu) return hipErrorInvalidValue;
  DispatchBool(fuse_relu, [&](auto relu) {
    constexpr bool RELU = decltype(relu)::value;
    if (UseV9(dtype, c)) {
      dim3 g9(BnGridV9(c, rows));
      hipLaunchKernelGGL((BnGradStatsKernelV9<RELU>), g9, dim3(256),
                         BnLdsBytes(c), stream, (const __bf16*)dy,
                         (const __bf16*)x, (const __bf16*)y_relu, mean,
                         inv_std, sum_dy, sum_dy_xhat, rows, c);
      DispatchBool(RELU && dside, [&](auto ds) {
        constexpr bool DSIDE = RELU && decltype(ds)::value;
        hipLaunchKernelGGL((BnGradKernelV9<RELU, DSIDE>), g9, dim3(256), 0,
                           stream, (const __bf16*)dy, (const __bf16*)x,
                           (const __bf16*)y_relu, mean, inv_std,
                           (const float*)scale, sum_dy, sum_dy_xhat,
                           (__bf16*)dx, (__bf16*)dside, rows, c);
      });
      return;
    }
    DispatchDtype(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      int64_t n = rows * c;
      hipLaunchKernelGGL((BnGradStatsKernel<T, RELU>), dim3(512), dim3(256),
                         BnLdsBytes(c), stream, (const T*)dy, (const T*)x,
                         (const T*)y_relu, mean, inv_std, sum_dy, sum_dy_xhat,
                         rows, c);
      DispatchBool(RELU && dside, [&](auto ds) {
        constexpr bool DSIDE = RELU && decltype(ds)::value;
        hipLaunchKernelGGL((BnGradKernel<T, RELU, DSIDE>),
                           ElemwiseGrid(n, 256, 4), dim3(256), 0, stream,
                           (const T*)dy, (const T*)x, (const T*)y_relu, mean,
                           inv_std, (const float*)scale, sum_dy, sum_dy_xhat,
                           (T*)dx, (T*)dside, n, rows, c);
      });
    });
  });
  return hipGetLastError();
}

}  // extern "C"
