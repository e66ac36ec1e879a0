// Max/avg pooling forward and backward, NHWC; f32 math. C % 8 == 0 bf16
// tensors take the 8-wide (16B load/store) kernels. (Replaces reference
// maxpooling_op_gpu, avgpooling_op_gpu — redesigned, not translated.)
#include "hip_common.h"
#include "stf_kernels.h"

namespace {

template <typename T, bool IS_MAX>
__global__ void PoolFwdKernel(const T* __restrict__ x, T* __restrict__ y,
                              StfPoolGeom g, int64_t total) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    int64_t rem = i;
    int c = (int)(rem % g.C); rem /= g.C;
    int q = (int)(rem % g.Q); rem /= g.Q;
    int p = (int)(rem % g.P); rem /= g.P;
    int n = (int)rem;
    float best = IS_MAX ? -3.4e38f : 0.f;
    int count = 0;
    for (int kh = 0; kh < g.kh; ++kh) {
      int ih = p * g.sh - g.ph + kh;
      if (ih < 0 || ih >= g.H) continue;
      for (int kw = 0; kw < g.kw; ++kw) {
        int iw = q * g.sw - g.pw + kw;
        if (iw < 0 || iw >= g.W) continue;
        float v = (float)x[((int64_t)(n * g.H + ih) * g.W + iw) * g.C + c];
        if (IS_MAX) best = fmaxf(best, v);
        else best += v;
        ++count;
      }
    }
    y[i] = (T)(IS_MAX ? best : best / count);
  }
}


// C%8==0 8-wide pooling (16B loads/stores, one index decomposition per 8
// channels, O(1) border-count instead of the nested window scan).
template <bool IS_MAX>
__global__ void PoolFwdKernelV8(const __bf16* __restrict__ x,
                                __bf16* __restrict__ y, StfPoolGeom g,
                                int64_t total8) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int c8 = g.C / 8;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total8;
       i += stride) {
    int64_t rem = i;
    int cw = (int)(rem % c8); rem /= c8;
    int q = (int)(rem % g.Q); rem /= g.Q;
    int p = (int)(rem % g.P); rem /= g.P;
    int n = (int)rem;
    int h0 = max(p * g.sh - g.ph, 0), h1 = min(p * g.sh - g.ph + g.kh, g.H);
    int w0 = max(q * g.sw - g.pw, 0), w1 = min(q * g.sw - g.pw + g.kw, g.W);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = IS_MAX ? -3.4e38f : 0.f;
    for (int ih = h0; ih < h1; ++ih)
      for (int iw = w0; iw < w1; ++iw) {
        __bf16 v[8];
        *(ulong2*)v = *(const ulong2*)(
            x + ((int64_t)(n * g.H + ih) * g.W + iw) * g.C + cw * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float f = (float)v[e];
          if (IS_MAX) acc[e] = fmaxf(acc[e], f);
          else acc[e] += f;
        }
      }
    float inv = IS_MAX ? 1.f : 1.f / ((h1 - h0) * (w1 - w0));
    __bf16 o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (__bf16)(IS_MAX ? acc[e] : acc[e] * inv);
    *(ulong2*)(y + ((int64_t)(n * g.P + p) * g.Q + q) * g.C + cw * 8) =
        *(ulong2*)o;
  }
}

__global__ void AvgPoolGradKernelV8(const __bf16* __restrict__ dy,
                                    __bf16* __restrict__ dx, StfPoolGeom g,
                                    int64_t total8) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int c8 = g.C / 8;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total8;
       i += stride) {
    int64_t rem = i;
    int cw = (int)(rem % c8); rem /= c8;
    int iw = (int)(rem % g.W); rem /= g.W;
    int ih = (int)(rem % g.H); rem /= g.H;
    int n = (int)rem;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // output rows whose window covers ih: p*sh <= ih+ph < p*sh+kh
    int plo = max((ih + g.ph - g.kh + g.sh) / g.sh, 0);
    int phi = min((ih + g.ph) / g.sh, g.P - 1);
    int qlo = max((iw + g.pw - g.kw + g.sw) / g.sw, 0);
    int qhi = min((iw + g.pw) / g.sw, g.Q - 1);
    for (int p = plo; p <= phi; ++p) {
      int h0 = max(p * g.sh - g.ph, 0);
      int h1 = min(p * g.sh - g.ph + g.kh, g.H);
      for (int q = qlo; q <= qhi; ++q) {
        int w0 = max(q * g.sw - g.pw, 0);
        int w1 = min(q * g.sw - g.pw + g.kw, g.W);
        float inv = 1.f / ((h1 - h0) * (w1 - w0));
        __bf16 v[8];
        *(ulong2*)v = *(const ulong2*)(
            dy + ((int64_t)(n * g.P + p) * g.Q + q) * g.C + cw * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += (float)v[e] * inv;
      }
    }
    __bf16 o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (__bf16)acc[e];
    *(ulong2*)(dx + i * 8) = *(ulong2*)o;
  }
}


// Per-INPUT max-pool gradient, 8 channels wide, no atomics/f32 scratch:
// each input pixel sums dy over the covering windows where it is the
// first argmax (scan order matches the per-output kernel's routing).
__global__ void MaxPoolGradKernelV8(const __bf16* __restrict__ x,
                                    const __bf16* __restrict__ dy,
                                    __bf16* __restrict__ dx, StfPoolGeom g,
                                    int64_t total8) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int c8 = g.C / 8;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total8;
       i += stride) {
    int64_t rem = i;
    int cw = (int)(rem % c8); rem /= c8;
    int iw = (int)(rem % g.W); rem /= g.W;
    int ih = (int)(rem % g.H); rem /= g.H;
    int n = (int)rem;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float self[8];
    {
      __bf16 v[8];
      *(ulong2*)v = *(const ulong2*)(
          x + ((int64_t)(n * g.H + ih) * g.W + iw) * g.C + cw * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) self[e] = (float)v[e];
    }
    int plo = max((ih + g.ph - g.kh + g.sh) / g.sh, 0);
    int phi = min((ih + g.ph) / g.sh, g.P - 1);
    int qlo = max((iw + g.pw - g.kw + g.sw) / g.sw, 0);
    int qhi = min((iw + g.pw) / g.sw, g.Q - 1);
    for (int p = plo; p <= phi; ++p) {
      for (int q = qlo; q <= qhi; ++q) {
        // first-argmax position per channel within this window
        float best[8];
        int bpos[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          best[e] = -3.4e38f;
          bpos[e] = -1;
        }
        for (int kh = 0; kh < g.kh; ++kh) {
          int h = p * g.sh - g.ph + kh;
          if (h < 0 || h >= g.H) continue;
          for (int kw = 0; kw < g.kw; ++kw) {
            int w = q * g.sw - g.pw + kw;
            if (w < 0 || w >= g.W) continue;
            __bf16 v[8];
            *(ulong2*)v = *(const ulong2*)(
                x + ((int64_t)(n * g.H + h) * g.W + w) * g.C + cw * 8);
            int pos = h * g.W + w;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              float f = (float)v[e];
              if (f > best[e]) {
                best[e] = f;
                bpos[e] = pos;
              }
            }
          }
        }
        __bf16 gv[8];
        *(ulong2*)gv = *(const ulong2*)(
            dy + ((int64_t)(n * g.P + p) * g.Q + q) * g.C + cw * 8);
        int mypos = ih * g.W + iw;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (bpos[e] == mypos) acc[e] += (float)gv[e];
      }
    }
    __bf16 o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (__bf16)acc[e];
    *(ulong2*)(dx + i * 8) = *(ulong2*)o;
  }
}

// Tiled max-pool gradient for 3x3 windows of stride 2, bf16, C % 8 == 0.
// A block owns a core of TH x TW input pixels by CS channels and every
// window that covers a core pixel: (TH/2+1) x (TW/2+1) of them, whose taps
// span a halo of (TH+3) x (TW+3) pixels. x reaches the block once (the halo,
// staged in LDS), each window's first argmax is found once (phase 1, one
// 4-bit tap number per channel, 15 = no winner) and each core pixel then
// sums dy over its covering windows in MaxPoolGradKernelV8's order (phase
// 2): same addends, same order, one rounding, so dx is bit-equal to it.
// Windows that straddle two cores are evaluated by both blocks.
template <int TH, int TW, int CS>
struct MaxPoolGradTile {
  static_assert(TH % 2 == 0 && TW % 2 == 0 && CS % 8 == 0, "tile shape");
  static constexpr int kThreads = 256;
  static constexpr int HR = TH + 3, HC = TW + 3;          // x halo, pixels
  static constexpr int WR = TH / 2 + 1, WC = TW / 2 + 1;  // windows
  static constexpr int CG = CS / 8;                       // 16-byte groups
};

template <int TH, int TW, int CS>
__global__ __launch_bounds__(256) void MaxPoolGradTiled(
    const __bf16* __restrict__ x, const __bf16* __restrict__ dy,
    __bf16* __restrict__ dx, StfPoolGeom g, int tiles_h, int tiles_w,
    int slices) {
  using T = MaxPoolGradTile<TH, TW, CS>;
  constexpr int HC = T::HC, WC = T::WC, CG = T::CG;
  __shared__ ulong2 halo[T::HR * HC * CG];
  __shared__ uint32_t argmax[T::WR * WC * CG];

  int b = blockIdx.x;
  const int slice = b % slices; b /= slices;
  const int tile_w = b % tiles_w; b /= tiles_w;
  const int tile_h = b % tiles_h;
  const int n = b / tiles_h;
  const int h0 = tile_h * TH, w0 = tile_w * TW, c0 = slice * CS;
  // first window (it may lie outside the output) that covers the core's
  // first row / column, and the image position of its first tap
  const int pb = (h0 + g.ph - 1) >> 1, qb = (w0 + g.pw - 1) >> 1;
  const int hr0 = pb * 2 - g.ph, wc0 = qb * 2 - g.pw;
  // 8-channel groups of this slice that exist
  const int ncg = min(CG, (g.C - c0) / 8);
  const int tid = threadIdx.x;

  // ---- stage the halo; what lies outside the image or past C is -inf,
  // which never passes `f > best`
  for (int i = tid; i < T::HR * HC * CG; i += T::kThreads) {
    int cg = i % CG, pix = i / CG;
    int h = hr0 + pix / HC, w = wc0 + pix % HC;
    ulong2 v;
    v.x = v.y = 0xFF80FF80FF80FF80ull;
    if (h >= 0 && h < g.H && w >= 0 && w < g.W && cg < ncg)
      v = *(const ulong2*)(
          x + ((int64_t)(n * g.H + h) * g.W + w) * g.C + c0 + cg * 8);
    halo[i] = v;
  }
  __syncthreads();

  // ---- phase 1: first argmax of every window, per channel
  for (int i = tid; i < T::WR * WC * CG; i += T::kThreads) {
    int cg = i % CG, win = i / CG;
    int jr = win / WC, jc = win % WC;
    float best[8];
    uint32_t tap[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      best[e] = -3.4e38f;
      tap[e] = 15;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        __bf16 v[8];
        *(ulong2*)v = halo[((2 * jr + a) * HC + 2 * jc + c) * CG + cg];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float f = (float)v[e];
          if (f > best[e]) {
            best[e] = f;
            tap[e] = a * 3 + c;
          }
        }
      }
    uint32_t word = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) word |= tap[e] << (4 * e);
    argmax[i] = word;
  }
  __syncthreads();

  // ---- phase 2: every core pixel inside the image gathers its dy
  for (int i = tid; i < TH * TW * CG; i += T::kThreads) {
    int cg = i % CG, pix = i / CG;
    int h = h0 + pix / TW, w = w0 + pix % TW;
    if (h >= g.H || w >= g.W || cg >= ncg) continue;
    // halo coordinates, >= 1; window j spans halo rows 2j .. 2j+2
    int lr = h - hr0, lc = w - wc0;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      int jr = ((lr - 1) >> 1) + a, p = pb + jr;
      if (jr > (lr >> 1) || p < 0 || p >= g.P) continue;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        int jc = ((lc - 1) >> 1) + c, q = qb + jc;
        if (jc > (lc >> 1) || q < 0 || q >= g.Q) continue;
        uint32_t word = argmax[(jr * WC + jc) * CG + cg];
        uint32_t mine = (lr - 2 * jr) * 3 + (lc - 2 * jc);
        __bf16 gv[8];
        *(ulong2*)gv = *(const ulong2*)(
            dy + ((int64_t)(n * g.P + p) * g.Q + q) * g.C + c0 + cg * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (((word >> (4 * e)) & 15) == mine) acc[e] += (float)gv[e];
      }
    }
    __bf16 o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (__bf16)acc[e];
    *(ulong2*)(dx + ((int64_t)(n * g.H + h) * g.W + w) * g.C + c0 + cg * 8) =
        *(ulong2*)o;
  }
}

// false (nothing launched) if the block count does not fit a 1-D grid.
template <int TH, int TW, int CS>
bool LaunchMaxPoolGradTiled(const void* x, const void* dy, void* dx,
                            const StfPoolGeom& g, hipStream_t stream) {
  int tiles_h = (g.H + TH - 1) / TH, tiles_w = (g.W + TW - 1) / TW;
  int slices = (g.C + CS - 1) / CS;
  int64_t blocks = (int64_t)g.N * tiles_h * tiles_w * slices;
  if (blocks > 0x7FFFFFFF) return false;
  if (blocks == 0) return true;
  hipLaunchKernelGGL((MaxPoolGradTiled<TH, TW, CS>), dim3((unsigned)blocks),
                     dim3(MaxPoolGradTile<TH, TW, CS>::kThreads), 0, stream,
                     (const __bf16*)x, (const __bf16*)dy, (__bf16*)dx, g,
                     tiles_h, tiles_w, slices);
  return true;
}

// max pool grad: scan window for the argmax, atomically add into f32 scratch.
template <typename T>
__global__ void MaxPoolGradKernel(const T* __restrict__ x,
                                  const T* __restrict__ dy,
                                  float* __restrict__ dx_f32, StfPoolGeom g,
                                  int64_t total_out) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total_out;
       i += stride) {
    int64_t rem = i;
    int c = (int)(rem % g.C); rem /= g.C;
    int q = (int)(rem % g.Q); rem /= g.Q;
    int p = (int)(rem % g.P); rem /= g.P;
    int n = (int)rem;
    float best = -3.4e38f;
    int64_t best_idx = -1;
    for (int kh = 0; kh < g.kh; ++kh) {
      int ih = p * g.sh - g.ph + kh;
      if (ih < 0 || ih >= g.H) continue;
      for (int kw = 0; kw < g.kw; ++kw) {
        int iw = q * g.sw - g.pw + kw;
        if (iw < 0 || iw >= g.W) continue;
        int64_t idx = ((int64_t)(n * g.H + ih) * g.W + iw) * g.C + c;
        float v = (float)x[idx];
        if (v > best) {
          best = v;
          best_idx = idx;
        }
      }
    }
    if (best_idx >= 0) atomicAdd(&dx_f32[best_idx], (float)dy[i]);
  }
}

template <typename T>
__global__ void AvgPoolGradKernel(const T* __restrict__ dy,
                                  T* __restrict__ dx, StfPoolGeom g,
                                  int64_t total_in) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total_in;
       i += stride) {
    int64_t rem = i;
    int c = (int)(rem % g.C); rem /= g.C;
    int iw = (int)(rem % g.W); rem /= g.W;
    int ih = (int)(rem % g.H); rem /= g.H;
    int n = (int)rem;
    float acc = 0.f;
    for (int kh = 0; kh < g.kh; ++kh) {
      int phh = ih + g.ph - kh;
      if (phh < 0 || phh % g.sh) continue;
      int p = phh / g.sh;
      if (p >= g.P) continue;
      for (int kw = 0; kw < g.kw; ++kw) {
        int pww = iw + g.pw - kw;
        if (pww < 0 || pww % g.sw) continue;
        int q = pww / g.sw;
        if (q >= g.Q) continue;
        // count of valid positions for this output window
        int cnt = 0;
        for (int a = 0; a < g.kh; ++a) {
          int t = p * g.sh - g.ph + a;
          if (t < 0 || t >= g.H) continue;
          for (int b = 0; b < g.kw; ++b) {
            int u = q * g.sw - g.pw + b;
            if (u >= 0 && u < g.W) ++cnt;
          }
        }
        acc += (float)dy[((int64_t)(n * g.P + p) * g.Q + q) * g.C + c] / cnt;
      }
    }
    dx[i] = (T)acc;
  }
}

}  // namespace

extern "C" {

hipError_t stf_pool_fwd(int dtype, int is_max, const void* x, void* y,
                        const StfPoolGeom* gp, hipStream_t stream) {
  const StfPoolGeom g = *gp;
  int64_t total = (int64_t)g.N * g.P * g.Q * g.C;
  DispatchBool(is_max, [&](auto m) {
    constexpr bool IS_MAX = decltype(m)::value;
    if (dtype != 0 && g.C % 8 == 0) {
      int64_t total8 = total / 8;
      hipLaunchKernelGGL((PoolFwdKernelV8<IS_MAX>),
                         ElemwiseGrid(total8, 256, 1), dim3(256), 0, stream,
                         (const __bf16*)x, (__bf16*)y, g, total8);
      return;
    }
    DispatchDtype(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      hipLaunchKernelGGL((PoolFwdKernel<T, IS_MAX>),
                         ElemwiseGrid(total, 256, 1), dim3(256), 0, stream,
                         (const T*)x, (T*)y, g, total);
    });
  });
  return hipGetLastError();
}

// One thread per output element, atomics into f32 scratch: the f32 and
// C % 8 != 0 path. (An 8-channel variant of this atomic form measured 2x
// slower: with runtime window loops the per-thread argmax state spills.
// MaxPoolGradTiled's phase 1 is the per-output 8-channel form that does
// not: 3x3 unrolled, the argmax kept as a tap number per channel, no
// scratch.)
hipError_t stf_max_pool_bwd(int dtype, const void* x, const void* dy,
                            float* dx_f32, const StfPoolGeom* gp,
                            hipStream_t stream) {
  const StfPoolGeom g = *gp;
  int64_t total = (int64_t)g.N * g.P * g.Q * g.C;
  DispatchDtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((MaxPoolGradKernel<T>), ElemwiseGrid(total, 256, 1),
                       dim3(256), 0, stream, (const T*)x, (const T*)dy,
                       dx_f32, g, total);
  });
  return hipGetLastError();
}

hipError_t stf_max_pool_bwd_v8(const void* x, const void* dy, void* dx_bf16,
                               const StfPoolGeom* gp, int tiled,
                               hipStream_t stream) {
  const StfPoolGeom g = *gp;
  if (g.C % 8 != 0) return hipErrorInvalidValue;
  if (tiled && g.kh == 3 && g.kw == 3 && g.sh == 2 && g.sw == 2) {
    // 16 x 16 x 32: profiles/resnet50_max_pool_grad.md has the shapes tried
    if (LaunchMaxPoolGradTiled<16, 16, 32>(x, dy, dx_bf16, g, stream))
      return hipGetLastError();
  }
  int64_t total8 = (int64_t)g.N * g.H * g.W * g.C / 8;
  hipLaunchKernelGGL(MaxPoolGradKernelV8, ElemwiseGrid(total8, 256, 1),
                     dim3(256), 0, stream, (const __bf16*)x,
                     (const __bf16*)dy, (__bf16*)dx_bf16, g, total8);
  return hipGetLastError();
}

hipError_t stf_avg_pool_bwd(int dtype, const void* dy, void* dx,
                            const StfPoolGeom* gp, hipStream_t stream) {
  const StfPoolGeom g = *gp;
  int64_t total = (int64_t)g.N * g.H * g.W * g.C;
  if (dtype != 0 && g.C % 8 == 0) {
    int64_t total8 = total / 8;
    hipLaunchKernelGGL(AvgPoolGradKernelV8, ElemwiseGrid(total8, 256, 1),
                       dim3(256), 0, stream, (const __bf16*)dy, (__bf16*)dx,
                       g, total8);
    return hipGetLastError();
  }
  DispatchDtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((AvgPoolGradKernel<T>), ElemwiseGrid(total, 256, 1),
                       dim3(256), 0, stream, (const T*)dy, (T*)dx, g, total);
  });
  return hipGetLastError();
}

}  // extern "C"
