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

// One thread per output element. (An 8-channel variant of this per-output
// form measured 2x slower: the per-thread argmax state spills.)
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
                               const StfPoolGeom* gp, hipStream_t stream) {
  const StfPoolGeom g = *gp;
  if (g.C % 8 != 0) return hipErrorInvalidValue;
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
