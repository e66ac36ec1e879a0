// Depthwise conv NHWC (reference core/kernels/depthwise_conv_op_gpu.cu.cc
// fwd :40 / bwd-input :270 / bwd-filter :437) — direct per-output kernels,
// channel-vectorized where C%8==0 is not required (grid-stride, 16B loads
// opportunistic via contiguous channel runs).
#include "hip_common.h"
#include "stf_kernels.h"

namespace {

struct DwGeom {
  int N, H, W, C, R, S, sh, sw, ph, pw, P, Q, mult;
};

__global__ void DwFwdKernel(const __bf16* __restrict__ x,
                            const __bf16* __restrict__ w,
                            __bf16* __restrict__ y, DwGeom g, int64_t total) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int CM = g.C * g.mult;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    int64_t rem = i;
    int cm = (int)(rem % CM); rem /= CM;
    int q = (int)(rem % g.Q); rem /= g.Q;
    int p = (int)(rem % g.P); rem /= g.P;
    int n = (int)rem;
    int c = cm / g.mult, m = cm % g.mult;
    float acc = 0.f;
    for (int r = 0; r < g.R; ++r) {
      int ih = p * g.sh - g.ph + r;
      if (ih < 0 || ih >= g.H) continue;
      for (int s = 0; s < g.S; ++s) {
        int iw = q * g.sw - g.pw + s;
        if (iw < 0 || iw >= g.W) continue;
        acc += (float)x[((int64_t)(n * g.H + ih) * g.W + iw) * g.C + c] *
               (float)w[((r * g.S + s) * g.C + c) * g.mult + m];
      }
    }
    y[i] = (__bf16)acc;
  }
}

__global__ void DwBwdInputKernel(const __bf16* __restrict__ dy,
                                 const __bf16* __restrict__ w,
                                 __bf16* __restrict__ dx, DwGeom g,
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
    for (int r = 0; r < g.R; ++r) {
      int ph = ih + g.ph - r;
      if (ph < 0 || ph % g.sh) continue;
      int p = ph / g.sh;
      if (p >= g.P) continue;
      for (int s = 0; s < g.S; ++s) {
        int pw = iw + g.pw - s;
        if (pw < 0 || pw % g.sw) continue;
        int q = pw / g.sw;
        if (q >= g.Q) continue;
        for (int m = 0; m < g.mult; ++m) {
          acc += (float)dy[((int64_t)(n * g.P + p) * g.Q + q) *
                               (g.C * g.mult) + c * g.mult + m] *
                 (float)w[((r * g.S + s) * g.C + c) * g.mult + m];
        }
      }
    }
    dx[i] = (__bf16)acc;
  }
}

// dW via f32 atomics (zeroed scratch): one thread per output position.
__global__ void DwBwdFilterKernel(const __bf16* __restrict__ x,
                                  const __bf16* __restrict__ dy,
                                  float* __restrict__ dw_f32, DwGeom g,
                                  int64_t total_out) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int CM = g.C * g.mult;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total_out;
       i += stride) {
    int64_t rem = i;
    int cm = (int)(rem % CM); rem /= CM;
    int q = (int)(rem % g.Q); rem /= g.Q;
    int p = (int)(rem % g.P); rem /= g.P;
    int n = (int)rem;
    int c = cm / g.mult, m = cm % g.mult;
    float gy = (float)dy[i];
    for (int r = 0; r < g.R; ++r) {
      int ih = p * g.sh - g.ph + r;
      if (ih < 0 || ih >= g.H) continue;
      for (int s = 0; s < g.S; ++s) {
        int iw = q * g.sw - g.pw + s;
        if (iw < 0 || iw >= g.W) continue;
        float xv = (float)x[((int64_t)(n * g.H + ih) * g.W + iw) * g.C + c];
        atomicAdd(&dw_f32[((r * g.S + s) * g.C + c) * g.mult + m], gy * xv);
      }
    }
  }
}

DwGeom MakeDwGeom(const StfConvGeom& g, int mult) {
  return DwGeom{g.n,  g.h,  g.w,  g.c, g.r, g.s, g.sh,
                g.sw, g.ph, g.pw, g.p, g.q, mult};
}

}  // namespace

extern "C" hipError_t stf_depthwise_fwd(const void* x, const void* w, void* y,
                                        const StfConvGeom* cg, int mult,
                                        hipStream_t stream) {
  DwGeom g = MakeDwGeom(*cg, mult);
  int64_t total = (int64_t)g.N * g.P * g.Q * g.C * mult;
  hipLaunchKernelGGL(DwFwdKernel, ElemwiseGrid(total, 256, 1), dim3(256), 0,
                     stream, (const __bf16*)x, (const __bf16*)w, (__bf16*)y,
                     g, total);
  return hipGetLastError();
}

extern "C" hipError_t stf_depthwise_bwd_input(const void* dy, const void* w,
                                              void* dx, const StfConvGeom* cg,
                                              int mult, hipStream_t stream) {
  DwGeom g = MakeDwGeom(*cg, mult);
  int64_t total = (int64_t)g.N * g.H * g.W * g.C;
  hipLaunchKernelGGL(DwBwdInputKernel, ElemwiseGrid(total, 256, 1), dim3(256),
                     0, stream, (const __bf16*)dy, (const __bf16*)w,
                     (__bf16*)dx, g, total);
  return hipGetLastError();
}

extern "C" hipError_t stf_depthwise_bwd_filter(const void* x, const void* dy,
                                               float* dw_f32,
                                               const StfConvGeom* cg, int mult,
                                               hipStream_t stream) {
  DwGeom g = MakeDwGeom(*cg, mult);
  int64_t total = (int64_t)g.N * g.P * g.Q * g.C * mult;
  hipLaunchKernelGGL(DwBwdFilterKernel, ElemwiseGrid(total, 256, 1),
                     dim3(256), 0, stream, (const __bf16*)x,
                     (const __bf16*)dy, dw_f32, g, total);
  return hipGetLastError();
}
