// Optimizer applies on f32 variables: SGD, Momentum (plain / Nesterov), Adam.
// The gradient is f32 or bf16; hyper-parameters are read from device scalars.
// (Replaces reference training_ops_gpu.)
#include "hip_common.h"

namespace {

template <typename G>
__global__ void ApplySgdKernel(float* __restrict__ var,
                               const float* __restrict__ lr,
                               const G* __restrict__ grad, int64_t n) {
  float l = lr[0];
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    var[i] -= l * (float)grad[i];
}

template <typename G>
__global__ void ApplyMomentumKernel(float* __restrict__ var,
                                    float* __restrict__ accum,
                                    const float* __restrict__ lr,
                                    const G* __restrict__ grad,
                                    const float* __restrict__ momentum,
                                    int nesterov, int64_t n) {
  float l = lr[0], mom = momentum[0];
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float g = (float)grad[i];
    float a = accum[i] * mom + g;
    accum[i] = a;
    var[i] -= nesterov ? l * (g + mom * a) : l * a;
  }
}

template <typename G>
__global__ void ApplyAdamKernel(float* __restrict__ var, float* __restrict__ m,
                                float* __restrict__ v,
                                const float* __restrict__ b1p_p,
                                const float* __restrict__ b2p_p,
                                const float* __restrict__ lr_p,
                                const float* __restrict__ b1_p,
                                const float* __restrict__ b2_p,
                                const float* __restrict__ eps_p,
                                const G* __restrict__ grad, int64_t n) {
  float b1p = b1p_p[0], b2p = b2p_p[0], lr = lr_p[0];
  float b1 = b1_p[0], b2 = b2_p[0], eps = eps_p[0];
  float alpha = lr * sqrtf(1.f - b2p) / (1.f - b1p);
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float g = (float)grad[i];
    float mi = m[i] + (g - m[i]) * (1.f - b1);
    float vi = v[i] + (g * g - v[i]) * (1.f - b2);
    m[i] = mi;
    v[i] = vi;
    var[i] -= alpha * mi / (sqrtf(vi) + eps);
  }
}

}  // namespace

extern "C" {

hipError_t stf_apply_sgd(int grad_bf16, void* var, const void* lr,
                         const void* grad, int64_t n, hipStream_t stream) {
  DispatchDtype(grad_bf16, [&](auto t) {
    using G = typename decltype(t)::type;
    hipLaunchKernelGGL((ApplySgdKernel<G>), ElemwiseGrid(n, 256, 4),
                       dim3(256), 0, stream, (float*)var, (const float*)lr,
                       (const G*)grad, n);
  });
  return hipGetLastError();
}

hipError_t stf_apply_momentum(int grad_bf16, void* var, void* accum,
                              const void* lr, const void* grad,
                              const void* momentum, int nesterov, int64_t n,
                              hipStream_t stream) {
  DispatchDtype(grad_bf16, [&](auto t) {
    using G = typename decltype(t)::type;
    hipLaunchKernelGGL((ApplyMomentumKernel<G>), ElemwiseGrid(n, 256, 4),
                       dim3(256), 0, stream, (float*)var, (float*)accum,
                       (const float*)lr, (const G*)grad,
                       (const float*)momentum, nesterov, n);
  });
  return hipGetLastError();
}

hipError_t stf_apply_adam(int grad_bf16, void* var, void* m, void* v,
                          const void* b1p, const void* b2p, const void* lr,
                          const void* b1, const void* b2, const void* eps,
                          const void* grad, int64_t n, hipStream_t stream) {
  DispatchDtype(grad_bf16, [&](auto t) {
    using G = typename decltype(t)::type;
    hipLaunchKernelGGL((ApplyAdamKernel<G>), ElemwiseGrid(n, 256, 4),
                       dim3(256), 0, stream, (float*)var, (float*)m,
                       (float*)v, (const float*)b1p, (const float*)b2p,
                       (const float*)lr, (const float*)b1, (const float*)b2,
                       (const float*)eps, (const G*)grad, n);
  });
  return hipGetLastError();
}

}  // extern "C"
