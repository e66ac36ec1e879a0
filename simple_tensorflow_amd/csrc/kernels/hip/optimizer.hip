// Optimizer applies on f32 variables: SGD, Momentum (plain / Nesterov), Adam.
// The gradient is f32 or bf16; hyper-parameters are read from device scalars.
// (Replaces reference training_ops_gpu.)
#include "hip_common.h"
#include "multi_apply_pack.h"

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

// The momentum update of one element. ApplyMomentumKernel and
// MultiApplyMomentum both go through this one function, so the compiler
// contracts (or does not contract) the same expressions in both and their
// results are bit-equal.
__device__ __forceinline__ void MomentumUpdate(float& var, float& accum,
                                               float g, float l, float mom,
                                               int nesterov) {
  float a = accum * mom + g;
  accum = a;
  var -= nesterov ? l * (g + mom * a) : l * a;
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
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    MomentumUpdate(var[i], accum[i], (float)grad[i], l, mom, nesterov);
}

// ---------------------------------------------------------------------------
// Multi-tensor apply: one launch updates many variables. The table of tensors
// and the block -> (tensor, chunk) map travel by value in the kernel
// arguments (multi_apply_pack.h builds them), so nothing on the device has to
// stay valid between launches and a captured graph holds all of it.
// ---------------------------------------------------------------------------
struct MultiApplyArgs {
  float* var[kMultiApplyMaxTensors];
  float* accum[kMultiApplyMaxTensors];
  const void* grad[kMultiApplyMaxTensors];
  int64_t n[kMultiApplyMaxTensors];
  int32_t block_chunk[kMultiApplyMaxBlocks];
  uint8_t block_tensor[kMultiApplyMaxBlocks];
};
static_assert(sizeof(MultiApplyArgs) <= 3200,
              "kernel arguments are limited to 4 KB");

constexpr int kMultiApplyThreads = 512;

// Block b updates one chunk of one tensor. A chunk starts a multiple of
// kMultiApplyChunk elements into its tensor, so it is 16-byte aligned when
// the tensor is; then groups of four elements move as vectors and the ragged
// tail of the tensor's last chunk goes element by element. A tensor whose
// base is not 16-byte aligned goes element by element altogether.
template <typename G>
__global__ __launch_bounds__(kMultiApplyThreads) void MultiApplyMomentum(
    const MultiApplyArgs args, const float* __restrict__ lr,
    const float* __restrict__ momentum, int nesterov) {
  using GVec = __attribute__((ext_vector_type(4))) G;
  const int t = args.block_tensor[blockIdx.x];
  const int64_t start = (int64_t)args.block_chunk[blockIdx.x] * kMultiApplyChunk;
  const int64_t left = args.n[t] - start;
  const int n = (int)(left < kMultiApplyChunk ? left : kMultiApplyChunk);
  float* __restrict__ var = args.var[t] + start;
  float* __restrict__ accum = args.accum[t] + start;
  const G* __restrict__ grad = (const G*)args.grad[t] + start;
  const float l = lr[0], mom = momentum[0];

  const bool aligned =
      (((uintptr_t)var | (uintptr_t)accum | (uintptr_t)grad) & 15) == 0;
  const int nvec = aligned ? n / 4 : 0;
  for (int i = threadIdx.x; i < nvec; i += kMultiApplyThreads) {
    f32x4 v = ((const f32x4*)var)[i];
    f32x4 a = ((const f32x4*)accum)[i];
    GVec g = ((const GVec*)grad)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float vk = v[k], ak = a[k];
      MomentumUpdate(vk, ak, (float)g[k], l, mom, nesterov);
      v[k] = vk;
      a[k] = ak;
    }
    ((f32x4*)accum)[i] = a;
    ((f32x4*)var)[i] = v;
  }
  for (int i = nvec * 4 + threadIdx.x; i < n; i += kMultiApplyThreads)
    MomentumUpdate(var[i], accum[i], (float)grad[i], l, mom, nesterov);
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

hipError_t stf_multi_apply_momentum(int grad_bf16, int count,
                                    void* const* vars, void* const* accums,
                                    const void* const* grads,
                                    const int64_t* sizes, const void* lr,
                                    const void* momentum, int nesterov,
                                    hipStream_t stream) {
  bool ok = PackMultiApply(sizes, count, [&](const MultiApplyPlan& p) {
    MultiApplyArgs args = {};
    for (int s = 0; s < p.num_tensors; ++s) {
      int t = p.tensor_index[s];
      args.var[s] = (float*)vars[t];
      args.accum[s] = (float*)accums[t];
      args.grad[s] = grads[t];
      args.n[s] = sizes[t];
    }
    for (int b = 0; b < p.num_blocks; ++b) {
      args.block_chunk[b] = p.block_chunk[b];
      args.block_tensor[b] = p.block_tensor[b];
    }
    DispatchDtype(grad_bf16, [&](auto t) {
      using G = typename decltype(t)::type;
      hipLaunchKernelGGL((MultiApplyMomentum<G>), dim3(p.num_blocks),
                         dim3(kMultiApplyThreads), 0, stream, args,
                         (const float*)lr, (const float*)momentum, nesterov);
    });
  });
  if (!ok) return hipErrorInvalidValue;
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
