// Philox RNG fills: uniform [0,1), standard normal, truncated normal.
// The philox offset lives in DEVICE memory so a hipGraph replay of the step
// still draws fresh numbers (AdvanceCtrKernel bumps it in-graph after every
// fill). (Replaces reference random_op_gpu.)
#include "hip_common.h"

#include "../philox.h"

namespace {

__global__ void RandomUniformKernel(uint64_t seed,
                                    const unsigned long long* __restrict__ ctr,
                                    float* __restrict__ out, int64_t n,
                                    int as_bf16) {
  uint64_t offset = ctr[0];
  int64_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i * 4 < n; i += stride) {
    stf::random::Philox4x32 rng(seed, offset + i);
    uint32_t r[4];
    rng.Next(r);
    int64_t base = i * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (base + e < n) {
        float v = stf::random::Uint32ToFloat01(r[e]);
        if (as_bf16) ((__bf16*)out)[base + e] = (__bf16)v;
        else out[base + e] = v;
      }
    }
  }
}

__global__ void RandomNormalKernel(uint64_t seed,
                                   const unsigned long long* __restrict__ ctr,
                                   float* __restrict__ out, int64_t n,
                                   int as_bf16, int truncated) {
  uint64_t offset = ctr[0];
  int64_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i * 4 < n; i += stride) {
    stf::random::Philox4x32 rng(seed, offset + i);
    uint32_t r[4];
    float z[4];
    rng.Next(r);
    stf::random::BoxMuller(r[0], r[1], &z[0], &z[1]);
    stf::random::BoxMuller(r[2], r[3], &z[2], &z[3]);
    if (truncated) {
      // redraw per element until |z| < 2 (bounded attempts)
      for (int e = 0; e < 4; ++e) {
        int tries = 0;
        while (fabsf(z[e]) >= 2.f && tries < 16) {
          rng.Next(r);
          float z2;
          stf::random::BoxMuller(r[0], r[1], &z[e], &z2);
          ++tries;
        }
        if (fabsf(z[e]) >= 2.f) z[e] = 0.f;
      }
    }
    int64_t base = i * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (base + e < n) {
        if (as_bf16) ((__bf16*)out)[base + e] = (__bf16)z[e];
        else out[base + e] = z[e];
      }
    }
  }
}

__global__ void AdvanceCtrKernel(unsigned long long* ctr,
                                 unsigned long long delta) {
  if (threadIdx.x == 0 && blockIdx.x == 0) ctr[0] += delta;
}

}  // namespace

extern "C" {

hipError_t stf_random_uniform(uint64_t seed, void* ctr_dev, void* out,
                              int64_t n, int as_bf16, hipStream_t stream) {
  dim3 grid = ElemwiseGrid(n, 256, 4);
  hipLaunchKernelGGL(RandomUniformKernel, grid, dim3(256), 0, stream, seed,
                     (const unsigned long long*)ctr_dev, (float*)out, n,
                     as_bf16);
  hipLaunchKernelGGL(AdvanceCtrKernel, dim3(1), dim3(64), 0, stream,
                     (unsigned long long*)ctr_dev,
                     (unsigned long long)((n + 3) / 4 + 1));
  return hipGetLastError();
}

hipError_t stf_random_normal(uint64_t seed, void* ctr_dev, void* out,
                             int64_t n, int as_bf16, int truncated,
                             hipStream_t stream) {
  dim3 grid = ElemwiseGrid(n, 256, 4);
  hipLaunchKernelGGL(RandomNormalKernel, grid, dim3(256), 0, stream, seed,
                     (const unsigned long long*)ctr_dev, (float*)out, n,
                     as_bf16, truncated);
  hipLaunchKernelGGL(AdvanceCtrKernel, dim3(1), dim3(64), 0, stream,
                     (unsigned long long*)ctr_dev,
                     (unsigned long long)((n + 3) / 4 + 16));
  return hipGetLastError();
}

}  // extern "C"
