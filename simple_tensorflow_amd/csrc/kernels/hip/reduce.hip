// Sum / max / min reductions to f32 (full, trailing-axes "row", leading-axes
// "col") and the fused L2Loss. One Reducer, one block reduce and one atomic
// combine serve all of them. (Replaces reference reduction_ops_gpu,
// l2loss_op_gpu — wave64-native designs.)
#include "hip_common.h"

namespace {

template <StfReduce RED>
struct Reducer {
  static constexpr StfReduce kind = RED;
  static __device__ __forceinline__ float init() {
    return StfReduceIdentity(RED);
  }
  static __device__ __forceinline__ float combine(float a, float b) {
    if (RED == STF_REDUCE_SUM) return a + b;
    if (RED == STF_REDUCE_MAX) return fmaxf(a, b);
    return fminf(a, b);
  }
  // max/min only: would v replace old?
  static __device__ __forceinline__ bool improves(float v, float old) {
    return RED == STF_REDUCE_MAX ? v > old : v < old;
  }
};

// Reduces acc over a 256-thread block: wave shuffle, then a 4-slot LDS
// combine. Thread 0 alone gets the block's result, as thread0(result).
template <typename R, typename F>
__device__ __forceinline__ void BlockReduce(float acc, F&& thread0) {
  __shared__ float lds4[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    acc = R::combine(acc, __shfl_down(acc, off, 64));
  int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds4[wid] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = lds4[0];
    for (int w = 1; w < 4; ++w) v = R::combine(v, lds4[w]);
    thread0(v);
  }
}

// *out = combine(*out, v), atomically. Float max/min go through a CAS loop.
template <typename R>
__device__ __forceinline__ void AtomicCombine(float* out, float v) {
  if (R::kind == STF_REDUCE_SUM) {
    atomicAdd(out, v);
    return;
  }
  float old = *out;
  while (R::improves(v, old)) {
    float assumed = old;
    old = __uint_as_float(atomicCAS((unsigned*)out, __float_as_uint(assumed),
                                    __float_as_uint(v)));
    if (old == assumed) break;
  }
}

// 0.5 * sum(x^2) fused in one pass (L2Loss hot path: clip_by_global_norm
// reduces every gradient tensor; the square-temp + reduce pair costs 3
// memory passes, this costs 1).
template <typename T>
__global__ void SquareSumKernel(const T* __restrict__ x,
                                float* __restrict__ out, int64_t n) {
  using R = Reducer<STF_REDUCE_SUM>;
  float acc = 0.f;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float v = (float)x[i];
    acc += v * v;
  }
  BlockReduce<R>(acc, [&](float v) { AtomicCombine<R>(out, 0.5f * v); });
}

// full reduce to scalar: block partials combined atomically into *out, which
// the caller pre-fills with the identity
template <typename T, StfReduce RED>
__global__ void FullReduceKernel(const T* __restrict__ x,
                                 float* __restrict__ out, int64_t n) {
  using R = Reducer<RED>;
  float acc = R::init();
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    acc = R::combine(acc, (float)x[i]);
  BlockReduce<R>(acc, [&](float v) { AtomicCombine<R>(out, v); });
}

// row reduce: [rows, inner] -> [rows]; one block per row
template <typename T, StfReduce RED>
__global__ void RowReduceKernel(const T* __restrict__ x, float* __restrict__ y,
                                int64_t rows, int64_t inner) {
  using R = Reducer<RED>;
  int64_t r = blockIdx.x;
  if (r >= rows) return;
  const T* row = x + r * inner;
  float acc = R::init();
  for (int64_t i = threadIdx.x; i < inner; i += blockDim.x)
    acc = R::combine(acc, (float)row[i]);
  BlockReduce<R>(acc, [&](float v) { y[r] = v; });
}

// outer reduce: [outer, inner] -> [inner] (column sums; e.g. bias-style)
template <typename T, StfReduce RED>
__global__ void ColReduceKernel(const T* __restrict__ x, float* __restrict__ y,
                                int64_t outer, int64_t inner) {
  using R = Reducer<RED>;
  // grid-stride over inner; each thread owns one column strip
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t c = blockIdx.x * blockDim.x + threadIdx.x; c < inner;
       c += stride) {
    float acc = R::init();
    for (int64_t r = 0; r < outer; ++r)
      acc = R::combine(acc, (float)x[r * inner + c]);
    y[c] = acc;
  }
}

// Run-time dtype code and reduce kind -> compile-time arguments, in the
// style of DispatchDtype: f(t, r) gets the element-type tag and a
// std::integral_constant<StfReduce, kind>.
template <typename F>
inline void DispatchReduce(int dtype, StfReduce red, F&& f) {
  DispatchDtype(dtype, [&](auto t) {
    if (red == STF_REDUCE_SUM)
      f(t, std::integral_constant<StfReduce, STF_REDUCE_SUM>{});
    else if (red == STF_REDUCE_MAX)
      f(t, std::integral_constant<StfReduce, STF_REDUCE_MAX>{});
    else
      f(t, std::integral_constant<StfReduce, STF_REDUCE_MIN>{});
  });
}

}  // namespace

extern "C" {

hipError_t stf_l2loss(int dtype, const void* x, float* out_f32, int64_t n,
                      hipStream_t stream) {
  DispatchDtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((SquareSumKernel<T>), ElemwiseGrid(n, 256, 8),
                       dim3(256), 0, stream, (const T*)x, out_f32, n);
  });
  return hipGetLastError();
}

hipError_t stf_full_reduce(int dtype, StfReduce red, const void* x,
                           float* out_f32, int64_t n, hipStream_t stream) {
  DispatchReduce(dtype, red, [&](auto t, auto r) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((FullReduceKernel<T, decltype(r)::value>),
                       ElemwiseGrid(n, 256, 8), dim3(256), 0, stream,
                       (const T*)x, out_f32, n);
  });
  return hipGetLastError();
}

hipError_t stf_row_reduce(int dtype, StfReduce red, const void* x, float* y,
                          int64_t rows, int64_t inner, hipStream_t stream) {
  DispatchReduce(dtype, red, [&](auto t, auto r) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((RowReduceKernel<T, decltype(r)::value>),
                       dim3((uint32_t)rows), dim3(256), 0, stream,
                       (const T*)x, y, rows, inner);
  });
  return hipGetLastError();
}

hipError_t stf_col_reduce(int dtype, StfReduce red, const void* x, float* y,
                          int64_t outer, int64_t inner, hipStream_t stream) {
  DispatchReduce(dtype, red, [&](auto t, auto r) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((ColReduceKernel<T, decltype(r)::value>),
                       ElemwiseGrid(inner, 256, 1), dim3(256), 0, stream,
                       (const T*)x, y, outer, inner);
  });
  return hipGetLastError();
}

}  // extern "C"
