// Embedding lookup and its gradient: row gather, and scatter-add of rows into
// an f32 accumulator (UnsortedSegmentSum). Out-of-range indices read as zero
// rows / are dropped. (Replaces reference gather_functor_gpu,
// segment_reduction_ops_gpu.)
#include "hip_common.h"

namespace {

// embedding gather: out[i, :] = params[indices[i], :]
template <typename T, typename I>
__global__ void GatherRowsKernel(const T* __restrict__ params,
                                 const I* __restrict__ indices,
                                 T* __restrict__ out, int64_t nidx,
                                 int64_t row, int64_t nrows) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t n = nidx * row;
  for (int64_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n;
       idx += stride) {
    int64_t i = idx / row, r = idx % row;
    int64_t src = (int64_t)indices[i];
    out[idx] = (src >= 0 && src < nrows) ? params[src * row + r] : (T)0.f;
  }
}

// embedding grad scatter-add into f32 accumulator (zeroed)
template <typename T, typename I>
__global__ void SegmentSumKernel(const T* __restrict__ data,
                                 const I* __restrict__ ids,
                                 float* __restrict__ out, int64_t nidx,
                                 int64_t row, int64_t nseg) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t n = nidx * row;
  for (int64_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n;
       idx += stride) {
    int64_t i = idx / row, r = idx % row;
    int64_t seg = (int64_t)ids[i];
    if (seg >= 0 && seg < nseg)
      atomicAdd(&out[seg * row + r], (float)data[idx]);
  }
}

}  // namespace

extern "C" {

hipError_t stf_gather_rows(int dtype, int idx_i32, const void* params,
                           const void* indices, void* out, int64_t nidx,
                           int64_t row, int64_t nrows, hipStream_t stream) {
  DispatchDtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    DispatchIndex(idx_i32, [&](auto ix) {
      using I = typename decltype(ix)::type;
      hipLaunchKernelGGL((GatherRowsKernel<T, I>),
                         ElemwiseGrid(nidx * row, 256, 4), dim3(256), 0,
                         stream, (const T*)params, (const I*)indices, (T*)out,
                         nidx, row, nrows);
    });
  });
  return hipGetLastError();
}

hipError_t stf_segment_sum(int dtype, int idx_i32, const void* data,
                           const void* ids, float* out_f32, int64_t nidx,
                           int64_t row, int64_t nseg, hipStream_t stream) {
  DispatchDtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    DispatchIndex(idx_i32, [&](auto ix) {
      using I = typename decltype(ix)::type;
      hipLaunchKernelGGL((SegmentSumKernel<T, I>),
                         ElemwiseGrid(nidx * row, 256, 4), dim3(256), 0,
                         stream, (const T*)data, (const I*)ids, out_f32, nidx,
                         row, nseg);
    });
  });
  return hipGetLastError();
}

}  // extern "C"
