// Bias add/grad, softmax and fused softmax cross-entropy (sparse and dense
// labels); f32 math. (Replaces reference bias_op_gpu.cu.cc, softmax_op_gpu,
// xent_op_gpu — redesigned for wave64 + LDS per the CDNA4 guide, not
// translated.)
#include "hip_common.h"
#include "stf_kernels.h"

namespace {

__device__ __forceinline__ float WaveReduceSum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ float WaveReduceMax(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_down(v, off, 64));
  return v;
}

// Block-level (256 threads) reduce; result valid in thread 0.
__device__ float BlockReduceSum(float v, float* lds4) {
  v = WaveReduceSum(v);
  int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds4[wid] = v;
  __syncthreads();
  if (threadIdx.x == 0) v = lds4[0] + lds4[1] + lds4[2] + lds4[3];
  return v;
}
__device__ float BlockReduceMax(float v, float* lds4) {
  v = WaveReduceMax(v);
  int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds4[wid] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    v = fmaxf(fmaxf(lds4[0], lds4[1]), fmaxf(lds4[2], lds4[3]));
  return v;
}

// ---------------- bias ----------------
template <typename T>
__global__ void BiasAddKernel(const T* __restrict__ x,
                              const T* __restrict__ bias, T* __restrict__ y,
                              int64_t n, int c) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    y[i] = (T)((float)x[i] + (float)bias[i % c]);
}

// Column sum of dy[rows, c] into db[c] (pre-zeroed f32). 2D grid: x covers
// columns (thread = one column, coalesced reads), y chunks the rows so the
// grid reaches a few hundred blocks even for skinny row counts (an LSTM
// timestep has rows = batch = 20); each thread accumulates its chunk in a
// register and lands ONE atomicAdd.
template <typename T>
__global__ void BiasGradKernel(const T* __restrict__ dy, float* __restrict__ db,
                               int64_t rows, int c, int rows_per_block) {
  int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= c) return;
  int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  int64_t r1 = min(r0 + (int64_t)rows_per_block, rows);
  float acc = 0.f;
  const T* p = dy + r0 * c + col;
  for (int64_t r = r0; r < r1; ++r, p += c) acc += (float)*p;
  if (gridDim.y == 1)
    db[col] = acc;  // contract: db was zeroed; single chunk can store
  else
    atomicAdd(&db[col], acc);
}

// ---------------- softmax / xent ----------------
// one block per row
template <typename T, bool LOG>
__global__ void SoftmaxKernel(const T* __restrict__ x, T* __restrict__ y,
                              int cols) {
  __shared__ float lds4[4];
  __shared__ float stat[2];  // max, sum
  const T* row = x + (int64_t)blockIdx.x * cols;
  T* out = y + (int64_t)blockIdx.x * cols;
  float mx = -3.4e38f;
  for (int i = threadIdx.x; i < cols; i += blockDim.x)
    mx = fmaxf(mx, (float)row[i]);
  mx = BlockReduceMax(mx, lds4);
  if (threadIdx.x == 0) stat[0] = mx;
  __syncthreads();
  mx = stat[0];
  float sum = 0.f;
  for (int i = threadIdx.x; i < cols; i += blockDim.x)
    sum += __expf((float)row[i] - mx);
  __syncthreads();
  sum = BlockReduceSum(sum, lds4);
  if (threadIdx.x == 0) stat[1] = sum;
  __syncthreads();
  sum = stat[1];
  if (LOG) {
    float lsum = __logf(sum);
    for (int i = threadIdx.x; i < cols; i += blockDim.x)
      out[i] = (T)((float)row[i] - mx - lsum);
  } else {
    float inv = 1.f / sum;
    for (int i = threadIdx.x; i < cols; i += blockDim.x)
      out[i] = (T)(__expf((float)row[i] - mx) * inv);
  }
}

// fused sparse softmax xent: loss[row], backprop[row, cols]
template <typename T, typename L>
__global__ void SparseXentKernel(const T* __restrict__ logits,
                                 const L* __restrict__ labels,
                                 float* __restrict__ loss,
                                 T* __restrict__ backprop, int cols) {
  __shared__ float lds4[4];
  __shared__ float stat[2];
  int64_t r = blockIdx.x;
  const T* row = logits + r * cols;
  T* bp = backprop + r * cols;
  float mx = -3.4e38f;
  for (int i = threadIdx.x; i < cols; i += blockDim.x)
    mx = fmaxf(mx, (float)row[i]);
  mx = BlockReduceMax(mx, lds4);
  if (threadIdx.x == 0) stat[0] = mx;
  __syncthreads();
  mx = stat[0];
  float sum = 0.f;
  for (int i = threadIdx.x; i < cols; i += blockDim.x)
    sum += __expf((float)row[i] - mx);
  __syncthreads();
  sum = BlockReduceSum(sum, lds4);
  if (threadIdx.x == 0) stat[1] = sum;
  __syncthreads();
  sum = stat[1];
  float lsum = __logf(sum);
  L lbl = labels[r];
  if (lbl < 0 || lbl >= (L)cols) {
    // a label outside [0, cols) has no class to score: NaN loss and a NaN
    // backprop row, as the reference's GPU path gives
    float nan = __builtin_nanf("");
    for (int i = threadIdx.x; i < cols; i += blockDim.x) bp[i] = (T)nan;
    if (threadIdx.x == 0 && loss) loss[r] = nan;
    return;
  }
  for (int i = threadIdx.x; i < cols; i += blockDim.x) {
    float logp = (float)row[i] - mx - lsum;
    bp[i] = (T)(__expf(logp) - (i == lbl ? 1.f : 0.f));
    if (i == lbl && loss) loss[r] = -logp;
  }
}

// dense-label fused xent
template <typename T>
__global__ void XentKernel(const T* __restrict__ logits,
                           const T* __restrict__ labels,
                           float* __restrict__ loss, T* __restrict__ backprop,
                           int cols) {
  __shared__ float lds4[4];
  __shared__ float stat[2];
  int64_t r = blockIdx.x;
  const T* row = logits + r * cols;
  const T* lab = labels + r * cols;
  T* bp = backprop + r * cols;
  float mx = -3.4e38f;
  for (int i = threadIdx.x; i < cols; i += blockDim.x)
    mx = fmaxf(mx, (float)row[i]);
  mx = BlockReduceMax(mx, lds4);
  if (threadIdx.x == 0) stat[0] = mx;
  __syncthreads();
  mx = stat[0];
  float sum = 0.f;
  for (int i = threadIdx.x; i < cols; i += blockDim.x)
    sum += __expf((float)row[i] - mx);
  __syncthreads();
  sum = BlockReduceSum(sum, lds4);
  if (threadIdx.x == 0) stat[1] = sum;
  __syncthreads();
  sum = stat[1];
  float lsum = __logf(sum);
  float lsum_part = 0.f;
  for (int i = threadIdx.x; i < cols; i += blockDim.x) {
    float logp = (float)row[i] - mx - lsum;
    float l = (float)lab[i];
    bp[i] = (T)(__expf(logp) - l);
    lsum_part -= l * logp;
  }
  __syncthreads();
  lsum_part = BlockReduceSum(lsum_part, lds4);
  if (threadIdx.x == 0) loss[r] = lsum_part;
}

}  // namespace

extern "C" {

hipError_t stf_bias_add(int dtype, const void* x, const void* bias, void* y,
                        int64_t n, int c, hipStream_t stream) {
  dim3 grid = ElemwiseGrid(n, 256, 4);
  DispatchDtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((BiasAddKernel<T>), grid, dim3(256), 0, stream,
                       (const T*)x, (const T*)bias, (T*)y, n, c);
  });
  return hipGetLastError();
}

// db_f32 must be zeroed
hipError_t stf_bias_grad(int dtype, const void* dy, void* db_f32, int64_t rows,
                         int c, hipStream_t stream) {
  if (rows <= 0 || c <= 0) return hipSuccess;  // db stays at its zeros
  uint32_t colb = (uint32_t)((c + 255) / 256);
  // enough row chunks to put ~512 blocks on the 256 CUs, but at least 4 rows
  // per chunk so the atomic traffic stays bounded
  int64_t yb = 512 / (colb ? colb : 1);
  int64_t max_yb = (rows + 3) / 4;
  if (yb > max_yb) yb = max_yb;
  if (yb < 1) yb = 1;
  int rpb = (int)((rows + yb - 1) / yb);
  yb = (rows + rpb - 1) / rpb;
  dim3 grid(colb, (uint32_t)yb);
  DispatchDtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((BiasGradKernel<T>), grid, dim3(256), 0, stream,
                       (const T*)dy, (float*)db_f32, rows, c, rpb);
  });
  return hipGetLastError();
}

hipError_t stf_softmax(int dtype, int log_sm, const void* x, void* y,
                       int64_t rows, int cols, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;  // empty input: nothing to launch
  DispatchDtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    DispatchBool(log_sm, [&](auto log) {
      hipLaunchKernelGGL((SoftmaxKernel<T, decltype(log)::value>),
                         dim3((uint32_t)rows), dim3(256), 0, stream,
                         (const T*)x, (T*)y, cols);
    });
  });
  return hipGetLastError();
}

hipError_t stf_sparse_xent(int dtype, const void* logits, const void* labels,
                           int labels_i32, void* loss_f32, void* backprop,
                           int64_t rows, int cols, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  DispatchDtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    DispatchBool(labels_i32, [&](auto i32) {
      using L = std::conditional_t<decltype(i32)::value, int32_t, int64_t>;
      hipLaunchKernelGGL((SparseXentKernel<T, L>), dim3((uint32_t)rows),
                         dim3(256), 0, stream, (const T*)logits,
                         (const L*)labels, (float*)loss_f32, (T*)backprop,
                         cols);
    });
  });
  return hipGetLastError();
}

hipError_t stf_xent(int dtype, const void* logits, const void* labels,
                    void* loss_f32, void* backprop, int64_t rows, int cols,
                    hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  DispatchDtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((XentKernel<T>), dim3((uint32_t)rows), dim3(256), 0,
                       stream, (const T*)logits, (const T*)labels,
                       (float*)loss_f32, (T*)backprop, cols);
  });
  return hipGetLastError();
}

}  // extern "C"
