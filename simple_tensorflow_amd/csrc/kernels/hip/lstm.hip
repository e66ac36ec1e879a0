// Fused LSTM cell pointwise kernels, forward and backward; f32 math.
#include "hip_common.h"
#include "stf_kernels.h"

namespace {

// One pass over the post-GEMM gate matrix (layout [B, 4H] in BasicLSTMCell
// split order i, j, f, o) + c_prev -> all cell outputs and every activation
// the backward pass needs. Replaces the ~17-kernel elementwise chain the
// composed cell launches per timestep (reference capability analog:
// contrib/rnn lstm_ops.cc LSTMBlockCell fused CUDA kernel).
__device__ __forceinline__ float stf_sigmoid(float x) {
  return 1.f / (1.f + __expf(-x));
}

template <typename T>
__global__ void LstmGatesKernel(const T* __restrict__ gates,
                                const T* __restrict__ c_prev,
                                float forget_bias, T* __restrict__ i_out,
                                T* __restrict__ f_out, T* __restrict__ o_out,
                                T* __restrict__ ci_out, T* __restrict__ cs_out,
                                T* __restrict__ co_out, T* __restrict__ h_out,
                                int64_t total, int H) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += stride) {
    int64_t b = idx / H;
    int hcol = (int)(idx - b * H);
    const T* g = gates + b * 4 * H;
    float i = stf_sigmoid((float)g[hcol]);
    float ci = tanhf((float)g[H + hcol]);
    float f = stf_sigmoid((float)g[2 * H + hcol] + forget_bias);
    float o = stf_sigmoid((float)g[3 * H + hcol]);
    float cs = f * (float)c_prev[idx] + i * ci;
    float co = tanhf(cs);
    i_out[idx] = (T)i;
    f_out[idx] = (T)f;
    o_out[idx] = (T)o;
    ci_out[idx] = (T)ci;
    cs_out[idx] = (T)cs;
    co_out[idx] = (T)co;
    h_out[idx] = (T)(o * co);
  }
}

// Backward of the pointwise cell: dh + dc(next) + saved activations ->
// packed dgates [B, 4H] (feeds the dW / dx GEMMs directly, no 4-way concat)
// and dc_prev.
template <typename T>
__global__ void LstmGatesGradKernel(
    const T* __restrict__ c_prev, const T* __restrict__ i_,
    const T* __restrict__ f_, const T* __restrict__ o_,
    const T* __restrict__ ci_, const T* __restrict__ co_,
    const T* __restrict__ dh, const T* __restrict__ dcs_next,
    T* __restrict__ dgates, T* __restrict__ dc_prev, int64_t total, int H) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += stride) {
    int64_t b = idx / H;
    int hcol = (int)(idx - b * H);
    float i = (float)i_[idx], f = (float)f_[idx], o = (float)o_[idx];
    float ci = (float)ci_[idx], co = (float)co_[idx];
    float dhv = (float)dh[idx];
    float dcs = dhv * o * (1.f - co * co) + (float)dcs_next[idx];
    T* dg = dgates + b * 4 * H;
    dg[hcol] = (T)(dcs * ci * i * (1.f - i));
    dg[H + hcol] = (T)(dcs * i * (1.f - ci * ci));
    dg[2 * H + hcol] = (T)(dcs * (float)c_prev[idx] * f * (1.f - f));
    dg[3 * H + hcol] = (T)(dhv * co * o * (1.f - o));
    dc_prev[idx] = (T)(dcs * f);
  }
}

}  // namespace

extern "C" {

hipError_t stf_lstm_gates(int dtype, const void* gates, const void* c_prev,
                          float forget_bias, void* i_out, void* f_out,
                          void* o_out, void* ci_out, void* cs_out,
                          void* co_out, void* h_out, int64_t batch, int H,
                          hipStream_t stream) {
  int64_t total = batch * H;
  dim3 grid = ElemwiseGrid(total, 256, 1);
  DispatchDtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((LstmGatesKernel<T>), grid, dim3(256), 0, stream,
                       (const T*)gates, (const T*)c_prev, forget_bias,
                       (T*)i_out, (T*)f_out, (T*)o_out, (T*)ci_out,
                       (T*)cs_out, (T*)co_out, (T*)h_out, total, H);
  });
  return hipGetLastError();
}

hipError_t stf_lstm_gates_grad(int dtype, const void* c_prev, const void* i_,
                               const void* f_, const void* o_, const void* ci_,
                               const void* co_, const void* dh,
                               const void* dcs_next, void* dgates,
                               void* dc_prev, int64_t batch, int H,
                               hipStream_t stream) {
  int64_t total = batch * H;
  dim3 grid = ElemwiseGrid(total, 256, 1);
  DispatchDtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((LstmGatesGradKernel<T>), grid, dim3(256), 0, stream,
                       (const T*)c_prev, (const T*)i_, (const T*)f_,
                       (const T*)o_, (const T*)ci_, (const T*)co_,
                       (const T*)dh, (const T*)dcs_next, (T*)dgates,
                       (T*)dc_prev, total, H);
  });
  return hipGetLastError();
}

}  // extern "C"
