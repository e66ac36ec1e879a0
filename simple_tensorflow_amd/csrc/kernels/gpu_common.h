// Shared by the GPU OpKernel files (kernels/gpu_*.cc): thin wrappers that
// resolve shapes/attrs and enqueue the hand-written CDNA4 HIP kernels
// (kernels/hip/*.hip) on the device's compute stream. These REPLACE library
// paths (no rocBLAS/MIOpen): MatMul/Conv2D run on the in-tree MFMA GEMM.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <functional>

#include "kernels/hip/stf_kernels.h"
#include "kernels/kernel_util.h"
#include "kernels/window_geom.h"

#define GPU_STREAM(ctx) ((hipStream_t)(ctx)->device()->compute_stream())
#define OP_HIP_OK(ctx, expr)                                              \
  {                                                                       \
    hipError_t _e = (expr);                                               \
    if (_e != hipSuccess) {                                               \
      (ctx)->SetStatus(errors::Internal("HIP kernel failure: ",           \
                                        hipGetErrorString(_e)));          \
      return;                                                             \
    }                                                                     \
  }

namespace stf {

inline int DtypeCode(DataType dt) { return dt == DT_FLOAT ? 0 : 1; }

inline int CastCode(DataType dt) {
  switch (dt) {
    case DT_FLOAT: return 0;
    case DT_BFLOAT16: return 1;
    case DT_HALF: return 2;
    case DT_INT32: return 3;
    case DT_INT64: return 4;
    case DT_BOOL: return 5;
    default: return -1;
  }
}

// matches UOp / BOp order in elementwise.hip
enum {
  U_NEG, U_ABS, U_SIGN, U_SQUARE, U_SQRT, U_RSQRT, U_EXP, U_LOG, U_LOG1P,
  U_TANH, U_SIGMOID, U_RELU, U_RELU6, U_SOFTPLUS, U_RECIP, U_FLOOR, U_CEIL,
  U_SIN, U_COS
};
enum {
  B_ADD, B_SUB, B_MUL, B_DIV, B_MAX, B_MIN, B_POW, B_SQDIFF, B_SIGMOID_GRAD,
  B_TANH_GRAD, B_RSQRT_GRAD, B_SQRT_GRAD, B_RELU_GRAD, B_RELU6_GRAD,
  B_SOFTPLUS_GRAD
};

// Window geometry (kernels/window_geom.h) as the HIP entry points take it:
// InvalidArgument, not truncation, where a field does not fit in int.
inline Status FitInt(const std::string& op,
                     std::initializer_list<int64_t> values) {
  for (int64_t v : values)
    if (v > INT_MAX)
      return errors::InvalidArgument(op, ": dimension ", v,
                                     " does not fit the GPU kernels' int");
  return Status::OK();
}
inline Status ToAbi(const std::string& op, const ConvGeom& g,
                    StfConvGeom* out) {
  STF_RETURN_IF_ERROR(FitInt(op, {g.N, g.H, g.W, g.C, g.R, g.S, g.sh, g.sw,
                                  g.ph, g.pw, g.P, g.Q}));
  *out = StfConvGeom{(int)g.N,  (int)g.H,  (int)g.W,  (int)g.C,
                     (int)g.R,  (int)g.S,  (int)g.sh, (int)g.sw,
                     (int)g.ph, (int)g.pw, (int)g.P,  (int)g.Q, g.K};
  return Status::OK();
}
inline Status ToAbi(const std::string& op, const PoolGeom& g,
                    StfPoolGeom* out) {
  STF_RETURN_IF_ERROR(FitInt(op, {g.N, g.H, g.W, g.C, g.kh, g.kw, g.sh, g.sw,
                                  g.ph, g.pw, g.P, g.Q}));
  *out = StfPoolGeom{(int)g.N,  (int)g.H,  (int)g.W,  (int)g.C,
                     (int)g.kh, (int)g.kw, (int)g.sh, (int)g.sw,
                     (int)g.ph, (int)g.pw, (int)g.P,  (int)g.Q};
  return Status::OK();
}
// A conv's geometry both ways; the pool ops need nothing but the ABI struct.
inline Status MakeConvGeom(const TensorShape& x, const TensorShape& filter,
                           const ConvAttrs& a, ConvGeom* g, StfConvGeom* sg) {
  STF_RETURN_IF_ERROR(MakeConvGeom(x, filter, a, g));
  return ToAbi(a.op, *g, sg);
}
inline Status MakePoolGeom(const TensorShape& x, const PoolAttrs& a,
                           StfPoolGeom* out) {
  PoolGeom g;
  STF_RETURN_IF_ERROR(MakePoolGeom(x, a, &g));
  return ToAbi(a.op, g, out);
}

// zero an f32 device buffer on the stream
inline hipError_t ZeroF32(void* p, int64_t n, hipStream_t s) {
  return hipMemsetAsync(p, 0, n * 4, s);
}

// The helpers below own process-wide state (one arena map, one zero page)
// and are therefore defined once, in gpu_common.cc.

// Choose a split-K factor so the grid covers the 256 CUs; 1 = no split.
int PickSplitK(int64_t M, int64_t N, int64_t K);

// Persistent pre-zeroed f32 split-K accumulator (per GPU); nullptr when
// `elems` is too large or allocation fails.
float* SplitKArena(int ordinal, int64_t elems, hipStream_t s);

// 256 zeroed device bytes for the implicit-GEMM address generators'
// out-of-bounds (padding) loads; nullptr if allocation failed.
const void* ZeroPage();

// Runs a split-K accumulation of `elems` f32 values and casts the result to
// `out_bf16`: `launch(acc)` must atomically accumulate into the zeroed f32
// buffer `acc`. Uses the arena (drained by the cast-and-rezero kernel) when
// it fits, else a zeroed temp and a plain cast.
hipError_t SplitKInto(OpKernelContext* ctx, int64_t elems,
                      const std::function<hipError_t(float*)>& launch,
                      void* out_bf16);

// GEMM helper: picks plain vs split-K (f32 accumulate + cast) automatically.
// a_km/b_km: the operand is stored contraction-major ([K,M]/[K,N], row
// stride lda/ldb) and transposed in-kernel during LDS staging.
hipError_t GemmBf16AutoEx(OpKernelContext* ctx, const void* A, const void* B,
                          void* C_bf16, int64_t M, int64_t N, int64_t K,
                          int64_t lda, int64_t ldb, int a_km, int b_km,
                          hipStream_t s);

}  // namespace stf
