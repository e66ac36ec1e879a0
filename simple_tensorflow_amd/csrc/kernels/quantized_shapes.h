// Shape checks and layout of the quantized ops whose CPU and GPU kernels
// (kernels/cpu_quantized.cc, kernels/gpu_quantized.cc) must agree on them:
// the one copy of each check and of QuantizedConcat's layout. Plain C++ (no
// HIP types).
#pragma once

#include <vector>

#include "framework/op_kernel.h"
#include "kernels/kernel_util.h"

namespace stf {

// a [M, K] x b [K, N] after the transposes.
inline Status QuantMatMulDims(const TensorShape& a, const TensorShape& b,
                              bool transpose_a, bool transpose_b, int64_t* M,
                              int64_t* N, int64_t* K) {
  if (a.dims() != 2 || b.dims() != 2)
    return errors::InvalidArgument("QuantizedMatMul needs matrices");
  *M = transpose_a ? a.dim_size(1) : a.dim_size(0);
  *K = transpose_a ? a.dim_size(0) : a.dim_size(1);
  *N = transpose_b ? b.dim_size(0) : b.dim_size(1);
  if (*K != (transpose_b ? b.dim_size(1) : b.dim_size(0)))
    return errors::InvalidArgument("QuantizedMatMul inner dim mismatch");
  return Status::OK();
}

// The input viewed as [rows, C] with C the bias length.
inline Status QuantBiasAddDims(const TensorShape& in, const TensorShape& bias,
                               int64_t* rows, int64_t* C) {
  if (in.dims() < 1 || bias.dims() != 1 ||
      in.dim_size(in.dims() - 1) != bias.dim_size(0))
    return errors::InvalidArgument("QuantizedBiasAdd: the last input "
                                   "dimension must equal the bias length");
  *C = bias.dim_size(0);
  *rows = *C ? in.num_elements() / *C : 0;
  return Status::OK();
}

// QuantizedConcat of n inputs, each viewed as [outer, row[k]] bytes; input k
// lands at byte off[k] of every out_row-byte output row. The op's inputs are
// concat_dim, the n tensors, their n minima, their n maxima.
struct QuantConcatPlan {
  int n = 0;
  TensorShape out_shape;
  int64_t outer = 1, out_row = 0;
  std::vector<int64_t> row, off;
  int value(int k) const { return 1 + k; }
  int min(int k) const { return 1 + n + k; }
  int max(int k) const { return 1 + 2 * n + k; }
};

inline Status MakeQuantConcatPlan(OpKernelContext* ctx, int num_inputs,
                                  QuantConcatPlan* p) {
  p->n = (num_inputs - 1) / 3;
  const Tensor& first = ctx->input(p->value(0));
  int rank = first.dims();
  int64_t axis = IntVector(ctx->input(0))[0];
  if (axis < -rank || axis >= rank)
    return errors::InvalidArgument("QuantizedConcat: concat_dim ", axis,
                                   " out of range for rank ", rank);
  if (axis < 0) axis += rank;
  int64_t inner = 1;
  for (int i = 0; i < axis; ++i) p->outer *= first.dim_size(i);
  for (int i = (int)axis + 1; i < rank; ++i) inner *= first.dim_size(i);
  int64_t axis_total = 0;
  for (int k = 0; k < p->n; ++k) {
    const Tensor& t = ctx->input(p->value(k));
    if (t.dims() != rank)
      return errors::InvalidArgument("QuantizedConcat: input ", k,
                                     " has rank ", t.dims(),
                                     ", input 0 has rank ", rank);
    for (int d = 0; d < rank; ++d)
      if (d != axis && t.dim_size(d) != first.dim_size(d))
        return errors::InvalidArgument(
            "QuantizedConcat: input ", k, " has shape ",
            t.shape().DebugString(), ", input 0 has shape ",
            first.shape().DebugString(),
            "; they may differ on the concat axis only");
    p->row.push_back(t.dim_size((int)axis) * inner);
    p->off.push_back(axis_total * inner);
    axis_total += t.dim_size((int)axis);
  }
  p->out_shape = first.shape();
  p->out_shape.set_dim((int)axis, axis_total);
  p->out_row = axis_total * inner;
  return Status::OK();
}

}  // namespace stf
