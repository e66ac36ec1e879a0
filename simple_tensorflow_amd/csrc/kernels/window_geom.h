// SAME/VALID window geometry of the NHWC conv, depthwise and pool ops, on the
// CPU and the GPU: the one copy of the arithmetic and of the argument checks.
// Plain C++ (no HIP types); gpu_common.h converts to the kernels' ABI structs.
#pragma once

#include <algorithm>
#include <string>
#include <vector>

#include "framework/op_kernel.h"

namespace stf {

// One spatial axis: `in` input pixels, window `k`, step `stride`. *out is the
// output extent, *pad_before the padding in front of the input; of an odd
// total the extra pixel goes after. An empty input gives an empty output
// under either padding; a VALID window larger than a non-empty input is an
// error.
inline Status WindowOutput(const std::string& op, int64_t in, int64_t k,
                           int64_t stride, const std::string& padding,
                           int64_t* out, int64_t* pad_before) {
  if (k < 1 || stride < 1)
    return errors::InvalidArgument(op, ": window ", k, " and stride ", stride,
                                   " must be at least 1");
  if (padding == "SAME") {
    *out = (in + stride - 1) / stride;
    *pad_before = std::max<int64_t>(0, (*out - 1) * stride + k - in) / 2;
  } else if (padding == "VALID") {
    // checked before the division, which truncates a negative span to 0
    if (in > 0 && in < k)
      return errors::InvalidArgument(op, ": window larger than the VALID "
                                     "input (", k, " > ", in, ")");
    *out = in > 0 ? (in - k) / stride + 1 : 0;
    *pad_before = 0;
  } else {
    return errors::InvalidArgument(op, ": padding must be SAME or VALID, "
                                   "got '", padding, "'");
  }
  return Status::OK();
}

// The attributes of a conv or depthwise conv kernel, and its op name for the
// error texts.
struct ConvAttrs {
  explicit ConvAttrs(OpKernelConstruction* c) : op(c->def().op) {
    c->GetAttr("strides", &strides);
    c->GetAttr("padding", &padding);
  }
  std::string op, padding;
  std::vector<int64_t> strides;
};

struct PoolAttrs : ConvAttrs {
  explicit PoolAttrs(OpKernelConstruction* c) : ConvAttrs(c) {
    c->GetAttr("ksize", &ksize);
  }
  std::vector<int64_t> ksize;
};

// NHWC input, [R, S, C, K] filter (depthwise: K is the channel multiplier),
// [N, P, Q, ...] output.
struct ConvGeom {
  int64_t N, H, W, C, R, S, K, sh, sw, ph, pw, P, Q;
  int64_t M() const { return N * P * Q; }
  int64_t RSC() const { return R * S * C; }
  // K-dim padded to the GEMM K-step so glds staging stays 16B-aligned
  // (conv1's RSC=147 would otherwise force the scalar edge path everywhere).
  int64_t RSCp() const { return (RSC() + 63) & ~int64_t(63); }
  bool is_1x1_s1() const {
    return R == 1 && S == 1 && sh == 1 && sw == 1 && ph == 0 && pw == 0;
  }
};

inline Status MakeConvGeom(const TensorShape& x, const TensorShape& filter,
                           const ConvAttrs& a, ConvGeom* g) {
  if (x.dims() != 4 || filter.dims() != 4)
    return errors::InvalidArgument(a.op, ": needs rank-4 input and filter, "
                                   "got ranks ", x.dims(), " and ",
                                   filter.dims());
  if (a.strides.size() != 4 || a.strides[0] != 1 || a.strides[3] != 1)
    return errors::InvalidArgument(a.op, ": strides must be [1, sh, sw, 1]");
  if (filter.dim_size(2) != x.dim_size(3))
    return errors::InvalidArgument(a.op, ": channel mismatch, input has ",
                                   x.dim_size(3), ", filter ",
                                   filter.dim_size(2));
  g->N = x.dim_size(0);
  g->H = x.dim_size(1);
  g->W = x.dim_size(2);
  g->C = x.dim_size(3);
  g->R = filter.dim_size(0);
  g->S = filter.dim_size(1);
  g->K = filter.dim_size(3);
  g->sh = a.strides[1];
  g->sw = a.strides[2];
  STF_RETURN_IF_ERROR(
      WindowOutput(a.op, g->H, g->R, g->sh, a.padding, &g->P, &g->ph));
  return WindowOutput(a.op, g->W, g->S, g->sw, a.padding, &g->Q, &g->pw);
}

// NHWC input, [N, P, Q, C] output.
struct PoolGeom {
  int64_t N, H, W, C, kh, kw, sh, sw, ph, pw, P, Q;
};

inline Status MakePoolGeom(const TensorShape& x, const PoolAttrs& a,
                           PoolGeom* g) {
  if (x.dims() != 4)
    return errors::InvalidArgument(a.op, ": needs rank-4 input, got rank ",
                                   x.dims());
  if (a.ksize.size() != 4 || a.strides.size() != 4)
    return errors::InvalidArgument(a.op, ": ksize and strides must be "
                                   "[1, h, w, 1]");
  g->N = x.dim_size(0);
  g->H = x.dim_size(1);
  g->W = x.dim_size(2);
  g->C = x.dim_size(3);
  g->kh = a.ksize[1];
  g->kw = a.ksize[2];
  g->sh = a.strides[1];
  g->sw = a.strides[2];
  STF_RETURN_IF_ERROR(
      WindowOutput(a.op, g->H, g->kh, g->sh, a.padding, &g->P, &g->ph));
  return WindowOutput(a.op, g->W, g->kw, g->sw, a.padding, &g->Q, &g->pw);
}

}  // namespace stf
