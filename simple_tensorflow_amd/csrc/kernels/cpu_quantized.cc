// Quantized op kernels (capability analogs of reference quantize_op.cc,
// dequantize_op.cc, quantized_matmul_op.cc, quantization_utils.h):
// MIN_COMBINED affine mapping float <-> quint8 (carried as uint8), qint32
// accumulation for the quantized matmul with exact range propagation.
// Requantize, QuantizedBiasAdd, QuantizedMaxPool and QuantizedReshape carry
// a quantize_nodes graph (python/tools/quantize_graph_lib.py) from the conv
// or matmul to the next one. These kernels are the specification that
// kernels/hip/quantized.hip reproduces bit for bit: the per-element formulas
// are defined once, in kernels/quantized_util.h, and called from both; the
// shape checks shared with kernels/gpu_quantized.cc are in
// kernels/quantized_shapes.h.
#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "framework/op_kernel.h"
#include "kernels/kernel_util.h"
#include "kernels/quantized_shapes.h"
#include "kernels/quantized_util.h"
#include "kernels/window_geom.h"

namespace stf {
namespace {

// The scalar range input i.
float RangeIn(OpKernelContext* ctx, int i) {
  return ctx->input(i).flat<float>()[0];
}

// Writes an output range to the scalar outputs i and i + 1.
void RangeOut(OpKernelContext* ctx, int i, float mn, float mx) {
  ctx->allocate_output(i, TensorShape({}))->flat<float>()[0] = mn;
  ctx->allocate_output(i + 1, TensorShape({}))->flat<float>()[0] = mx;
}

// MIN_COMBINED: q = round((x - min) / range * 255); x = min + q * range/255.
class QuantizeV2Op : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    float mn = RangeIn(ctx, 1);
    float mx = RangeIn(ctx, 2);
    if (mx <= mn) mx = mn + 1e-6f;
    Tensor* out = ctx->allocate_output(0, in.shape());
    float scale = 255.f / (mx - mn);
    const float* p = in.flat<float>();
    uint8_t* o = out->flat<uint8_t>();
    for (int64_t i = 0; i < in.NumElements(); ++i)
      o[i] = QuantizeU8(p[i], mn, scale);
    RangeOut(ctx, 1, mn, mx);
  }
};
REGISTER_KERNEL_BUILDER(Name("QuantizeV2").Device(DEVICE_CPU), QuantizeV2Op);

class DequantizeOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    float mn = RangeIn(ctx, 1);
    float mx = RangeIn(ctx, 2);
    Tensor* out = ctx->allocate_output(0, in.shape());
    float* o = out->flat<float>();
    if (in.dtype() == DT_UINT8) {
      float step = QuantStep(mn, mx);
      const uint8_t* p = in.flat<uint8_t>();
      for (int64_t i = 0; i < in.NumElements(); ++i)
        o[i] = DequantizeU8(p[i], mn, step);
    } else {  // qint32 carrier: min/max map the full int32 range
      const int32_t* p = in.flat<int32_t>();
      double scale = QuantUnitI32(mn, mx);
      for (int64_t i = 0; i < in.NumElements(); ++i)
        o[i] = DequantizeI32(p[i], scale, mn);
    }
  }
};
REGISTER_KERNEL_BUILDER(Name("Dequantize").Device(DEVICE_CPU), DequantizeOp);

// out_int32 = sum (a_q - a_zero) * (b_q - b_zero) in float-equivalent units:
// we accumulate raw products and propagate the float range exactly as the
// reference does (min/max of the int32 result in float units).
class QuantizedMatMulOp : public OpKernel {
 public:
  explicit QuantizedMatMulOp(OpKernelConstruction* c) : OpKernel(c) {
    c->GetAttr("transpose_a", &ta_);
    c->GetAttr("transpose_b", &tb_);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& a = ctx->input(0);
    const Tensor& b = ctx->input(1);
    float min_a = RangeIn(ctx, 2);
    float max_a = RangeIn(ctx, 3);
    float min_b = RangeIn(ctx, 4);
    float max_b = RangeIn(ctx, 5);
    int64_t M, N, K;
    OP_REQUIRES_OK(ctx,
                   QuantMatMulDims(a.shape(), b.shape(), ta_, tb_, &M, &N, &K));
    Tensor* out = ctx->allocate_output(0, TensorShape({M, N}));
    const uint8_t* ap = a.flat<uint8_t>();
    const uint8_t* bp = b.flat<uint8_t>();
    int32_t* op = out->flat<int32_t>();
    // zero points for MIN_COMBINED quint8
    float sa = QuantStep(min_a, max_a);
    float sb = QuantStep(min_b, max_b);
    int32_t za = QuantZeroPoint(min_a, max_a);
    int32_t zb = QuantZeroPoint(min_b, max_b);
    for (int64_t m = 0; m < M; ++m)
      for (int64_t n = 0; n < N; ++n) {
        int64_t acc = 0;
        for (int64_t k = 0; k < K; ++k) {
          int32_t av = ta_ ? ap[k * M + m] : ap[m * K + k];
          int32_t bv = tb_ ? bp[n * K + k] : bp[k * N + n];
          acc += (int64_t)(av - za) * (bv - zb);
        }
        op[m * N + n] = (int32_t)acc;
      }
    // float value of one output unit = sa * sb; int32 range maps to:
    RangeOut(ctx, 1, QuantProductMin(sa, sb), QuantProductMax(sa, sb));
  }

 private:
  bool ta_ = false, tb_ = false;
};
REGISTER_KERNEL_BUILDER(Name("QuantizedMatMul").Device(DEVICE_CPU),
                        QuantizedMatMulOp);

// out[n,p,q,k] = sum over the taps inside the image of
// (x - z_in) * (w - z_f), NHWC input, [R,S,C,K] filter, reduced to int32
// modulo 2^32 (reference quantized_conv_ops.cc analog). Zero points and the
// output range follow QuantizedMatMul.
class QuantizedConv2DOp : public OpKernel {
 public:
  explicit QuantizedConv2DOp(OpKernelConstruction* c)
      : OpKernel(c), attrs_(c) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    const Tensor& w = ctx->input(1);
    ConvGeom g;
    OP_REQUIRES_OK(ctx, MakeConvGeom(x.shape(), w.shape(), attrs_, &g));
    float min_x = RangeIn(ctx, 2);
    float max_x = RangeIn(ctx, 3);
    float min_w = RangeIn(ctx, 4);
    float max_w = RangeIn(ctx, 5);
    Tensor* out = ctx->allocate_output(0, TensorShape({g.N, g.P, g.Q, g.K}));
    const uint8_t* xp = x.flat<uint8_t>();
    const uint8_t* wp = w.flat<uint8_t>();
    int32_t* op = out->flat<int32_t>();
    float sx = QuantStep(min_x, max_x);
    float sf = QuantStep(min_w, max_w);
    int32_t zx = QuantZeroPoint(min_x, max_x);
    int32_t zf = QuantZeroPoint(min_w, max_w);
    std::vector<int64_t> acc(g.K);
    for (int64_t n = 0; n < g.N; ++n)
      for (int64_t p = 0; p < g.P; ++p)
        for (int64_t q = 0; q < g.Q; ++q) {
          std::fill(acc.begin(), acc.end(), 0);
          for (int64_t r = 0; r < g.R; ++r) {
            int64_t h = p * g.sh - g.ph + r;
            if (h < 0 || h >= g.H) continue;
            for (int64_t s = 0; s < g.S; ++s) {
              int64_t wi = q * g.sw - g.pw + s;
              if (wi < 0 || wi >= g.W) continue;
              const uint8_t* xr = xp + ((n * g.H + h) * g.W + wi) * g.C;
              const uint8_t* wr = wp + (r * g.S + s) * g.C * g.K;
              for (int64_t c = 0; c < g.C; ++c) {
                int64_t xv = (int32_t)xr[c] - zx;
                for (int64_t k = 0; k < g.K; ++k)
                  acc[k] += xv * ((int32_t)wr[c * g.K + k] - zf);
              }
            }
          }
          int32_t* o = op + ((n * g.P + p) * g.Q + q) * g.K;
          for (int64_t k = 0; k < g.K; ++k) o[k] = (int32_t)acc[k];
        }
    RangeOut(ctx, 1, QuantProductMin(sx, sf), QuantProductMax(sx, sf));
  }

 private:
  ConvAttrs attrs_;
};
REGISTER_KERNEL_BUILDER(Name("QuantizedConv2D").Device(DEVICE_CPU),
                        QuantizedConv2DOp);

class QuantizedReluOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    float mn = RangeIn(ctx, 1);
    float mx = RangeIn(ctx, 2);
    Tensor* out = ctx->allocate_output(0, in.shape());
    // the quantized value representing 0.0
    int32_t zero_q = QuantZeroPoint(mn, mx);
    const uint8_t* p = in.flat<uint8_t>();
    uint8_t* o = out->flat<uint8_t>();
    for (int64_t i = 0; i < in.NumElements(); ++i)
      o[i] = (uint8_t)std::max<int32_t>(p[i], std::max(0, zero_q));
    RangeOut(ctx, 1, mn, mx);
  }
};
REGISTER_KERNEL_BUILDER(Name("QuantizedRelu").Device(DEVICE_CPU),
                        QuantizedReluOp);

class RequantizationRangeOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    float mn = RangeIn(ctx, 1);
    float mx = RangeIn(ctx, 2);
    double unit = QuantUnitI32(mn, mx);
    const int32_t* p = in.flat<int32_t>();
    int32_t lo = 0, hi = 0;
    for (int64_t i = 0; i < in.NumElements(); ++i) {
      lo = std::min(lo, p[i]);
      hi = std::max(hi, p[i]);
    }
    RangeOut(ctx, 0, (float)(lo * unit), (float)(hi * unit));
  }
};
REGISTER_KERNEL_BUILDER(Name("RequantizationRange").Device(DEVICE_CPU),
                        RequantizationRangeOp);

class QuantizeDownAndShrinkRangeOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    float mn = RangeIn(ctx, 1);
    float mx = RangeIn(ctx, 2);
    double unit = QuantUnitI32(mn, mx);
    const int32_t* p = in.flat<int32_t>();
    int64_t n = in.NumElements();
    double lo = 0, hi = 0;
    for (int64_t i = 0; i < n; ++i) {
      double v = p[i] * unit;
      lo = std::min(lo, v);
      hi = std::max(hi, v);
    }
    if (hi <= lo) hi = lo + 1e-6;
    Tensor* out = ctx->allocate_output(0, in.shape());
    uint8_t* o = out->flat<uint8_t>();
    double scale = 255.0 / (hi - lo);
    for (int64_t i = 0; i < n; ++i)
      o[i] = QuantizeDownI32(p[i], unit, lo, scale);
    RangeOut(ctx, 1, (float)lo, (float)hi);
  }
};
REGISTER_KERNEL_BUILDER(Name("QuantizeDownAndShrinkRange").Device(DEVICE_CPU),
                        QuantizeDownAndShrinkRangeOp);

// QuantizeDownAndShrinkRange's second loop with a range that is given
// instead of measured: one pass, no reduction.
class RequantizeOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    float mn = RangeIn(ctx, 1);
    float mx = RangeIn(ctx, 2);
    double unit = QuantUnitI32(mn, mx);
    double lo = (double)RangeIn(ctx, 3);
    double hi = (double)RangeIn(ctx, 4);
    if (hi <= lo) hi = lo + 1e-6;
    const int32_t* p = in.flat<int32_t>();
    int64_t n = in.NumElements();
    Tensor* out = ctx->allocate_output(0, in.shape());
    uint8_t* o = out->flat<uint8_t>();
    double scale = 255.0 / (hi - lo);
    for (int64_t i = 0; i < n; ++i)
      o[i] = QuantizeDownI32(p[i], unit, lo, scale);
    RangeOut(ctx, 1, (float)lo, (float)hi);
  }
};
REGISTER_KERNEL_BUILDER(Name("Requantize").Device(DEVICE_CPU), RequantizeOp);

// out = round((fx + fb) / unit) with fx, fb the f32 values Dequantize gives
// and unit the qint32 unit of the output range. That range is +-2^17 times
// the largest absolute input range value (the reference's headroom rule), so
// |quotient| stays near 2^15 and nothing clamps.
class QuantizedBiasAddOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    const Tensor& bias = ctx->input(1);
    int64_t rows, C;
    OP_REQUIRES_OK(ctx, QuantBiasAddDims(in.shape(), bias.shape(), &rows, &C));
    QuantBiasAddScale sc = MakeQuantBiasAddScale(
        RangeIn(ctx, 2), RangeIn(ctx, 3), RangeIn(ctx, 4), RangeIn(ctx, 5));
    Tensor* out = ctx->allocate_output(0, in.shape());
    const uint8_t* x = in.flat<uint8_t>();
    const uint8_t* b = bias.flat<uint8_t>();
    int32_t* o = out->flat<int32_t>();
    for (int64_t i = 0; i < rows * C; ++i)
      o[i] = QuantBiasAddI32(x[i], b[i % C], sc);
    RangeOut(ctx, 1, -sc.max_out, sc.max_out);
  }
};
REGISTER_KERNEL_BUILDER(Name("QuantizedBiasAdd").Device(DEVICE_CPU),
                        QuantizedBiasAddOp);

// Attributes of the two NHWC quint8 pools. Both pass their ranges through.
class QuantizedPoolOp : public OpKernel {
 public:
  explicit QuantizedPoolOp(OpKernelConstruction* c)
      : OpKernel(c), attrs_(c) {}

 protected:
  void ForwardRanges(OpKernelContext* ctx) const {
    RangeOut(ctx, 1, RangeIn(ctx, 1), RangeIn(ctx, 2));
  }
  PoolAttrs attrs_;
};

// NHWC max over the taps inside the image. The mapping is monotone, so the
// ranges pass through.
class QuantizedMaxPoolOp : public QuantizedPoolOp {
 public:
  using QuantizedPoolOp::QuantizedPoolOp;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    PoolGeom g;
    OP_REQUIRES_OK(ctx, MakePoolGeom(in.shape(), attrs_, &g));
    Tensor* out = ctx->allocate_output(0, TensorShape({g.N, g.P, g.Q, g.C}));
    const uint8_t* x = in.flat<uint8_t>();
    uint8_t* y = out->flat<uint8_t>();
    for (int64_t n = 0; n < g.N; ++n)
      for (int64_t p = 0; p < g.P; ++p)
        for (int64_t q = 0; q < g.Q; ++q) {
          uint8_t* o = y + ((n * g.P + p) * g.Q + q) * g.C;
          std::fill(o, o + g.C, (uint8_t)0);
          for (int64_t r = 0; r < g.kh; ++r) {
            int64_t ih = p * g.sh - g.ph + r;
            if (ih < 0 || ih >= g.H) continue;
            for (int64_t s = 0; s < g.kw; ++s) {
              int64_t iw = q * g.sw - g.pw + s;
              if (iw < 0 || iw >= g.W) continue;
              const uint8_t* xr = x + ((n * g.H + ih) * g.W + iw) * g.C;
              for (int64_t c = 0; c < g.C; ++c)
                o[c] = std::max(o[c], xr[c]);
            }
          }
        }
    ForwardRanges(ctx);
  }
};
REGISTER_KERNEL_BUILDER(Name("QuantizedMaxPool").Device(DEVICE_CPU),
                        QuantizedMaxPoolOp);

// NHWC integer mean over the taps inside the image (the reference's
// SpatialAvgPool<int32>): the divisor is the in-image tap count, not kh*kw,
// and the division truncates. The mean of values in [mn, mx] lies in
// [mn, mx], so the ranges pass through.
class QuantizedAvgPoolOp : public QuantizedPoolOp {
 public:
  using QuantizedPoolOp::QuantizedPoolOp;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    PoolGeom g;
    OP_REQUIRES_OK(ctx, MakePoolGeom(in.shape(), attrs_, &g));
    Tensor* out = ctx->allocate_output(0, TensorShape({g.N, g.P, g.Q, g.C}));
    const uint8_t* x = in.flat<uint8_t>();
    uint8_t* y = out->flat<uint8_t>();
    std::vector<int32_t> acc(g.C);
    for (int64_t n = 0; n < g.N; ++n)
      for (int64_t p = 0; p < g.P; ++p)
        for (int64_t q = 0; q < g.Q; ++q) {
          std::fill(acc.begin(), acc.end(), 0);
          int32_t taps = 0;
          for (int64_t r = 0; r < g.kh; ++r) {
            int64_t ih = p * g.sh - g.ph + r;
            if (ih < 0 || ih >= g.H) continue;
            for (int64_t s = 0; s < g.kw; ++s) {
              int64_t iw = q * g.sw - g.pw + s;
              if (iw < 0 || iw >= g.W) continue;
              const uint8_t* xr = x + ((n * g.H + ih) * g.W + iw) * g.C;
              for (int64_t c = 0; c < g.C; ++c) acc[c] += xr[c];
              ++taps;
            }
          }
          uint8_t* o = y + ((n * g.P + p) * g.Q + q) * g.C;
          // a window always holds a tap inside the image; 0 guards the rest
          for (int64_t c = 0; c < g.C; ++c)
            o[c] = taps ? (uint8_t)(acc[c] / taps) : 0;
        }
    ForwardRanges(ctx);
  }
};
REGISTER_KERNEL_BUILDER(Name("QuantizedAvgPool").Device(DEVICE_CPU),
                        QuantizedAvgPoolOp);

// out = min(max(x, lo), hi) with lo the clamped zero point and hi the quint8
// of 6.0 (kernels/quantized_util.h). QuantizedRelu wraps a zero point above
// 255 into the byte; Relu6 clamps it instead. The order is max, then min:
// where hi < lo the result is hi.
class QuantizedRelu6Op : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    float mn = RangeIn(ctx, 1);
    float mx = RangeIn(ctx, 2);
    Tensor* out = ctx->allocate_output(0, in.shape());
    int32_t lo = QuantRelu6Floor(mn, mx);
    int32_t hi = QuantRelu6Ceil(mn, mx);
    const uint8_t* p = in.flat<uint8_t>();
    uint8_t* o = out->flat<uint8_t>();
    for (int64_t i = 0; i < in.NumElements(); ++i)
      o[i] = (uint8_t)std::min(std::max<int32_t>(p[i], lo), hi);
    RangeOut(ctx, 1, mn, mx);
  }
};
REGISTER_KERNEL_BUILDER(Name("QuantizedRelu6").Device(DEVICE_CPU),
                        QuantizedRelu6Op);

// Concatenation of N quint8 tensors that each carry a range of their own
// (reference quantized_concat_op.cc analog). The output range is
// [min(0, min_i mn_i), max_i mx_i]. An input whose range equals it, under
// f32 == on both ends, is copied byte for byte; every other input goes
// through RequantizeU8. The copy rule is part of the specification: for the
// degenerate range (0, 0) requantizing maps every byte to 0.
class QuantizedConcatOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    QuantConcatPlan plan;
    OP_REQUIRES_OK(ctx, MakeQuantConcatPlan(ctx, num_inputs(), &plan));
    Tensor* out = ctx->allocate_output(0, plan.out_shape);
    float lo = 0, hi = 0;
    for (int k = 0; k < plan.n; ++k)
      QuantConcatRangeFold(RangeIn(ctx, plan.min(k)),
                           RangeIn(ctx, plan.max(k)), k == 0, &lo, &hi);
    uint8_t* dst = out->flat<uint8_t>();
    for (int k = 0; k < plan.n; ++k) {
      float mn = RangeIn(ctx, plan.min(k));
      float mx = RangeIn(ctx, plan.max(k));
      int64_t row = plan.row[k];
      const uint8_t* src = ctx->input(plan.value(k)).flat<uint8_t>();
      uint8_t lut[256];
      bool copy = mn == lo && mx == hi;
      for (int v = 0; v < 256; ++v)
        lut[v] = copy ? (uint8_t)v : RequantizeU8(v, mn, mx, lo, hi);
      for (int64_t o = 0; o < plan.outer; ++o) {
        const uint8_t* s = src + o * row;
        uint8_t* d = dst + o * plan.out_row + plan.off[k];
        for (int64_t j = 0; j < row; ++j) d[j] = lut[s[j]];
      }
    }
    RangeOut(ctx, 1, lo, hi);
  }
};
REGISTER_KERNEL_BUILDER(Name("QuantizedConcat").Device(DEVICE_CPU),
                        QuantizedConcatOp);

// Reshape with the two range scalars forwarded. Like ReshapeOp it shares
// the buffers and touches no tensor data, so one class serves both devices.
class QuantizedReshapeOp : public OpKernel {
 public:
  explicit QuantizedReshapeOp(OpKernelConstruction* c) : OpKernel(c) {
    set_expensive(false);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    auto dims = IntVector(ctx->input(1));
    int64_t known = 1;
    int infer = -1;
    for (size_t i = 0; i < dims.size(); ++i) {
      if (dims[i] == -1) {
        OP_REQUIRES(ctx, infer < 0,
                    errors::InvalidArgument("multiple -1 dims in "
                                            "QuantizedReshape"));
        infer = (int)i;
      } else {
        known *= dims[i];
      }
    }
    if (infer >= 0) dims[infer] = known ? in.NumElements() / known : 0;
    TensorShape shape(dims);
    OP_REQUIRES(ctx, shape.num_elements() == in.NumElements(),
                errors::InvalidArgument("QuantizedReshape size mismatch: "
                                        "input ", in.shape().DebugString(),
                                        " to ", shape.DebugString()));
    ctx->set_output(0, in.Reshaped(shape));
    ctx->set_output(1, ctx->input(2));
    ctx->set_output(2, ctx->input(3));
  }
};
REGISTER_KERNEL_BUILDER(Name("QuantizedReshape").Device(DEVICE_CPU),
                        QuantizedReshapeOp);
REGISTER_KERNEL_BUILDER(
    Name("QuantizedReshape").Device(DEVICE_GPU).HostMemory("shape"),
    QuantizedReshapeOp);

}  // namespace
}  // namespace stf
