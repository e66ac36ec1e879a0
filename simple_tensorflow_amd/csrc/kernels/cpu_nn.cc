// CPU NN kernels: Conv2D (NHWC direct loops), pooling, batch norm.
// These are the fp32 reference implementations the HIP kernels are validated
// against (SURVEY.md §4 test strategy); CPU speed is not a goal.
#include <cmath>

#include "kernels/kernel_util.h"
#include "kernels/window_geom.h"

namespace stf {

template <typename T>
class Conv2DOp : public OpKernel {
 public:
  explicit Conv2DOp(OpKernelConstruction* ctx) : OpKernel(ctx), attrs_(ctx) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    const Tensor& filter = ctx->input(1);
    ConvGeom p;
    OP_REQUIRES_OK(ctx, MakeConvGeom(in.shape(), filter.shape(), attrs_, &p));
    Tensor* out = ctx->allocate_output(0, TensorShape({p.N, p.P, p.Q, p.K}));
    const T* x = in.flat<T>();
    const T* w = filter.flat<T>();
    T* y = out->flat<T>();
    std::memset(y, 0, out->TotalBytes());
    for (int64_t n = 0; n < p.N; ++n)
      for (int64_t oh = 0; oh < p.P; ++oh)
        for (int64_t ow = 0; ow < p.Q; ++ow) {
          T* yrow = y + ((n * p.P + oh) * p.Q + ow) * p.K;
          for (int64_t r = 0; r < p.R; ++r) {
            int64_t ih = oh * p.sh - p.ph + r;
            if (ih < 0 || ih >= p.H) continue;
            for (int64_t s = 0; s < p.S; ++s) {
              int64_t iw = ow * p.sw - p.pw + s;
              if (iw < 0 || iw >= p.W) continue;
              const T* xrow = x + ((n * p.H + ih) * p.W + iw) * p.C;
              const T* wrow = w + (r * p.S + s) * p.C * p.K;
              for (int64_t c = 0; c < p.C; ++c) {
                T xv = xrow[c];
                const T* wk = wrow + c * p.K;
                for (int64_t k = 0; k < p.K; ++k) yrow[k] += xv * wk[k];
              }
            }
          }
        }
  }

 private:
  ConvAttrs attrs_;
};
REGISTER_CPU_KERNEL_FLOATS("Conv2D", Conv2DOp)

template <typename T>
class Conv2DBackpropInputOp : public OpKernel {
 public:
  explicit Conv2DBackpropInputOp(OpKernelConstruction* ctx, bool side = false)
      : OpKernel(ctx), attrs_(ctx), side_(side) {}
  void Compute(OpKernelContext* ctx) override {
    auto in_sizes = IntVector(ctx->input(0));
    const Tensor& filter = ctx->input(1);
    const Tensor& dy = ctx->input(2);
    TensorShape in_shape(in_sizes);
    ConvGeom p;
    OP_REQUIRES_OK(ctx, MakeConvGeom(in_shape, filter.shape(), attrs_, &p));
    Tensor* out = ctx->allocate_output(0, in_shape);
    const T* w = filter.flat<T>();
    const T* g = dy.flat<T>();
    T* dx = out->flat<T>();
    if (side_) {
      // Conv2DBackpropInputAdd: accumulate on top of the side gradient
      // instead of zero (the add the gradient aggregator would have run).
      const Tensor& sd = ctx->input(3);
      OP_REQUIRES(ctx, sd.NumElements() == out->NumElements(),
                  errors::InvalidArgument(
                      "Conv2DBackpropInputAdd: side shape mismatch"));
      std::memcpy(dx, sd.flat<T>(), out->TotalBytes());
    } else {
      std::memset(dx, 0, out->TotalBytes());
    }
    for (int64_t n = 0; n < p.N; ++n)
      for (int64_t oh = 0; oh < p.P; ++oh)
        for (int64_t ow = 0; ow < p.Q; ++ow) {
          const T* grow = g + ((n * p.P + oh) * p.Q + ow) * p.K;
          for (int64_t r = 0; r < p.R; ++r) {
            int64_t ih = oh * p.sh - p.ph + r;
            if (ih < 0 || ih >= p.H) continue;
            for (int64_t s = 0; s < p.S; ++s) {
              int64_t iw = ow * p.sw - p.pw + s;
              if (iw < 0 || iw >= p.W) continue;
              T* xrow = dx + ((n * p.H + ih) * p.W + iw) * p.C;
              const T* wrow = w + (r * p.S + s) * p.C * p.K;
              for (int64_t c = 0; c < p.C; ++c) {
                const T* wk = wrow + c * p.K;
                T acc = 0;
                for (int64_t k = 0; k < p.K; ++k) acc += grow[k] * wk[k];
                xrow[c] += acc;
              }
            }
          }
        }
  }

 private:
  ConvAttrs attrs_;
  bool side_;
};
REGISTER_CPU_KERNEL_FLOATS("Conv2DBackpropInput", Conv2DBackpropInputOp)

template <typename T>
class Conv2DBackpropInputAddOp : public Conv2DBackpropInputOp<T> {
 public:
  explicit Conv2DBackpropInputAddOp(OpKernelConstruction* ctx)
      : Conv2DBackpropInputOp<T>(ctx, true) {}
};
REGISTER_CPU_KERNEL_FLOATS("Conv2DBackpropInputAdd", Conv2DBackpropInputAddOp)

template <typename T>
class Conv2DBackpropFilterOp : public OpKernel {
 public:
  explicit Conv2DBackpropFilterOp(OpKernelConstruction* ctx)
      : OpKernel(ctx), attrs_(ctx) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    auto f_sizes = IntVector(ctx->input(1));
    const Tensor& dy = ctx->input(2);
    TensorShape f_shape(f_sizes);
    ConvGeom p;
    OP_REQUIRES_OK(ctx, MakeConvGeom(in.shape(), f_shape, attrs_, &p));
    Tensor* out = ctx->allocate_output(0, f_shape);
    const T* x = in.flat<T>();
    const T* g = dy.flat<T>();
    T* dw = out->flat<T>();
    std::memset(dw, 0, out->TotalBytes());
    for (int64_t n = 0; n < p.N; ++n)
      for (int64_t oh = 0; oh < p.P; ++oh)
        for (int64_t ow = 0; ow < p.Q; ++ow) {
          const T* grow = g + ((n * p.P + oh) * p.Q + ow) * p.K;
          for (int64_t r = 0; r < p.R; ++r) {
            int64_t ih = oh * p.sh - p.ph + r;
            if (ih < 0 || ih >= p.H) continue;
            for (int64_t s = 0; s < p.S; ++s) {
              int64_t iw = ow * p.sw - p.pw + s;
              if (iw < 0 || iw >= p.W) continue;
              const T* xrow = x + ((n * p.H + ih) * p.W + iw) * p.C;
              T* wrow = dw + (r * p.S + s) * p.C * p.K;
              for (int64_t c = 0; c < p.C; ++c) {
                T xv = xrow[c];
                T* wk = wrow + c * p.K;
                for (int64_t k = 0; k < p.K; ++k) wk[k] += xv * grow[k];
              }
            }
          }
        }
  }

 private:
  ConvAttrs attrs_;
};
REGISTER_CPU_KERNEL_FLOATS("Conv2DBackpropFilter", Conv2DBackpropFilterOp)

// --------------------------------- pooling ---------------------------------
template <typename T, bool is_max>
class PoolOp : public OpKernel {
 public:
  explicit PoolOp(OpKernelConstruction* ctx) : OpKernel(ctx), attrs_(ctx) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    PoolGeom p;
    OP_REQUIRES_OK(ctx, MakePoolGeom(in.shape(), attrs_, &p));
    Tensor* out = ctx->allocate_output(0, TensorShape({p.N, p.P, p.Q, p.C}));
    const T* x = in.flat<T>();
    T* y = out->flat<T>();
    for (int64_t n = 0; n < p.N; ++n)
      for (int64_t oh = 0; oh < p.P; ++oh)
        for (int64_t ow = 0; ow < p.Q; ++ow)
          for (int64_t c = 0; c < p.C; ++c) {
            T best = is_max ? std::numeric_limits<T>::lowest() : T(0);
            int64_t count = 0;
            for (int64_t kh = 0; kh < p.kh; ++kh) {
              int64_t ih = oh * p.sh - p.ph + kh;
              if (ih < 0 || ih >= p.H) continue;
              for (int64_t kw = 0; kw < p.kw; ++kw) {
                int64_t iw = ow * p.sw - p.pw + kw;
                if (iw < 0 || iw >= p.W) continue;
                T v = x[((n * p.H + ih) * p.W + iw) * p.C + c];
                if (is_max) best = v > best ? v : best;
                else best += v;
                ++count;
              }
            }
            y[((n * p.P + oh) * p.Q + ow) * p.C + c] =
                is_max ? best : best / (T)count;
          }
  }

 private:
  PoolAttrs attrs_;
};
REGISTER_KERNEL_BUILDER(Name("MaxPool").Device(DEVICE_CPU).TypeConstraint<float>("T"), PoolOp<float, true>);
REGISTER_KERNEL_BUILDER(Name("MaxPool").Device(DEVICE_CPU).TypeConstraint<double>("T"), PoolOp<double, true>);
REGISTER_KERNEL_BUILDER(Name("AvgPool").Device(DEVICE_CPU).TypeConstraint<float>("T"), PoolOp<float, false>);
REGISTER_KERNEL_BUILDER(Name("AvgPool").Device(DEVICE_CPU).TypeConstraint<double>("T"), PoolOp<double, false>);

template <typename T>
class MaxPoolGradOp : public OpKernel {
 public:
  explicit MaxPoolGradOp(OpKernelConstruction* ctx)
      : OpKernel(ctx), attrs_(ctx) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    const Tensor& dy = ctx->input(2);
    PoolGeom p;
    OP_REQUIRES_OK(ctx, MakePoolGeom(in.shape(), attrs_, &p));
    Tensor* out = ctx->allocate_output(0, in.shape());
    const T* x = in.flat<T>();
    const T* g = dy.flat<T>();
    T* dx = out->flat<T>();
    std::memset(dx, 0, out->TotalBytes());
    for (int64_t n = 0; n < p.N; ++n)
      for (int64_t oh = 0; oh < p.P; ++oh)
        for (int64_t ow = 0; ow < p.Q; ++ow)
          for (int64_t c = 0; c < p.C; ++c) {
            // find argmax
            T best = std::numeric_limits<T>::lowest();
            int64_t bi = -1;
            for (int64_t kh = 0; kh < p.kh; ++kh) {
              int64_t ih = oh * p.sh - p.ph + kh;
              if (ih < 0 || ih >= p.H) continue;
              for (int64_t kw = 0; kw < p.kw; ++kw) {
                int64_t iw = ow * p.sw - p.pw + kw;
                if (iw < 0 || iw >= p.W) continue;
                int64_t idx = ((n * p.H + ih) * p.W + iw) * p.C + c;
                if (x[idx] > best) {
                  best = x[idx];
                  bi = idx;
                }
              }
            }
            if (bi >= 0) dx[bi] += g[((n * p.P + oh) * p.Q + ow) * p.C + c];
          }
  }

 private:
  PoolAttrs attrs_;
};
REGISTER_KERNEL_BUILDER(Name("MaxPoolGrad").Device(DEVICE_CPU).TypeConstraint<float>("T"), MaxPoolGradOp<float>);
REGISTER_KERNEL_BUILDER(Name("MaxPoolGrad").Device(DEVICE_CPU).TypeConstraint<double>("T"), MaxPoolGradOp<double>);

template <typename T>
class AvgPoolGradOp : public OpKernel {
 public:
  explicit AvgPoolGradOp(OpKernelConstruction* ctx)
      : OpKernel(ctx), attrs_(ctx) {}
  void Compute(OpKernelContext* ctx) override {
    auto in_sizes = IntVector(ctx->input(0));
    const Tensor& dy = ctx->input(1);
    TensorShape in_shape(in_sizes);
    PoolGeom p;
    OP_REQUIRES_OK(ctx, MakePoolGeom(in_shape, attrs_, &p));
    Tensor* out = ctx->allocate_output(0, in_shape);
    const T* g = dy.flat<T>();
    T* dx = out->flat<T>();
    std::memset(dx, 0, out->TotalBytes());
    for (int64_t n = 0; n < p.N; ++n)
      for (int64_t oh = 0; oh < p.P; ++oh)
        for (int64_t ow = 0; ow < p.Q; ++ow) {
          // count valid positions
          int64_t count = 0;
          for (int64_t kh = 0; kh < p.kh; ++kh) {
            int64_t ih = oh * p.sh - p.ph + kh;
            if (ih < 0 || ih >= p.H) continue;
            for (int64_t kw = 0; kw < p.kw; ++kw) {
              int64_t iw = ow * p.sw - p.pw + kw;
              if (iw >= 0 && iw < p.W) ++count;
            }
          }
          for (int64_t c = 0; c < p.C; ++c) {
            T gv = g[((n * p.P + oh) * p.Q + ow) * p.C + c] / (T)count;
            for (int64_t kh = 0; kh < p.kh; ++kh) {
              int64_t ih = oh * p.sh - p.ph + kh;
              if (ih < 0 || ih >= p.H) continue;
              for (int64_t kw = 0; kw < p.kw; ++kw) {
                int64_t iw = ow * p.sw - p.pw + kw;
                if (iw < 0 || iw >= p.W) continue;
                dx[((n * p.H + ih) * p.W + iw) * p.C + c] += gv;
              }
            }
          }
        }
  }

 private:
  PoolAttrs attrs_;
};
REGISTER_KERNEL_BUILDER(Name("AvgPoolGrad").Device(DEVICE_CPU).TypeConstraint<float>("T").HostMemory("orig_input_shape"), AvgPoolGradOp<float>);
REGISTER_KERNEL_BUILDER(Name("AvgPoolGrad").Device(DEVICE_CPU).TypeConstraint<double>("T").HostMemory("orig_input_shape"), AvgPoolGradOp<double>);

// ------------------------------ FusedBatchNorm -------------------------------
class FusedBatchNormOp : public OpKernel {
 public:
  explicit FusedBatchNormOp(OpKernelConstruction* ctx) : OpKernel(ctx) {
    ctx->GetAttr("epsilon", &eps_);
    ctx->GetAttr("is_training", &training_);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    const Tensor& scale = ctx->input(1);
    const Tensor& offset = ctx->input(2);
    int64_t C = x.dim_size(3);
    int64_t rows = x.NumElements() / C;
    Tensor* y = ctx->allocate_output(0, x.shape());
    Tensor* mean_out = ctx->allocate_output(1, TensorShape({C}));
    Tensor* var_out = ctx->allocate_output(2, TensorShape({C}));
    Tensor* save_mean = ctx->allocate_output(3, TensorShape({C}));
    Tensor* save_inv = ctx->allocate_output(4, TensorShape({C}));
    const float* xp = x.flat<float>();
    float* yp = y->flat<float>();
    std::vector<double> mean(C, 0), var(C, 0);
    if (training_) {
      for (int64_t i = 0; i < rows; ++i)
        for (int64_t c = 0; c < C; ++c) mean[c] += xp[i * C + c];
      for (int64_t c = 0; c < C; ++c) mean[c] /= rows;
      for (int64_t i = 0; i < rows; ++i)
        for (int64_t c = 0; c < C; ++c) {
          double d = xp[i * C + c] - mean[c];
          var[c] += d * d;
        }
      for (int64_t c = 0; c < C; ++c) var[c] /= rows;
    } else {
      const float* m = ctx->input(3).flat<float>();
      const float* v = ctx->input(4).flat<float>();
      for (int64_t c = 0; c < C; ++c) {
        mean[c] = m[c];
        var[c] = v[c];
      }
    }
    const float* sc = scale.flat<float>();
    const float* of = offset.flat<float>();
    std::vector<float> inv(C);
    for (int64_t c = 0; c < C; ++c) {
      inv[c] = 1.0f / std::sqrt((float)var[c] + eps_);
      mean_out->flat<float>()[c] = (float)mean[c];
      var_out->flat<float>()[c] = (float)var[c];
      save_mean->flat<float>()[c] = (float)mean[c];
      save_inv->flat<float>()[c] = inv[c];
    }
    for (int64_t i = 0; i < rows; ++i)
      for (int64_t c = 0; c < C; ++c)
        yp[i * C + c] =
            ((xp[i * C + c] - (float)mean[c]) * inv[c]) * sc[c] + of[c];
  }

 private:
  float eps_ = 1e-4f;
  bool training_ = true;
};
REGISTER_KERNEL_BUILDER(Name("FusedBatchNorm").Device(DEVICE_CPU).TypeConstraint<float>("T"), FusedBatchNormOp);

class FusedBatchNormGradOp : public OpKernel {
 public:
  explicit FusedBatchNormGradOp(OpKernelConstruction* ctx) : OpKernel(ctx) {
    ctx->GetAttr("epsilon", &eps_);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& dy = ctx->input(0);
    const Tensor& x = ctx->input(1);
    const Tensor& scale = ctx->input(2);
    const Tensor& saved_mean = ctx->input(3);
    const Tensor& saved_inv = ctx->input(4);  // 1/sqrt(var+eps)
    int64_t C = x.dim_size(3);
    int64_t rows = x.NumElements() / C;
    Tensor* dx = ctx->allocate_output(0, x.shape());
    Tensor* dscale = ctx->allocate_output(1, TensorShape({C}));
    Tensor* doffset = ctx->allocate_output(2, TensorShape({C}));
    ctx->allocate_output(3, TensorShape({0}));
    ctx->allocate_output(4, TensorShape({0}));
    const float* g = dy.flat<float>();
    const float* xp = x.flat<float>();
    const float* sc = scale.flat<float>();
    const float* mu = saved_mean.flat<float>();
    const float* inv = saved_inv.flat<float>();
    float* dxp = dx->flat<float>();
    std::vector<double> sum_dy(C, 0), sum_dy_xhat(C, 0);
    for (int64_t i = 0; i < rows; ++i)
      for (int64_t c = 0; c < C; ++c) {
        float xhat = (xp[i * C + c] - mu[c]) * inv[c];
        sum_dy[c] += g[i * C + c];
        sum_dy_xhat[c] += g[i * C + c] * xhat;
      }
    for (int64_t c = 0; c < C; ++c) {
      dscale->flat<float>()[c] = (float)sum_dy_xhat[c];
      doffset->flat<float>()[c] = (float)sum_dy[c];
    }
    for (int64_t i = 0; i < rows; ++i)
      for (int64_t c = 0; c < C; ++c) {
        float xhat = (xp[i * C + c] - mu[c]) * inv[c];
        dxp[i * C + c] =
            sc[c] * inv[c] *
            (g[i * C + c] - (float)sum_dy[c] / rows -
             xhat * (float)sum_dy_xhat[c] / rows);
      }
  }

 private:
  float eps_ = 1e-4f;
};
REGISTER_KERNEL_BUILDER(Name("FusedBatchNormGrad").Device(DEVICE_CPU).TypeConstraint<float>("T"), FusedBatchNormGradOp);


// ---------------------- depthwise conv (CPU reference) ----------------------
// (reference core/kernels/depthwise_conv_op.cc; plain loops, f32 accum)
namespace {

// d.K is the channel multiplier of the [R, S, C, mult] filter.
template <typename T>
class CpuDepthwiseConvOp : public OpKernel {
 public:
  explicit CpuDepthwiseConvOp(OpKernelConstruction* c)
      : OpKernel(c), attrs_(c) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    const Tensor& w = ctx->input(1);
    ConvGeom d;
    OP_REQUIRES_OK(ctx, MakeConvGeom(x.shape(), w.shape(), attrs_, &d));
    Tensor* y = ctx->allocate_output(
        0, TensorShape({d.N, d.P, d.Q, d.C * d.K}));
    const T* xp = x.flat<T>();
    const T* wp = w.flat<T>();
    T* yp = y->flat<T>();
    int64_t CM = d.C * d.K;
    for (int64_t n = 0; n < d.N; ++n)
      for (int64_t p = 0; p < d.P; ++p)
        for (int64_t q = 0; q < d.Q; ++q)
          for (int64_t c = 0; c < d.C; ++c)
            for (int64_t m = 0; m < d.K; ++m) {
              float acc = 0.f;
              for (int64_t r = 0; r < d.R; ++r) {
                int64_t ih = p * d.sh - d.ph + r;
                if (ih < 0 || ih >= d.H) continue;
                for (int64_t s2 = 0; s2 < d.S; ++s2) {
                  int64_t iw = q * d.sw - d.pw + s2;
                  if (iw < 0 || iw >= d.W) continue;
                  acc += (float)xp[((n * d.H + ih) * d.W + iw) * d.C + c] *
                         (float)wp[((r * d.S + s2) * d.C + c) * d.K + m];
                }
              }
              yp[((n * d.P + p) * d.Q + q) * CM + c * d.K + m] = (T)acc;
            }
  }

 private:
  ConvAttrs attrs_;
};
REGISTER_KERNEL_BUILDER(Name("DepthwiseConv2dNative").Device(DEVICE_CPU).TypeConstraint<float>("T"), CpuDepthwiseConvOp<float>);
REGISTER_KERNEL_BUILDER(Name("DepthwiseConv2dNative").Device(DEVICE_CPU).TypeConstraint<bfloat16>("T"), CpuDepthwiseConvOp<bfloat16>);

// Local response normalization over the channel (last) axis:
// y_i = x_i / (bias + alpha * sum_{|j-i|<=r} x_j^2)^beta
// (reference lrn_op.cc; the backward pass is a python composite in
// python/ops/nn_grad.py _lrn_grad).
class LRNOp : public OpKernel {
 public:
  explicit LRNOp(OpKernelConstruction* ctx) : OpKernel(ctx) {
    ctx->GetAttr("depth_radius", &radius_);
    ctx->GetAttr("bias", &bias_);
    ctx->GetAttr("alpha", &alpha_);
    ctx->GetAttr("beta", &beta_);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    Tensor* out = ctx->allocate_output(0, in.shape());
    int64_t c = in.shape().dim_size(in.shape().dims() - 1);
    int64_t rows = in.NumElements() / c;
    const float* x = in.flat<float>();
    float* y = out->flat<float>();
    for (int64_t rI = 0; rI < rows; ++rI) {
      const float* xr = x + rI * c;
      float* yr = y + rI * c;
      for (int64_t k = 0; k < c; ++k) {
        int64_t lo = k - radius_ < 0 ? 0 : k - radius_;
        int64_t hi = k + radius_ + 1 > c ? c : k + radius_ + 1;
        float s = bias_;
        for (int64_t j = lo; j < hi; ++j) s += alpha_ * xr[j] * xr[j];
        yr[k] = xr[k] / std::pow(s, beta_);
      }
    }
  }

 private:
  int64_t radius_ = 5;
  float bias_ = 1.f, alpha_ = 1.f, beta_ = 0.5f;
};
REGISTER_KERNEL_BUILDER(Name("LRN").Device(DEVICE_CPU), LRNOp);

// ------------------------- fused LSTM cell pointwise ------------------------
// CPU reference of the GPU LstmGates kernels (hip/lstm.hip); gate order
// i, j, f, o as produced by BasicLSTMCell's single [B, 4H] GEMM.
template <typename T>
class LSTMGatesOp : public OpKernel {
 public:
  explicit LSTMGatesOp(OpKernelConstruction* ctx) : OpKernel(ctx) {
    ctx->GetAttr("forget_bias", &forget_bias_);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& gates = ctx->input(0);
    const Tensor& c_prev = ctx->input(1);
    int64_t B = c_prev.shape().dim_size(0);
    int64_t H = c_prev.shape().dim_size(1);
    Tensor* outs[7];
    for (int k = 0; k < 7; ++k) outs[k] = ctx->allocate_output(k, c_prev.shape());
    const T* g = gates.flat<T>();
    const T* cp = c_prev.flat<T>();
    for (int64_t b = 0; b < B; ++b) {
      const T* gr = g + b * 4 * H;
      for (int64_t h = 0; h < H; ++h) {
        float i = 1.f / (1.f + std::exp(-(float)gr[h]));
        float ci = std::tanh((float)gr[H + h]);
        float f = 1.f / (1.f + std::exp(-((float)gr[2 * H + h] + forget_bias_)));
        float o = 1.f / (1.f + std::exp(-(float)gr[3 * H + h]));
        float cs = f * (float)cp[b * H + h] + i * ci;
        float co = std::tanh(cs);
        int64_t idx = b * H + h;
        outs[0]->flat<T>()[idx] = (T)i;
        outs[1]->flat<T>()[idx] = (T)f;
        outs[2]->flat<T>()[idx] = (T)o;
        outs[3]->flat<T>()[idx] = (T)ci;
        outs[4]->flat<T>()[idx] = (T)cs;
        outs[5]->flat<T>()[idx] = (T)co;
        outs[6]->flat<T>()[idx] = (T)(o * co);
      }
    }
  }

 private:
  float forget_bias_ = 1.f;
};
REGISTER_KERNEL_BUILDER(Name("LSTMGates").Device(DEVICE_CPU).TypeConstraint<float>("T"), LSTMGatesOp<float>);
REGISTER_KERNEL_BUILDER(Name("LSTMGates").Device(DEVICE_CPU).TypeConstraint<bfloat16>("T"), LSTMGatesOp<bfloat16>);

template <typename T>
class LSTMGatesGradOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& c_prev = ctx->input(0);
    int64_t B = c_prev.shape().dim_size(0);
    int64_t H = c_prev.shape().dim_size(1);
    const T* cp = c_prev.flat<T>();
    const T* i_ = ctx->input(1).flat<T>();
    const T* f_ = ctx->input(2).flat<T>();
    const T* o_ = ctx->input(3).flat<T>();
    const T* ci_ = ctx->input(4).flat<T>();
    const T* co_ = ctx->input(5).flat<T>();
    const T* dh = ctx->input(6).flat<T>();
    const T* dcsn = ctx->input(7).flat<T>();
    Tensor* dgates = ctx->allocate_output(0, TensorShape({B, 4 * H}));
    Tensor* dc_prev = ctx->allocate_output(1, c_prev.shape());
    T* dg = dgates->flat<T>();
    T* dcp = dc_prev->flat<T>();
    for (int64_t idx = 0; idx < B * H; ++idx) {
      int64_t b = idx / H, h = idx % H;
      float i = (float)i_[idx], f = (float)f_[idx], o = (float)o_[idx];
      float ci = (float)ci_[idx], co = (float)co_[idx];
      float dhv = (float)dh[idx];
      float dcs = dhv * o * (1.f - co * co) + (float)dcsn[idx];
      T* row = dg + b * 4 * H;
      row[h] = (T)(dcs * ci * i * (1.f - i));
      row[H + h] = (T)(dcs * i * (1.f - ci * ci));
      row[2 * H + h] = (T)(dcs * (float)cp[idx] * f * (1.f - f));
      row[3 * H + h] = (T)(dhv * co * o * (1.f - o));
      dcp[idx] = (T)(dcs * f);
    }
  }
};
REGISTER_KERNEL_BUILDER(Name("LSTMGatesGrad").Device(DEVICE_CPU).TypeConstraint<float>("T"), LSTMGatesGradOp<float>);
REGISTER_KERNEL_BUILDER(Name("LSTMGatesGrad").Device(DEVICE_CPU).TypeConstraint<bfloat16>("T"), LSTMGatesGradOp<bfloat16>);

}  // namespace

}  // namespace stf
