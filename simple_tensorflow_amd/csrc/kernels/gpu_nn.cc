// GPU OpKernels: bias, softmax/xent, batch norm, pooling, LRN, LSTM gates, L2Loss.
#include "kernels/gpu_common.h"

namespace stf {
namespace {

// ---------------------------------------------------------------------------
// bias / softmax / xent
// ---------------------------------------------------------------------------
class GpuBiasAddOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    const Tensor& b = ctx->input(1);
    Tensor* y = ctx->allocate_output(0, x.shape());
    OP_HIP_OK(ctx, stf_bias_add(DtypeCode(x.dtype()), x.raw_data(),
                                b.raw_data(), y->raw_data(), x.NumElements(),
                                (int)b.NumElements(), GPU_STREAM(ctx)));
  }
};
REGISTER_KERNEL_BUILDER(Name("BiasAdd").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuBiasAddOp);
REGISTER_KERNEL_BUILDER(Name("BiasAdd").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuBiasAddOp);

class GpuBiasAddGradOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& dy = ctx->input(0);
    int c = (int)dy.dim_size(dy.dims() - 1);
    int64_t rows = c ? dy.NumElements() / c : 0;
    Tensor* db = ctx->allocate_output(0, TensorShape({c}));
    hipStream_t s = GPU_STREAM(ctx);
    Tensor scratch = ctx->allocate_temp(DT_FLOAT, TensorShape({c}));
    OP_HIP_OK(ctx, ZeroF32(scratch.raw_data(), c, s));
    OP_HIP_OK(ctx, stf_bias_grad(DtypeCode(dy.dtype()), dy.raw_data(),
                                 scratch.raw_data(), rows, c, s));
    OP_HIP_OK(ctx, stf_cast(0, CastCode(db->dtype()), scratch.raw_data(),
                            db->raw_data(), c, s));
  }
};
REGISTER_KERNEL_BUILDER(Name("BiasAddGrad").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuBiasAddGradOp);
REGISTER_KERNEL_BUILDER(Name("BiasAddGrad").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuBiasAddGradOp);

class GpuSoftmaxOp : public OpKernel {
 public:
  GpuSoftmaxOp(OpKernelConstruction* c, bool log_sm)
      : OpKernel(c), log_(log_sm) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    Tensor* y = ctx->allocate_output(0, x.shape());
    int cols = (int)x.dim_size(x.dims() - 1);
    int64_t rows = cols ? x.NumElements() / cols : 0;
    OP_HIP_OK(ctx, stf_softmax(DtypeCode(x.dtype()), log_, x.raw_data(),
                               y->raw_data(), rows, cols, GPU_STREAM(ctx)));
  }

 private:
  bool log_;
};
class SoftmaxGpu : public GpuSoftmaxOp {
 public:
  explicit SoftmaxGpu(OpKernelConstruction* c) : GpuSoftmaxOp(c, false) {}
};
class LogSoftmaxGpu : public GpuSoftmaxOp {
 public:
  explicit LogSoftmaxGpu(OpKernelConstruction* c) : GpuSoftmaxOp(c, true) {}
};
REGISTER_KERNEL_BUILDER(Name("Softmax").Device(DEVICE_GPU).TypeConstraint<float>("T"), SoftmaxGpu);
REGISTER_KERNEL_BUILDER(Name("Softmax").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), SoftmaxGpu);
REGISTER_KERNEL_BUILDER(Name("LogSoftmax").Device(DEVICE_GPU).TypeConstraint<float>("T"), LogSoftmaxGpu);

class GpuSparseXentOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& logits = ctx->input(0);
    const Tensor& labels = ctx->input(1);
    int64_t rows = logits.dim_size(0);
    int cols = (int)logits.dim_size(1);
    Tensor* loss = ctx->allocate_output(0, TensorShape({rows}));
    Tensor* bp = ctx->allocate_output(1, logits.shape());
    hipStream_t s = GPU_STREAM(ctx);
    Tensor loss_f32 = ctx->allocate_temp(DT_FLOAT, TensorShape({rows}));
    OP_HIP_OK(ctx,
              stf_sparse_xent(DtypeCode(logits.dtype()), logits.raw_data(),
                              labels.raw_data(), labels.dtype() == DT_INT32,
                              loss_f32.raw_data(), bp->raw_data(), rows, cols,
                              s));
    OP_HIP_OK(ctx, stf_cast(0, CastCode(loss->dtype()), loss_f32.raw_data(),
                            loss->raw_data(), rows, s));
  }
};
REGISTER_KERNEL_BUILDER(Name("SparseSoftmaxCrossEntropyWithLogits").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuSparseXentOp);
REGISTER_KERNEL_BUILDER(Name("SparseSoftmaxCrossEntropyWithLogits").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuSparseXentOp);

class GpuXentOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& logits = ctx->input(0);
    const Tensor& labels = ctx->input(1);
    int64_t rows = logits.dim_size(0);
    int cols = (int)logits.dim_size(1);
    Tensor* loss = ctx->allocate_output(0, TensorShape({rows}));
    Tensor* bp = ctx->allocate_output(1, logits.shape());
    hipStream_t s = GPU_STREAM(ctx);
    Tensor loss_f32 = ctx->allocate_temp(DT_FLOAT, TensorShape({rows}));
    OP_HIP_OK(ctx, stf_xent(DtypeCode(logits.dtype()), logits.raw_data(),
                            labels.raw_data(), loss_f32.raw_data(),
                            bp->raw_data(), rows, cols, s));
    OP_HIP_OK(ctx, stf_cast(0, CastCode(loss->dtype()), loss_f32.raw_data(),
                            loss->raw_data(), rows, s));
  }
};
REGISTER_KERNEL_BUILDER(Name("SoftmaxCrossEntropyWithLogits").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuXentOp);
REGISTER_KERNEL_BUILDER(Name("SoftmaxCrossEntropyWithLogits").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuXentOp);

// ---------------------------------------------------------------------------
// batch norm
// ---------------------------------------------------------------------------
// given_sums (the _...Stats forms, fed by _Conv2DBnStats): the last input is
// float[2c], the per-channel sum and sum of squares of x, so the pass that
// reads x to form them is skipped.
class GpuBatchNormMiOp : public OpKernel {
 public:
  explicit GpuBatchNormMiOp(OpKernelConstruction* c, bool given_sums = false)
      : OpKernel(c), given_sums_(given_sums) {
    c->GetAttr("epsilon", &eps_);
    c->GetAttr("fuse_relu", &fuse_relu_);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    const Tensor& scale = ctx->input(1);
    const Tensor& offset = ctx->input(2);
    int c = (int)x.dim_size(x.dims() - 1);
    int64_t rows = x.NumElements() / c;
    Tensor* y = ctx->allocate_output(0, x.shape());
    Tensor* mean = ctx->allocate_output(1, TensorShape({c}));
    Tensor* var = ctx->allocate_output(2, TensorShape({c}));
    Tensor* inv_std = ctx->allocate_output(3, TensorShape({c}));
    hipStream_t s = GPU_STREAM(ctx);
    if (given_sums_) {
      const Tensor& sums = ctx->input(3);
      OP_REQUIRES(ctx, sums.NumElements() == 2 * c,
                  errors::InvalidArgument("_BatchNormMiStats: sums size"));
      OP_HIP_OK(ctx, stf_bn_fwd_acc(DtypeCode(x.dtype()), x.raw_data(),
                                    scale.raw_data(), offset.raw_data(),
                                    sums.flat<float>(), mean->flat<float>(),
                                    var->flat<float>(),
                                    inv_std->flat<float>(), y->raw_data(),
                                    rows, c, eps_, fuse_relu_ ? 1 : 0, s));
      return;
    }
    Tensor acc = ctx->allocate_temp(DT_FLOAT, TensorShape({2 * c}));
    OP_HIP_OK(ctx, ZeroF32(acc.raw_data(), 2 * c, s));
    OP_HIP_OK(ctx, stf_bn_fwd(DtypeCode(x.dtype()), x.raw_data(),
                              scale.raw_data(), offset.raw_data(),
                              acc.flat<float>(), mean->flat<float>(),
                              var->flat<float>(), inv_std->flat<float>(),
                              y->raw_data(), rows, c, eps_,
                              fuse_relu_ ? 1 : 0, s));
  }

 private:
  bool given_sums_;
  float eps_ = 1e-4f;
  bool fuse_relu_ = false;
};
class GpuBatchNormMiStatsOp : public GpuBatchNormMiOp {
 public:
  explicit GpuBatchNormMiStatsOp(OpKernelConstruction* c)
      : GpuBatchNormMiOp(c, true) {}
};
REGISTER_KERNEL_BUILDER(Name("_BatchNormMiStats").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuBatchNormMiStatsOp);
REGISTER_KERNEL_BUILDER(Name("BatchNormMi").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuBatchNormMiOp);
REGISTER_KERNEL_BUILDER(Name("BatchNormMi").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuBatchNormMiOp);

// BN + residual-add + relu fused (reference has no equivalent; the CDNA4
// win is one elementwise pass instead of three over a [N,H,W,C] tensor).
class GpuBatchNormAddReluMiOp : public OpKernel {
 public:
  explicit GpuBatchNormAddReluMiOp(OpKernelConstruction* c,
                                   bool given_sums = false)
      : OpKernel(c), given_sums_(given_sums) {
    c->GetAttr("epsilon", &eps_);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    const Tensor& scale = ctx->input(1);
    const Tensor& offset = ctx->input(2);
    const Tensor& side = ctx->input(3);
    int c = (int)x.dim_size(x.dims() - 1);
    int64_t rows = x.NumElements() / c;
    Tensor* y = ctx->allocate_output(0, x.shape());
    Tensor* mean = ctx->allocate_output(1, TensorShape({c}));
    Tensor* var = ctx->allocate_output(2, TensorShape({c}));
    Tensor* inv_std = ctx->allocate_output(3, TensorShape({c}));
    hipStream_t s = GPU_STREAM(ctx);
    if (given_sums_) {  // see GpuBatchNormMiOp
      const Tensor& sums = ctx->input(4);
      OP_REQUIRES(ctx, sums.NumElements() == 2 * c,
                  errors::InvalidArgument(
                      "_BatchNormAddReluMiStats: sums size"));
      OP_HIP_OK(ctx, stf_bn_add_relu_acc(x.raw_data(), side.raw_data(),
                                         sums.flat<float>(),
                                         mean->flat<float>(),
                                         var->flat<float>(),
                                         inv_std->flat<float>(),
                                         scale.raw_data(), offset.raw_data(),
                                         y->raw_data(), rows, c, eps_, s));
      return;
    }
    Tensor acc = ctx->allocate_temp(DT_FLOAT, TensorShape({2 * c}));
    OP_HIP_OK(ctx, ZeroF32(acc.raw_data(), 2 * c, s));
    // stats + finalize from the plain BN path, then the fused normalize
    OP_HIP_OK(ctx, stf_bn_stats_only(DtypeCode(x.dtype()), x.raw_data(),
                                     acc.flat<float>(), mean->flat<float>(),
                                     var->flat<float>(),
                                     inv_std->flat<float>(), rows, c, eps_,
                                     s));
    OP_HIP_OK(ctx, stf_bn_add_relu(x.raw_data(), side.raw_data(),
                                   mean->flat<float>(),
                                   inv_std->flat<float>(), scale.raw_data(),
                                   offset.raw_data(), y->raw_data(), rows, c,
                                   s));
  }

 private:
  bool given_sums_;
  float eps_ = 1e-4f;
};
REGISTER_KERNEL_BUILDER(Name("BatchNormAddReluMi").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuBatchNormAddReluMiOp);
class GpuBatchNormAddReluMiStatsOp : public GpuBatchNormAddReluMiOp {
 public:
  explicit GpuBatchNormAddReluMiStatsOp(OpKernelConstruction* c)
      : GpuBatchNormAddReluMiOp(c, true) {}
};
REGISTER_KERNEL_BUILDER(Name("_BatchNormAddReluMiStats").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuBatchNormAddReluMiStatsOp);

class GpuBatchNormMiGradOp : public OpKernel {
 public:
  explicit GpuBatchNormMiGradOp(OpKernelConstruction* c) : OpKernel(c) {
    c->GetAttr("fuse_relu", &fuse_relu_);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& dy = ctx->input(0);
    const Tensor& x = ctx->input(1);
    const Tensor& scale = ctx->input(2);
    const Tensor& mean = ctx->input(3);
    const Tensor& inv_std = ctx->input(4);
    const Tensor& y_relu = ctx->input(5);
    int c = (int)x.dim_size(x.dims() - 1);
    int64_t rows = x.NumElements() / c;
    Tensor* dx = ctx->allocate_output(0, x.shape());
    Tensor* dscale = ctx->allocate_output(1, TensorShape({c}));
    Tensor* doffset = ctx->allocate_output(2, TensorShape({c}));
    hipStream_t s = GPU_STREAM(ctx);
    // stats accumulate straight into the gradient outputs (sum_dy ==
    // doffset, sum_dy_xhat == dscale) — no scratch, no d2d copies.
    OP_HIP_OK(ctx, ZeroF32(doffset->raw_data(), c, s));
    OP_HIP_OK(ctx, ZeroF32(dscale->raw_data(), c, s));
    OP_HIP_OK(ctx, stf_bn_bwd(DtypeCode(x.dtype()), dy.raw_data(),
                              x.raw_data(), y_relu.raw_data(),
                              mean.flat<float>(), inv_std.flat<float>(),
                              scale.raw_data(), doffset->flat<float>(),
                              dscale->flat<float>(), dx->raw_data(), nullptr,
                              rows, c, fuse_relu_ ? 1 : 0, s));
  }

 private:
  bool fuse_relu_ = false;
};
class GpuBatchNormAddReluMiGradOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& dy = ctx->input(0);
    const Tensor& x = ctx->input(1);
    const Tensor& scale = ctx->input(2);
    const Tensor& mean = ctx->input(3);
    const Tensor& inv_std = ctx->input(4);
    const Tensor& y_relu = ctx->input(5);
    int c = (int)x.dim_size(x.dims() - 1);
    int64_t rows = x.NumElements() / c;
    Tensor* dx = ctx->allocate_output(0, x.shape());
    Tensor* dscale = ctx->allocate_output(1, TensorShape({c}));
    Tensor* doffset = ctx->allocate_output(2, TensorShape({c}));
    Tensor* dside = ctx->allocate_output(3, x.shape());
    hipStream_t s = GPU_STREAM(ctx);
    OP_HIP_OK(ctx, ZeroF32(doffset->raw_data(), c, s));
    OP_HIP_OK(ctx, ZeroF32(dscale->raw_data(), c, s));
    // dside (the ReLU-masked dy) is stored by the same kernel that writes dx
    OP_HIP_OK(ctx, stf_bn_bwd(DtypeCode(x.dtype()), dy.raw_data(),
                              x.raw_data(), y_relu.raw_data(),
                              mean.flat<float>(), inv_std.flat<float>(),
                              scale.raw_data(), doffset->flat<float>(),
                              dscale->flat<float>(), dx->raw_data(),
                              dside->raw_data(), rows, c, 1, s));
  }
};
REGISTER_KERNEL_BUILDER(Name("BatchNormAddReluMiGrad").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuBatchNormAddReluMiGradOp);

REGISTER_KERNEL_BUILDER(Name("BatchNormMiGrad").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuBatchNormMiGradOp);
REGISTER_KERNEL_BUILDER(Name("BatchNormMiGrad").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuBatchNormMiGradOp);

// ---------------------------------------------------------------------------
// pooling
// ---------------------------------------------------------------------------
class GpuPoolOp : public OpKernel {
 public:
  GpuPoolOp(OpKernelConstruction* c, bool is_max)
      : OpKernel(c), is_max_(is_max), p_(c) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    StfPoolGeom g;
    OP_REQUIRES_OK(ctx, MakePoolGeom(x.shape(), p_, &g));
    Tensor* y = ctx->allocate_output(0, TensorShape({g.N, g.P, g.Q, g.C}));
    OP_HIP_OK(ctx, stf_pool_fwd(DtypeCode(x.dtype()), is_max_, x.raw_data(),
                                y->raw_data(), &g, GPU_STREAM(ctx)));
  }

 private:
  bool is_max_;
  PoolAttrs p_;
};
class MaxPoolGpu : public GpuPoolOp {
 public:
  explicit MaxPoolGpu(OpKernelConstruction* c) : GpuPoolOp(c, true) {}
};
class AvgPoolGpu : public GpuPoolOp {
 public:
  explicit AvgPoolGpu(OpKernelConstruction* c) : GpuPoolOp(c, false) {}
};
REGISTER_KERNEL_BUILDER(Name("MaxPool").Device(DEVICE_GPU).TypeConstraint<float>("T"), MaxPoolGpu);
REGISTER_KERNEL_BUILDER(Name("MaxPool").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), MaxPoolGpu);
REGISTER_KERNEL_BUILDER(Name("AvgPool").Device(DEVICE_GPU).TypeConstraint<float>("T"), AvgPoolGpu);
REGISTER_KERNEL_BUILDER(Name("AvgPool").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), AvgPoolGpu);

class GpuMaxPoolGradOp : public OpKernel {
 public:
  explicit GpuMaxPoolGradOp(OpKernelConstruction* c) : OpKernel(c), p_(c) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    const Tensor& dy = ctx->input(2);
    StfPoolGeom g;
    OP_REQUIRES_OK(ctx, MakePoolGeom(x.shape(), p_, &g));
    Tensor* dx = ctx->allocate_output(0, x.shape());
    hipStream_t s = GPU_STREAM(ctx);
    if (x.dtype() == DT_BFLOAT16 && g.C % 8 == 0) {
      // per-input direct path: no f32 scratch, no zero fill, no cast
      OP_HIP_OK(ctx, stf_max_pool_bwd_v8(x.raw_data(), dy.raw_data(),
                                         dx->raw_data(), &g, s));
      return;
    }
    Tensor scratch = ctx->allocate_temp(DT_FLOAT, x.shape());
    OP_HIP_OK(ctx, ZeroF32(scratch.raw_data(), x.NumElements(), s));
    OP_HIP_OK(ctx, stf_max_pool_bwd(DtypeCode(x.dtype()), x.raw_data(),
                                    dy.raw_data(), scratch.flat<float>(), &g,
                                    s));
    OP_HIP_OK(ctx, stf_cast(0, CastCode(dx->dtype()), scratch.raw_data(),
                            dx->raw_data(), x.NumElements(), s));
  }

 private:
  PoolAttrs p_;
};
REGISTER_KERNEL_BUILDER(Name("MaxPoolGrad").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuMaxPoolGradOp);
REGISTER_KERNEL_BUILDER(Name("MaxPoolGrad").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuMaxPoolGradOp);

class GpuAvgPoolGradOp : public OpKernel {
 public:
  explicit GpuAvgPoolGradOp(OpKernelConstruction* c) : OpKernel(c), p_(c) {}
  void Compute(OpKernelContext* ctx) override {
    auto in_sizes = IntVector(ctx->input(0));
    const Tensor& dy = ctx->input(1);
    TensorShape x_shape(in_sizes);
    StfPoolGeom g;
    OP_REQUIRES_OK(ctx, MakePoolGeom(x_shape, p_, &g));
    Tensor* dx = ctx->allocate_output(0, x_shape);
    OP_HIP_OK(ctx, stf_avg_pool_bwd(DtypeCode(dy.dtype()), dy.raw_data(),
                                    dx->raw_data(), &g, GPU_STREAM(ctx)));
  }

 private:
  PoolAttrs p_;
};
REGISTER_KERNEL_BUILDER(Name("AvgPoolGrad").Device(DEVICE_GPU).TypeConstraint<float>("T").HostMemory("orig_input_shape"), GpuAvgPoolGradOp);
REGISTER_KERNEL_BUILDER(Name("AvgPoolGrad").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T").HostMemory("orig_input_shape"), GpuAvgPoolGradOp);

// LRN forward on GPU (reference used cuDNN, lrn_op.cc:211). The composite
// python gradient runs on the GPU's elementwise kernels.
class GpuLRNOp : public OpKernel {
 public:
  explicit GpuLRNOp(OpKernelConstruction* c) : OpKernel(c) {
    c->GetAttr("depth_radius", &radius_);
    c->GetAttr("bias", &bias_);
    c->GetAttr("alpha", &alpha_);
    c->GetAttr("beta", &beta_);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    Tensor* y = ctx->allocate_output(0, x.shape());
    int64_t c = x.dim_size(x.dims() - 1);
    OP_HIP_OK(ctx, stf_lrn_fwd(x.raw_data(), y->raw_data(),
                               x.NumElements() / c, (int)c, (int)radius_,
                               bias_, alpha_, beta_, GPU_STREAM(ctx)));
  }

 private:
  int64_t radius_ = 5;
  float bias_ = 1.f, alpha_ = 1.f, beta_ = 0.5f;
};
REGISTER_KERNEL_BUILDER(Name("LRN").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuLRNOp);

// L2Loss: 0.5 * sum(x^2) — square into a temp then full-reduce (the
// reference's l2loss_op_gpu; without this PTB's clip_by_global_norm dragged
// multi-MB gradients through a CPU-placed reduction at ~22 s/step).
class GpuL2LossOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    hipStream_t s = GPU_STREAM(ctx);
    int dt = DtypeCode(x.dtype());
    int64_t n = x.NumElements();
    Tensor* out = ctx->allocate_output(0, TensorShape({}));
    if (x.dtype() == DT_FLOAT) {
      OP_HIP_OK(ctx, ZeroF32(out->raw_data(), 1, s));
      OP_HIP_OK(ctx, stf_l2loss(dt, x.raw_data(), out->flat<float>(), n, s));
    } else {
      Tensor acc = ctx->allocate_temp(DT_FLOAT, TensorShape({}));
      OP_HIP_OK(ctx, ZeroF32(acc.raw_data(), 1, s));
      OP_HIP_OK(ctx, stf_l2loss(dt, x.raw_data(), acc.flat<float>(), n, s));
      OP_HIP_OK(ctx, stf_cast(0, CastCode(x.dtype()), acc.raw_data(),
                              out->raw_data(), 1, s));
    }
  }
};
REGISTER_KERNEL_BUILDER(Name("L2Loss").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuL2LossOp);
REGISTER_KERNEL_BUILDER(Name("L2Loss").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuL2LossOp);

// Fused LSTM cell pointwise (hip/lstm.hip LstmGatesKernel); one launch
// replaces the composed cell's ~17 elementwise/split launches per timestep.
class GpuLSTMGatesOp : public OpKernel {
 public:
  explicit GpuLSTMGatesOp(OpKernelConstruction* c) : OpKernel(c) {
    c->GetAttr("forget_bias", &forget_bias_);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& gates = ctx->input(0);
    const Tensor& c_prev = ctx->input(1);
    int64_t B = c_prev.shape().dim_size(0);
    int64_t H = c_prev.shape().dim_size(1);
    void* outs[7];
    for (int k = 0; k < 7; ++k)
      outs[k] = ctx->allocate_output(k, c_prev.shape())->raw_data();
    OP_HIP_OK(ctx, stf_lstm_gates(DtypeCode(gates.dtype()), gates.raw_data(),
                                  c_prev.raw_data(), forget_bias_, outs[0],
                                  outs[1], outs[2], outs[3], outs[4], outs[5],
                                  outs[6], B, (int)H, GPU_STREAM(ctx)));
  }

 private:
  float forget_bias_ = 1.f;
};
REGISTER_KERNEL_BUILDER(Name("LSTMGates").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuLSTMGatesOp);
REGISTER_KERNEL_BUILDER(Name("LSTMGates").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuLSTMGatesOp);

class GpuLSTMGatesGradOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& c_prev = ctx->input(0);
    int64_t B = c_prev.shape().dim_size(0);
    int64_t H = c_prev.shape().dim_size(1);
    Tensor* dgates = ctx->allocate_output(0, TensorShape({B, 4 * H}));
    Tensor* dc_prev = ctx->allocate_output(1, c_prev.shape());
    OP_HIP_OK(ctx, stf_lstm_gates_grad(
                       DtypeCode(c_prev.dtype()), c_prev.raw_data(),
                       ctx->input(1).raw_data(), ctx->input(2).raw_data(),
                       ctx->input(3).raw_data(), ctx->input(4).raw_data(),
                       ctx->input(5).raw_data(), ctx->input(6).raw_data(),
                       ctx->input(7).raw_data(), dgates->raw_data(),
                       dc_prev->raw_data(), B, (int)H, GPU_STREAM(ctx)));
  }
};
REGISTER_KERNEL_BUILDER(Name("LSTMGatesGrad").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuLSTMGatesGradOp);
REGISTER_KERNEL_BUILDER(Name("LSTMGatesGrad").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuLSTMGatesGradOp);

}  // namespace
}  // namespace stf
