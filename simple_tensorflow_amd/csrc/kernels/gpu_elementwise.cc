// GPU OpKernels: unary, binary, cast, addn, fill, fused elementwise.
#include "kernels/gpu_common.h"

namespace stf {
namespace {

// ---------------------------------------------------------------------------
// elementwise
// ---------------------------------------------------------------------------
class GpuUnaryOp : public OpKernel {
 public:
  GpuUnaryOp(OpKernelConstruction* c, int op) : OpKernel(c), op_(op) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    Tensor* y = ctx->allocate_output(0, x.shape());
    OP_HIP_OK(ctx, stf_unary(op_, DtypeCode(x.dtype()), x.raw_data(),
                             y->raw_data(), x.NumElements(), GPU_STREAM(ctx)));
  }

 private:
  int op_;
};

#define REG_GPU_UNARY(NAME, CODE)                                             \
  struct NAME##GpuTag {};                                                     \
  class NAME##GpuOp : public GpuUnaryOp {                                     \
   public:                                                                    \
    explicit NAME##GpuOp(OpKernelConstruction* c) : GpuUnaryOp(c, CODE) {}    \
  };                                                                          \
  REGISTER_KERNEL_BUILDER(Name(#NAME).Device(DEVICE_GPU).TypeConstraint<float>("T"), NAME##GpuOp); \
  REGISTER_KERNEL_BUILDER(Name(#NAME).Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), NAME##GpuOp);

REG_GPU_UNARY(Neg, U_NEG)
REG_GPU_UNARY(Abs, U_ABS)
REG_GPU_UNARY(Sign, U_SIGN)
REG_GPU_UNARY(Square, U_SQUARE)
REG_GPU_UNARY(Sqrt, U_SQRT)
REG_GPU_UNARY(Rsqrt, U_RSQRT)
REG_GPU_UNARY(Exp, U_EXP)
REG_GPU_UNARY(Log, U_LOG)
REG_GPU_UNARY(Log1p, U_LOG1P)
REG_GPU_UNARY(Tanh, U_TANH)
REG_GPU_UNARY(Sigmoid, U_SIGMOID)
REG_GPU_UNARY(Relu, U_RELU)
REG_GPU_UNARY(Relu6, U_RELU6)
REG_GPU_UNARY(Softplus, U_SOFTPLUS)
REG_GPU_UNARY(Reciprocal, U_RECIP)
REG_GPU_UNARY(Floor, U_FLOOR)
REG_GPU_UNARY(Ceil, U_CEIL)
REG_GPU_UNARY(Sin, U_SIN)
REG_GPU_UNARY(Cos, U_COS)

class GpuBinaryOp : public OpKernel {
 public:
  GpuBinaryOp(OpKernelConstruction* c, int op) : OpKernel(c), op_(op) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& a = ctx->input(0);
    const Tensor& b = ctx->input(1);
    int dt = DtypeCode(a.dtype());
    hipStream_t s = GPU_STREAM(ctx);
    if (a.shape() == b.shape()) {
      Tensor* y = ctx->allocate_output(0, a.shape());
      OP_HIP_OK(ctx, stf_binary(op_, dt, a.raw_data(), b.raw_data(),
                                y->raw_data(), a.NumElements(), s));
      return;
    }
    // Scalar paths: the output takes the other side's shape, which is the
    // broadcast shape only while the scalar's rank does not exceed it.
    if (b.NumElements() == 1 && b.dims() <= a.dims()) {
      Tensor* y = ctx->allocate_output(0, a.shape());
      OP_HIP_OK(ctx, stf_binary_scalar(op_, dt, a.raw_data(), b.raw_data(),
                                       y->raw_data(), a.NumElements(), 0, s));
      return;
    }
    if (a.NumElements() == 1 && a.dims() <= b.dims()) {
      Tensor* y = ctx->allocate_output(0, b.shape());
      OP_HIP_OK(ctx, stf_binary_scalar(op_, dt, b.raw_data(), a.raw_data(),
                                       y->raw_data(), b.NumElements(), 1, s));
      return;
    }
    BCast bc(a.shape(), b.shape());
    OP_REQUIRES(ctx, bc.valid && bc.out.size() <= 6,
                errors::InvalidArgument("bad broadcast"));
    Tensor* y = ctx->allocate_output(0, bc.out_shape());
    OP_HIP_OK(ctx, stf_binary_bcast(op_, dt, a.raw_data(), b.raw_data(),
                                    y->raw_data(), bc.num_elements,
                                    (int)bc.out.size(), bc.out.data(),
                                    bc.sx.data(), bc.sy.data(), s));
  }

 private:
  int op_;
};

#define REG_GPU_BINARY(NAME, CODE)                                            \
  class NAME##GpuOp : public GpuBinaryOp {                                    \
   public:                                                                    \
    explicit NAME##GpuOp(OpKernelConstruction* c) : GpuBinaryOp(c, CODE) {}   \
  };                                                                          \
  REGISTER_KERNEL_BUILDER(Name(#NAME).Device(DEVICE_GPU).TypeConstraint<float>("T"), NAME##GpuOp); \
  REGISTER_KERNEL_BUILDER(Name(#NAME).Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), NAME##GpuOp);

REG_GPU_BINARY(Add, B_ADD)
REG_GPU_BINARY(Sub, B_SUB)
REG_GPU_BINARY(Mul, B_MUL)
REG_GPU_BINARY(RealDiv, B_DIV)
REG_GPU_BINARY(Div, B_DIV)
REG_GPU_BINARY(Maximum, B_MAX)
REG_GPU_BINARY(Minimum, B_MIN)
REG_GPU_BINARY(Pow, B_POW)
REG_GPU_BINARY(SquaredDifference, B_SQDIFF)
REG_GPU_BINARY(SigmoidGrad, B_SIGMOID_GRAD)
REG_GPU_BINARY(TanhGrad, B_TANH_GRAD)
REG_GPU_BINARY(RsqrtGrad, B_RSQRT_GRAD)
REG_GPU_BINARY(SqrtGrad, B_SQRT_GRAD)
REG_GPU_BINARY(ReluGrad, B_RELU_GRAD)
REG_GPU_BINARY(Relu6Grad, B_RELU6_GRAD)
REG_GPU_BINARY(SoftplusGrad, B_SOFTPLUS_GRAD)

class GpuCastOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    Tensor* y = ctx->allocate_output(0, x.shape());
    int sc = CastCode(x.dtype()), dc = CastCode(y->dtype());
    OP_REQUIRES(ctx, sc >= 0 && dc >= 0,
                errors::Unimplemented("GPU cast dtype"));
    OP_HIP_OK(ctx, stf_cast(sc, dc, x.raw_data(), y->raw_data(),
                            x.NumElements(), GPU_STREAM(ctx)));
  }
};
REGISTER_KERNEL_BUILDER(Name("Cast").Device(DEVICE_GPU), GpuCastOp);

class GpuAddNOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    int n = num_inputs();
    const Tensor& first = ctx->input(0);
    Tensor* y = ctx->allocate_output(0, first.shape());
    hipStream_t s = GPU_STREAM(ctx);
    int dt = DtypeCode(first.dtype());
    if (n == 1) {
      OP_HIP_OK(ctx, hipMemcpyAsync(y->raw_data(), first.raw_data(),
                                    first.TotalBytes(),
                                    hipMemcpyDeviceToDevice, s));
      return;
    }
    // pairwise adds: y = in0 + in1; y += in_k
    OP_HIP_OK(ctx, stf_binary(B_ADD, dt, first.raw_data(),
                              ctx->input(1).raw_data(), y->raw_data(),
                              first.NumElements(), s));
    for (int k = 2; k < n; ++k) {
      OP_HIP_OK(ctx, stf_binary(B_ADD, dt, y->raw_data(),
                                ctx->input(k).raw_data(), y->raw_data(),
                                first.NumElements(), s));
    }
  }
};
REGISTER_KERNEL_BUILDER(Name("AddN").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuAddNOp);
REGISTER_KERNEL_BUILDER(Name("AddN").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuAddNOp);

// ---------------------------------------------------------------------------
// fill-style
// ---------------------------------------------------------------------------
class GpuZerosLikeOp : public OpKernel {
 public:
  GpuZerosLikeOp(OpKernelConstruction* c, float v) : OpKernel(c), v_(v) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    Tensor* y = ctx->allocate_output(0, x.shape());
    OP_HIP_OK(ctx, stf_fill_f32(y->raw_data(), v_, x.NumElements(),
                                x.dtype() == DT_BFLOAT16, GPU_STREAM(ctx)));
  }

 private:
  float v_;
};
class ZerosLikeGpu : public GpuZerosLikeOp {
 public:
  explicit ZerosLikeGpu(OpKernelConstruction* c) : GpuZerosLikeOp(c, 0.f) {}
};
class OnesLikeGpu : public GpuZerosLikeOp {
 public:
  explicit OnesLikeGpu(OpKernelConstruction* c) : GpuZerosLikeOp(c, 1.f) {}
};
REGISTER_KERNEL_BUILDER(Name("ZerosLike").Device(DEVICE_GPU).TypeConstraint<float>("T"), ZerosLikeGpu);
REGISTER_KERNEL_BUILDER(Name("ZerosLike").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), ZerosLikeGpu);
REGISTER_KERNEL_BUILDER(Name("OnesLike").Device(DEVICE_GPU).TypeConstraint<float>("T"), OnesLikeGpu);
REGISTER_KERNEL_BUILDER(Name("OnesLike").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), OnesLikeGpu);

class GpuFillOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    auto dims = IntVector(ctx->input(0));
    const Tensor& v = ctx->input(1);  // host scalar
    Tensor* y = ctx->allocate_output(0, TensorShape(dims));
    float val = v.dtype() == DT_BFLOAT16
                    ? (float)v.flat<bfloat16>()[0]
                    : v.flat<float>()[0];
    OP_HIP_OK(ctx, stf_fill_f32(y->raw_data(), val, y->NumElements(),
                                y->dtype() == DT_BFLOAT16, GPU_STREAM(ctx)));
  }
};
REGISTER_KERNEL_BUILDER(Name("Fill").Device(DEVICE_GPU).TypeConstraint<float>("T").HostMemory("dims").HostMemory("value"), GpuFillOp);
REGISTER_KERNEL_BUILDER(Name("Fill").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T").HostMemory("dims").HostMemory("value"), GpuFillOp);

// _FusedElementwise: register-resident interpreter over the fused DAG
// (graph/optimizer.cc FuseElementwise; program format kernels/fused_ew.h).
class GpuFusedElementwiseOp : public OpKernel {
 public:
  explicit GpuFusedElementwiseOp(OpKernelConstruction* c) : OpKernel(c) {
    c->GetAttr("program", &prog_);
  }
  void Compute(OpKernelContext* ctx) override {
    int n_in = ctx->num_inputs();
    const Tensor& root = ctx->input(0);
    Tensor* out = ctx->allocate_output(0, root.shape());
    const void* ins[8];
    uint8_t scalar[8];
    for (int i = 0; i < n_in; ++i) {
      ins[i] = ctx->input(i).raw_data();
      scalar[i] = ctx->input(i).NumElements() == 1 ? 1 : 0;
    }
    OP_HIP_OK(ctx, stf_fused_elementwise(
                       DtypeCode(root.dtype()), ins, scalar, n_in,
                       prog_.data(), (int)prog_.size(), out->raw_data(),
                       root.NumElements(), GPU_STREAM(ctx)));
  }

 private:
  std::vector<int64_t> prog_;
};
REGISTER_KERNEL_BUILDER(Name("_FusedElementwise").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuFusedElementwiseOp);
REGISTER_KERNEL_BUILDER(Name("_FusedElementwise").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuFusedElementwiseOp);

}  // namespace
}  // namespace stf
