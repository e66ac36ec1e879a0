// GPU OpKernels: assign and the optimizer apply ops.
#include "kernels/gpu_common.h"

namespace stf {
namespace {

// ---------------------------------------------------------------------------
// state: Assign / AssignAdd / AssignSub
// ---------------------------------------------------------------------------
class GpuAssignOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    Tensor ref = ctx->input(0);
    const Tensor& value = ctx->input(1);
    OP_REQUIRES(ctx, ref.shape() == value.shape(),
                errors::InvalidArgument("Assign shape mismatch"));
    OP_HIP_OK(ctx, hipMemcpyAsync(ref.raw_data(), value.raw_data(),
                                  value.TotalBytes(), hipMemcpyDeviceToDevice,
                                  GPU_STREAM(ctx)));
    ctx->set_output(0, ref);
  }
};
REGISTER_KERNEL_BUILDER(Name("Assign").Device(DEVICE_GPU), GpuAssignOp);

template <int BOP>
class GpuAssignUpdateOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    Tensor ref = ctx->input(0);
    const Tensor& value = ctx->input(1);
    OP_HIP_OK(ctx, stf_binary(BOP, DtypeCode(ref.dtype()), ref.raw_data(),
                              value.raw_data(), ref.raw_data(),
                              ref.NumElements(), GPU_STREAM(ctx)));
    ctx->set_output(0, ref);
  }
};
REGISTER_KERNEL_BUILDER(Name("AssignAdd").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuAssignUpdateOp<B_ADD>);
REGISTER_KERNEL_BUILDER(Name("AssignSub").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuAssignUpdateOp<B_SUB>);

// ---------------------------------------------------------------------------
// optimizer applies (f32 vars)
// ---------------------------------------------------------------------------
class GpuApplySgdOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    Tensor var = ctx->input(0);
    const Tensor& lr = ctx->input(1);
    const Tensor& grad = ctx->input(2);
    OP_HIP_OK(ctx, stf_apply_sgd(grad.dtype() == DT_BFLOAT16, var.raw_data(),
                                 lr.raw_data(), grad.raw_data(),
                                 var.NumElements(), GPU_STREAM(ctx)));
    ctx->set_output(0, var);
  }
};
REGISTER_KERNEL_BUILDER(Name("ApplyGradientDescent").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuApplySgdOp);

class GpuApplyMomentumOp : public OpKernel {
 public:
  explicit GpuApplyMomentumOp(OpKernelConstruction* c) : OpKernel(c) {
    c->GetAttr("use_nesterov", &nesterov_);
  }
  void Compute(OpKernelContext* ctx) override {
    Tensor var = ctx->input(0);
    Tensor accum = ctx->input(1);
    const Tensor& lr = ctx->input(2);
    const Tensor& grad = ctx->input(3);
    const Tensor& mom = ctx->input(4);
    OP_HIP_OK(ctx, stf_apply_momentum(grad.dtype() == DT_BFLOAT16,
                                      var.raw_data(), accum.raw_data(),
                                      lr.raw_data(), grad.raw_data(),
                                      mom.raw_data(), nesterov_,
                                      var.NumElements(), GPU_STREAM(ctx)));
    ctx->set_output(0, var);
  }

 private:
  bool nesterov_ = false;
};
REGISTER_KERNEL_BUILDER(Name("ApplyMomentum").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuApplyMomentumOp);

class GpuApplyAdamOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    Tensor var = ctx->input(0);
    Tensor m = ctx->input(1);
    Tensor v = ctx->input(2);
    OP_HIP_OK(ctx, stf_apply_adam(
                       ctx->input(9).dtype() == DT_BFLOAT16, var.raw_data(),
                       m.raw_data(), v.raw_data(), ctx->input(3).raw_data(),
                       ctx->input(4).raw_data(), ctx->input(5).raw_data(),
                       ctx->input(6).raw_data(), ctx->input(7).raw_data(),
                       ctx->input(8).raw_data(), ctx->input(9).raw_data(),
                       var.NumElements(), GPU_STREAM(ctx)));
    ctx->set_output(0, var);
  }
};
REGISTER_KERNEL_BUILDER(Name("ApplyAdam").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuApplyAdamOp);

}  // namespace
}  // namespace stf
