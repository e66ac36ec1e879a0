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

// _MultiApplyMomentum (graph/optimizer.cc FuseApplyMomentum): N ApplyMomentum
// updates in as few launches as the kernel's tables allow. Inputs: vars
// [0, N), accums [N, 2N), lr 2N, grads [2N+1, 3N+1), momentum 3N+1.
class GpuMultiApplyMomentumOp : public OpKernel {
 public:
  explicit GpuMultiApplyMomentumOp(OpKernelConstruction* c) : OpKernel(c) {
    int64_t n = 0;
    c->GetAttr("N", &n);
    n_ = (int)n;
    c->GetAttr("use_nesterov", &nesterov_);
  }
  void Compute(OpKernelContext* ctx) override {
    const int n = n_;
    OP_REQUIRES(ctx, ctx->num_inputs() == 3 * n + 2,
                errors::InvalidArgument("_MultiApplyMomentum: ", 3 * n + 2,
                                        " inputs expected"));
    const DataType gt = ctx->input(2 * n + 1).dtype();
    std::vector<void*> vars(n), accums(n);
    std::vector<const void*> grads(n);
    std::vector<int64_t> sizes(n);
    for (int i = 0; i < n; ++i) {
      Tensor var = ctx->input(i);
      Tensor accum = ctx->input(n + i);
      const Tensor& grad = ctx->input(2 * n + 1 + i);
      OP_REQUIRES(ctx,
                  var.dtype() == DT_FLOAT && accum.dtype() == DT_FLOAT &&
                      grad.dtype() == gt,
                  errors::InvalidArgument("_MultiApplyMomentum: dtype of ",
                                          "variable ", i));
      OP_REQUIRES(ctx,
                  var.shape() == accum.shape() && var.shape() == grad.shape(),
                  errors::InvalidArgument("_MultiApplyMomentum: var, accum ",
                                          "and grad shapes differ at ", i));
      vars[i] = var.raw_data();
      accums[i] = accum.raw_data();
      grads[i] = grad.raw_data();
      sizes[i] = var.NumElements();
    }
    OP_HIP_OK(ctx, stf_multi_apply_momentum(
                       gt == DT_BFLOAT16, n, vars.data(), accums.data(),
                       grads.data(), sizes.data(),
                       ctx->input(2 * n).raw_data(),
                       ctx->input(3 * n + 1).raw_data(), nesterov_,
                       GPU_STREAM(ctx)));
  }

 private:
  int n_ = 0;
  bool nesterov_ = false;
};
REGISTER_KERNEL_BUILDER(Name("_MultiApplyMomentum").Device(DEVICE_GPU).TypeConstraint<float>("G"), GpuMultiApplyMomentumOp);
REGISTER_KERNEL_BUILDER(Name("_MultiApplyMomentum").Device(DEVICE_GPU).TypeConstraint<bfloat16>("G"), GpuMultiApplyMomentumOp);

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
