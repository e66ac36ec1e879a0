// GPU OpKernels: MatMul, BatchMatMul.
#include "kernels/gpu_common.h"

namespace stf {
namespace {

// ---------------------------------------------------------------------------
// MatMul (MFMA GEMM + pre-transposes to NT form)
// ---------------------------------------------------------------------------
class GpuMatMulOp : public OpKernel {
 public:
  explicit GpuMatMulOp(OpKernelConstruction* c) : OpKernel(c) {
    c->GetAttr("transpose_a", &ta_);
    c->GetAttr("transpose_b", &tb_);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& a = ctx->input(0);
    const Tensor& b = ctx->input(1);
    hipStream_t s = GPU_STREAM(ctx);
    int64_t m = ta_ ? a.dim_size(1) : a.dim_size(0);
    int64_t k = ta_ ? a.dim_size(0) : a.dim_size(1);
    int64_t n = tb_ ? b.dim_size(0) : b.dim_size(1);
    Tensor* y = ctx->allocate_output(0, TensorShape({m, n}));
    size_t es = DataTypeSize(a.dtype());
    if (a.dtype() == DT_BFLOAT16) {
      // The bf16 GEMM stages either operand layout directly (K-major
      // staging for transposed sides). A row stride that is no multiple of
      // 8 takes a pre-transpose first, which keeps the 16B global loads of
      // the K-major staging aligned. The result does not depend on it:
      // global loads need no alignment beyond the element (BatchMatMul
      // below hands over such strides as they are, and is tested bit for
      // bit there); the fallback stays because removing it has not been
      // timed.
      const void* ap = a.raw_data();
      const void* bp = b.raw_data();
      int a_km = ta_ ? 1 : 0;
      int64_t lda = a.dim_size(1);
      Tensor a_tmp;
      if (ta_ && (m & 7) != 0) {
        a_tmp = ctx->allocate_temp(a.dtype(), TensorShape({m, k}));
        OP_HIP_OK(ctx, stf_transpose2d((int)es, a.raw_data(),
                                       a_tmp.raw_data(), a.dim_size(0),
                                       a.dim_size(1), s));
        ap = a_tmp.raw_data();
        a_km = 0;
        lda = k;
      }
      int b_km = tb_ ? 0 : 1;
      int64_t ldb = b.dim_size(1);
      Tensor b_tmp;
      if (!tb_ && (n & 7) != 0) {
        b_tmp = ctx->allocate_temp(b.dtype(), TensorShape({n, k}));
        OP_HIP_OK(ctx, stf_transpose2d((int)es, b.raw_data(),
                                       b_tmp.raw_data(), b.dim_size(0),
                                       b.dim_size(1), s));
        bp = b_tmp.raw_data();
        b_km = 0;
        ldb = k;
      }
      OP_HIP_OK(ctx, GemmBf16AutoEx(ctx, ap, bp, y->raw_data(), m, n, k, lda,
                                    ldb, a_km, b_km, s));
    } else {
      // A effective [M,K]
      Tensor a_eff = a;
      if (ta_) {
        a_eff = ctx->allocate_temp(a.dtype(), TensorShape({m, k}));
        OP_HIP_OK(ctx, stf_transpose2d((int)es, a.raw_data(),
                                       a_eff.raw_data(), a.dim_size(0),
                                       a.dim_size(1), s));
      }
      // B effective [N,K]
      Tensor b_eff = b;
      if (!tb_) {
        b_eff = ctx->allocate_temp(b.dtype(), TensorShape({n, k}));
        OP_HIP_OK(ctx, stf_transpose2d((int)es, b.raw_data(),
                                       b_eff.raw_data(), b.dim_size(0),
                                       b.dim_size(1), s));
      }
      OP_HIP_OK(ctx, stf_gemm_f32_nt(a_eff.raw_data(), b_eff.raw_data(),
                                     y->raw_data(), m, n, k, s));
    }
  }

 private:
  bool ta_ = false, tb_ = false;
};
REGISTER_KERNEL_BUILDER(Name("MatMul").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuMatMulOp);
REGISTER_KERNEL_BUILDER(Name("MatMul").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuMatMulOp);

// BatchMatMul on GPU: per-batch MFMA GEMM launches with offset pointers
// (reference batch_matmul_op_impl.h:350 ThenBlasGemmBatchedWithScratch).
// The adj flags map onto the GEMM's contraction-major staging the same way
// MatMul's transpose flags do, so no transpose kernels are launched.
class GpuBatchMatMulOp : public OpKernel {
 public:
  explicit GpuBatchMatMulOp(OpKernelConstruction* c) : OpKernel(c) {
    c->GetAttr("adj_x", &ta_);
    c->GetAttr("adj_y", &tb_);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& a = ctx->input(0);
    const Tensor& b = ctx->input(1);
    hipStream_t s = GPU_STREAM(ctx);
    int ra = a.dims(), rb = b.dims();
    OP_REQUIRES(ctx, ra >= 2 && rb == ra,
                errors::InvalidArgument("BatchMatMul rank mismatch"));
    int64_t m = ta_ ? a.dim_size(ra - 1) : a.dim_size(ra - 2);
    int64_t k = ta_ ? a.dim_size(ra - 2) : a.dim_size(ra - 1);
    int64_t n = tb_ ? b.dim_size(rb - 2) : b.dim_size(rb - 1);
    int64_t kb = tb_ ? b.dim_size(rb - 1) : b.dim_size(rb - 2);
    OP_REQUIRES(ctx, k == kb,
                errors::InvalidArgument("BatchMatMul inner dim mismatch"));
    int64_t batch = 1;
    TensorShape out_shape;
    for (int i = 0; i < ra - 2; ++i) {
      batch *= a.dim_size(i);
      out_shape.AddDim(a.dim_size(i));
    }
    out_shape.AddDim(m);
    out_shape.AddDim(n);
    Tensor* y = ctx->allocate_output(0, out_shape);
    int64_t sa = m * k, sb = k * n, sc = m * n;
    if (a.dtype() == DT_BFLOAT16) {
      // adj_x: A [K,M] contraction-major -> a_km; plain B [K,N] -> b_km.
      int a_km = ta_ ? 1 : 0;
      int b_km = tb_ ? 0 : 1;
      int64_t lda = a.dim_size(ra - 1);
      int64_t ldb = b.dim_size(rb - 1);
      const uint16_t* ap = (const uint16_t*)a.raw_data();
      const uint16_t* bp = (const uint16_t*)b.raw_data();
      uint16_t* yp = (uint16_t*)y->raw_data();
      for (int64_t i = 0; i < batch; ++i) {
        OP_HIP_OK(ctx, stf_gemm_bf16(ap + i * sa, bp + i * sb, yp + i * sc, m,
                                     n, k, lda, ldb, a_km, b_km, s));
      }
    } else {
      // f32 path: pre-transpose per batch when adjoint flags are set.
      Tensor a_eff = a, b_eff = b;
      const float* ap = (const float*)a.raw_data();
      const float* bp = (const float*)b.raw_data();
      if (ta_) {
        a_eff = ctx->allocate_temp(DT_FLOAT, TensorShape({batch, m, k}));
        for (int64_t i = 0; i < batch; ++i)
          OP_HIP_OK(ctx, stf_transpose2d(4, ap + i * sa,
                                         (float*)a_eff.raw_data() + i * sa,
                                         k, m, s));
        ap = (const float*)a_eff.raw_data();
      }
      // GEMM f32 wants B as [N, K] (NT): transpose unless adj_y.
      if (!tb_) {
        b_eff = ctx->allocate_temp(DT_FLOAT, TensorShape({batch, n, k}));
        for (int64_t i = 0; i < batch; ++i)
          OP_HIP_OK(ctx, stf_transpose2d(4, bp + i * sb,
                                         (float*)b_eff.raw_data() + i * sb,
                                         k, n, s));
        bp = (const float*)b_eff.raw_data();
      }
      float* yp = (float*)y->raw_data();
      for (int64_t i = 0; i < batch; ++i)
        OP_HIP_OK(ctx, stf_gemm_f32_nt(ap + i * sa, bp + i * sb, yp + i * sc,
                                       m, n, k, s));
    }
  }

 private:
  bool ta_ = false, tb_ = false;
};
REGISTER_KERNEL_BUILDER(Name("BatchMatMul").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuBatchMatMulOp);
REGISTER_KERNEL_BUILDER(Name("BatchMatMul").Device(DEVICE_GPU).TypeConstraint<float>("T"), GpuBatchMatMulOp);

}  // namespace
}  // namespace stf
