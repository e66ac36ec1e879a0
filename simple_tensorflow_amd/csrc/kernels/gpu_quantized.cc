// GPU OpKernels: the quantized family (QuantizeV2, Dequantize,
// QuantizedMatMul, QuantizedConv2D, QuantizedRelu, RequantizationRange,
// QuantizeDownAndShrinkRange, Requantize, QuantizedBiasAdd,
// QuantizedMaxPool, QuantizedAvgPool, QuantizedRelu6, QuantizedConcat) on
// kernels/hip/gemm_i8.hip and kernels/hip/quantized.hip.
//
// The min/max ranges live in device memory on both sides of every op: only
// QuantizedConcat's axis is in host memory and nothing here reads a range
// value. The kernels derive zero points and steps from the device scalars
// and write the output ranges themselves, so a chain of quantized layers has
// no device-to-host sync and replays inside a captured step. The shape checks
// shared with kernels/cpu_quantized.cc are in kernels/quantized_shapes.h.
#include "kernels/gpu_common.h"
#include "kernels/quantized_shapes.h"

namespace stf {
namespace {

const float* F32(const Tensor& t) { return (const float*)t.raw_data(); }

float* ScalarOut(OpKernelContext* ctx, int i) {
  return (float*)ctx->allocate_output(i, TensorShape({}))->raw_data();
}

int64_t RoundUp64(int64_t k) { return (k + 63) & ~int64_t(63); }

class GpuQuantizeV2Op : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    Tensor* out = ctx->allocate_output(0, in.shape());
    float* omn = ScalarOut(ctx, 1);
    float* omx = ScalarOut(ctx, 2);
    OP_HIP_OK(ctx, stf_quantize_v2(F32(in), F32(ctx->input(1)),
                                   F32(ctx->input(2)),
                                   (uint8_t*)out->raw_data(), omn, omx,
                                   in.NumElements(), GPU_STREAM(ctx)));
  }
};
REGISTER_KERNEL_BUILDER(Name("QuantizeV2").Device(DEVICE_GPU),
                        GpuQuantizeV2Op);

class GpuDequantizeOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    Tensor* out = ctx->allocate_output(0, in.shape());
    OP_HIP_OK(ctx, stf_dequantize(in.dtype() == DT_UINT8 ? 0 : 1,
                                  in.raw_data(), F32(ctx->input(1)),
                                  F32(ctx->input(2)),
                                  (float*)out->raw_data(), in.NumElements(),
                                  GPU_STREAM(ctx)));
  }
};
REGISTER_KERNEL_BUILDER(Name("Dequantize").Device(DEVICE_GPU),
                        GpuDequantizeOp);

// Packs a u8 operand for the i8 GEMM: element (row, k) at src[row * sr +
// k * sk] -> s8 [rows][K rounded up to 64]. With sums, also allocates and
// fills the [1 or 1 + taps][rows] int32 sums of the packed rows.
hipError_t Pack(OpKernelContext* ctx, const void* src, int64_t sr, int64_t sk,
                int64_t rows, int64_t K, int taps, Tensor* packed,
                Tensor* sums, hipStream_t s) {
  *packed = ctx->allocate_temp(DT_UINT8, TensorShape({rows, RoundUp64(K)}));
  int32_t* sp = nullptr;
  if (sums) {
    int64_t n = (taps > 1 ? 1 + taps : 1) * rows;
    *sums = ctx->allocate_temp(DT_INT32, TensorShape({n}));
    sp = (int32_t*)sums->raw_data();
    hipError_t e = hipMemsetAsync(sp, 0, n * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
  }
  return stf_pack_i8(src, sr, sk, rows, K, packed->raw_data(), sp, taps, s);
}

class GpuQuantizedMatMulOp : public OpKernel {
 public:
  explicit GpuQuantizedMatMulOp(OpKernelConstruction* c) : OpKernel(c) {
    c->GetAttr("transpose_a", &ta_);
    c->GetAttr("transpose_b", &tb_);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& a = ctx->input(0);
    const Tensor& b = ctx->input(1);
    hipStream_t s = GPU_STREAM(ctx);
    int64_t M, N, K;
    OP_REQUIRES_OK(ctx,
                   QuantMatMulDims(a.shape(), b.shape(), ta_, tb_, &M, &N, &K));
    Tensor* out = ctx->allocate_output(0, TensorShape({M, N}));
    float* omn = ScalarOut(ctx, 1);
    float* omx = ScalarOut(ctx, 2);
    // B -> [N][Kp] s8 with its column sums; stored [K,N] unless transpose_b
    Tensor bp, bsums;
    OP_HIP_OK(ctx, Pack(ctx, b.raw_data(), tb_ ? K : 1, tb_ ? 1 : N, N, K, 1,
                        &bp, &bsums, s));
    // A is staged straight from the u8 matrix when its rows are k-contiguous
    // and 16-byte aligned; otherwise it goes through the packer too.
    const void* ap = a.raw_data();
    Tensor a_packed;
    bool pack_a = ta_ || (K & 15) != 0;
    if (pack_a) {
      OP_HIP_OK(ctx, Pack(ctx, a.raw_data(), ta_ ? 1 : K, ta_ ? M : 1, M, K,
                          1, &a_packed, nullptr, s));
      ap = a_packed.raw_data();
    }
    OP_HIP_OK(ctx, stf_gemm_i8(ap, pack_a ? 1 : 0, bp.raw_data(),
                               (const int32_t*)bsums.raw_data(),
                               F32(ctx->input(2)), F32(ctx->input(3)),
                               F32(ctx->input(4)), F32(ctx->input(5)),
                               (int32_t*)out->raw_data(), omn, omx, M, N, K,
                               s));
  }

 private:
  bool ta_ = false, tb_ = false;
};
REGISTER_KERNEL_BUILDER(Name("QuantizedMatMul").Device(DEVICE_GPU),
                        GpuQuantizedMatMulOp);

class GpuQuantizedConv2DOp : public OpKernel {
 public:
  explicit GpuQuantizedConv2DOp(OpKernelConstruction* c)
      : OpKernel(c), attrs_(c) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    const Tensor& w = ctx->input(1);
    hipStream_t s = GPU_STREAM(ctx);
    ConvGeom cg;
    StfConvGeom g;
    OP_REQUIRES_OK(ctx, MakeConvGeom(x.shape(), w.shape(), attrs_, &cg, &g));
    Tensor* y = ctx->allocate_output(0,
                                     TensorShape({cg.N, cg.P, cg.Q, cg.K}));
    float* omn = ScalarOut(ctx, 1);
    float* omx = ScalarOut(ctx, 2);
    int64_t rsc = cg.RSC();
    // filter [rsc, cout] -> [cout][Kp] s8 with the per-tap sums
    Tensor wp, wsums;
    OP_HIP_OK(ctx, Pack(ctx, w.raw_data(), 1, g.cout, g.cout, rsc,
                        g.r * g.s, &wp, &wsums, s));
    const void* ap = x.raw_data();
    Tensor col;
    bool implicit = (g.c & 15) == 0;
    if (!implicit) {
      // small-channel stems: materialized s8 column matrix
      int64_t kp = RoundUp64(rsc);
      col = ctx->allocate_temp(DT_UINT8, TensorShape({cg.M(), kp}));
      OP_HIP_OK(ctx, stf_im2col_i8(x.raw_data(), col.raw_data(), &g, kp, s));
      ap = col.raw_data();
    }
    OP_HIP_OK(ctx, stf_conv2d_i8(ap, implicit ? 1 : 0, wp.raw_data(),
                                 (const int32_t*)wsums.raw_data(),
                                 F32(ctx->input(2)), F32(ctx->input(3)),
                                 F32(ctx->input(4)), F32(ctx->input(5)),
                                 (int32_t*)y->raw_data(), omn, omx, &g, s));
  }

 private:
  ConvAttrs attrs_;
};
REGISTER_KERNEL_BUILDER(Name("QuantizedConv2D").Device(DEVICE_GPU),
                        GpuQuantizedConv2DOp);

// QuantizedRelu and QuantizedRelu6: two entry points of one signature.
using QuantizedClampFn = hipError_t (*)(const uint8_t*, const float*,
                                       const float*, uint8_t*, float*,
                                       float*, int64_t, hipStream_t);

class GpuQuantizedClampOp : public OpKernel {
 public:
  GpuQuantizedClampOp(OpKernelConstruction* c, QuantizedClampFn fn)
      : OpKernel(c), fn_(fn) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    Tensor* out = ctx->allocate_output(0, in.shape());
    float* omn = ScalarOut(ctx, 1);
    float* omx = ScalarOut(ctx, 2);
    OP_HIP_OK(ctx, fn_((const uint8_t*)in.raw_data(), F32(ctx->input(1)),
                       F32(ctx->input(2)), (uint8_t*)out->raw_data(), omn,
                       omx, in.NumElements(), GPU_STREAM(ctx)));
  }

 private:
  QuantizedClampFn fn_;
};
class GpuQuantizedReluOp : public GpuQuantizedClampOp {
 public:
  explicit GpuQuantizedReluOp(OpKernelConstruction* c)
      : GpuQuantizedClampOp(c, stf_quantized_relu) {}
};
class GpuQuantizedRelu6Op : public GpuQuantizedClampOp {
 public:
  explicit GpuQuantizedRelu6Op(OpKernelConstruction* c)
      : GpuQuantizedClampOp(c, stf_quantized_relu6) {}
};
REGISTER_KERNEL_BUILDER(Name("QuantizedRelu").Device(DEVICE_GPU),
                        GpuQuantizedReluOp);
REGISTER_KERNEL_BUILDER(Name("QuantizedRelu6").Device(DEVICE_GPU),
                        GpuQuantizedRelu6Op);

class GpuRequantizationRangeOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    float* omn = ScalarOut(ctx, 0);
    float* omx = ScalarOut(ctx, 1);
    Tensor lohi = ctx->allocate_temp(DT_INT32, TensorShape({2}));
    OP_HIP_OK(ctx, stf_requantization_range(
                       (const int32_t*)in.raw_data(), F32(ctx->input(1)),
                       F32(ctx->input(2)), (int32_t*)lohi.raw_data(), omn,
                       omx, in.NumElements(), GPU_STREAM(ctx)));
  }
};
REGISTER_KERNEL_BUILDER(Name("RequantizationRange").Device(DEVICE_GPU),
                        GpuRequantizationRangeOp);

class GpuQuantizeDownAndShrinkRangeOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    Tensor* out = ctx->allocate_output(0, in.shape());
    float* omn = ScalarOut(ctx, 1);
    float* omx = ScalarOut(ctx, 2);
    Tensor lohi = ctx->allocate_temp(DT_INT32, TensorShape({2}));
    OP_HIP_OK(ctx, stf_quantize_down((const int32_t*)in.raw_data(),
                                     F32(ctx->input(1)), F32(ctx->input(2)),
                                     (int32_t*)lohi.raw_data(),
                                     (uint8_t*)out->raw_data(), omn, omx,
                                     in.NumElements(), GPU_STREAM(ctx)));
  }
};
REGISTER_KERNEL_BUILDER(Name("QuantizeDownAndShrinkRange").Device(DEVICE_GPU),
                        GpuQuantizeDownAndShrinkRangeOp);

class GpuRequantizeOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    Tensor* out = ctx->allocate_output(0, in.shape());
    float* omn = ScalarOut(ctx, 1);
    float* omx = ScalarOut(ctx, 2);
    OP_HIP_OK(ctx, stf_requantize((const int32_t*)in.raw_data(),
                                  F32(ctx->input(1)), F32(ctx->input(2)),
                                  F32(ctx->input(3)), F32(ctx->input(4)),
                                  (uint8_t*)out->raw_data(), omn, omx,
                                  in.NumElements(), GPU_STREAM(ctx)));
  }
};
REGISTER_KERNEL_BUILDER(Name("Requantize").Device(DEVICE_GPU),
                        GpuRequantizeOp);

class GpuQuantizedBiasAddOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    const Tensor& bias = ctx->input(1);
    int64_t rows, C;
    OP_REQUIRES_OK(ctx, QuantBiasAddDims(in.shape(), bias.shape(), &rows, &C));
    Tensor* out = ctx->allocate_output(0, in.shape());
    float* omn = ScalarOut(ctx, 1);
    float* omx = ScalarOut(ctx, 2);
    OP_HIP_OK(ctx, stf_quantized_bias_add(
                       (const uint8_t*)in.raw_data(),
                       (const uint8_t*)bias.raw_data(), F32(ctx->input(2)),
                       F32(ctx->input(3)), F32(ctx->input(4)),
                       F32(ctx->input(5)), (int32_t*)out->raw_data(), omn,
                       omx, rows, C, GPU_STREAM(ctx)));
  }
};
REGISTER_KERNEL_BUILDER(Name("QuantizedBiasAdd").Device(DEVICE_GPU),
                        GpuQuantizedBiasAddOp);

// QuantizedMaxPool and QuantizedAvgPool: the same attributes and geometry in
// front of two entry points of one signature.
using QuantizedPoolFn = hipError_t (*)(const uint8_t*, const float*,
                                       const float*, uint8_t*, float*,
                                       float*, const StfPoolGeom*,
                                       hipStream_t);

class GpuQuantizedPoolOp : public OpKernel {
 public:
  GpuQuantizedPoolOp(OpKernelConstruction* c, QuantizedPoolFn fn)
      : OpKernel(c), fn_(fn), attrs_(c) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    StfPoolGeom g;
    OP_REQUIRES_OK(ctx, MakePoolGeom(x.shape(), attrs_, &g));
    Tensor* y = ctx->allocate_output(0, TensorShape({g.N, g.P, g.Q, g.C}));
    float* omn = ScalarOut(ctx, 1);
    float* omx = ScalarOut(ctx, 2);
    OP_HIP_OK(ctx, fn_((const uint8_t*)x.raw_data(), F32(ctx->input(1)),
                       F32(ctx->input(2)), (uint8_t*)y->raw_data(), omn, omx,
                       &g, GPU_STREAM(ctx)));
  }

 private:
  QuantizedPoolFn fn_;
  PoolAttrs attrs_;
};
class GpuQuantizedMaxPoolOp : public GpuQuantizedPoolOp {
 public:
  explicit GpuQuantizedMaxPoolOp(OpKernelConstruction* c)
      : GpuQuantizedPoolOp(c, stf_quantized_max_pool) {}
};
class GpuQuantizedAvgPoolOp : public GpuQuantizedPoolOp {
 public:
  explicit GpuQuantizedAvgPoolOp(OpKernelConstruction* c)
      : GpuQuantizedPoolOp(c, stf_quantized_avg_pool) {}
};
REGISTER_KERNEL_BUILDER(Name("QuantizedMaxPool").Device(DEVICE_GPU),
                        GpuQuantizedMaxPoolOp);
REGISTER_KERNEL_BUILDER(Name("QuantizedAvgPool").Device(DEVICE_GPU),
                        GpuQuantizedAvgPoolOp);

// Only concat_dim is in host memory. The N range pairs stay on the device:
// a range pass over all chunks of kStfQuantConcatMax inputs leaves the
// output range in the two output scalars, then one copy launch per chunk
// reads it from there.
class GpuQuantizedConcatOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    QuantConcatPlan plan;
    OP_REQUIRES_OK(ctx, MakeQuantConcatPlan(ctx, num_inputs(), &plan));
    Tensor* y = ctx->allocate_output(0, plan.out_shape);
    float* omn = ScalarOut(ctx, 1);
    float* omx = ScalarOut(ctx, 2);
    hipStream_t s = GPU_STREAM(ctx);
    std::vector<StfQuantConcatArgs> chunks;
    for (int k = 0; k < plan.n; ++k) {
      if (k % kStfQuantConcatMax == 0) {
        chunks.emplace_back();
        chunks.back().n = 0;
      }
      StfQuantConcatArgs& a = chunks.back();
      int j = a.n++;
      a.src[j] = (const uint8_t*)ctx->input(plan.value(k)).raw_data();
      a.mn[j] = F32(ctx->input(plan.min(k)));
      a.mx[j] = F32(ctx->input(plan.max(k)));
      a.inner[j] = plan.row[k];
      a.off[j] = plan.off[k];
    }
    for (size_t c = 0; c < chunks.size(); ++c)
      OP_HIP_OK(ctx, stf_quantized_concat_range(&chunks[c], c == 0, omn, omx,
                                                s));
    for (size_t c = 0; c < chunks.size(); ++c)
      OP_HIP_OK(ctx, stf_quantized_concat_copy(&chunks[c], omn, omx,
                                               (uint8_t*)y->raw_data(),
                                               plan.outer, plan.out_row, s));
  }
};
REGISTER_KERNEL_BUILDER(
    Name("QuantizedConcat").Device(DEVICE_GPU).HostMemory("concat_dim"),
    GpuQuantizedConcatOp);

// QuantizedReshape moves no data: its one kernel class is registered for
// both devices in kernels/cpu_quantized.cc, as Reshape's is in cpu_basic.cc.

}  // namespace
}  // namespace stf
