// GPU OpKernels: the Conv2D family and depthwise conv.
#include "kernels/gpu_common.h"

namespace stf {
namespace {

// ---------------------------------------------------------------------------
// Conv2D family (implicit-GEMM, or im2col + MFMA GEMM)
// ---------------------------------------------------------------------------
// Implicit-GEMM conv (the reference's cuDNN implicit-GEMM slot,
// conv_ops.cc:664): the column matrix is generated inside the GEMM's A
// staging — no im2col kernel, no column buffer. STF_NO_IMPLICIT_CONV
// (debug) forces the materialized-im2col paths instead.
static bool ImplicitConvEnabled() {
  static const bool enabled = getenv("STF_NO_IMPLICIT_CONV") == nullptr;
  return enabled;
}

// The implicit paths read 8-channel (16B) runs, so the C=3 stem is run on a
// copy of x zero-padded to C8 = 8 channels (the padded channels contribute
// nothing). Writes the copy to *xp and sets the channels of *g and *sg to C8.
static hipError_t PadChannels(OpKernelContext* ctx, const Tensor& x,
                              ConvGeom* g, StfConvGeom* sg, Tensor* xp,
                              hipStream_t s) {
  int64_t c8 = (g->C + 7) & ~7ll;
  *xp = ctx->allocate_temp(DT_BFLOAT16, TensorShape({g->N, g->H, g->W, c8}));
  hipError_t e = stf_block_pad(1, x.raw_data(), xp->raw_data(),
                               g->N * g->H * g->W, g->C, c8, s);
  g->C = c8;
  sg->c = (int)c8;
  return e;
}

// Materialized column matrix col[M, ld] (ld >= RSC; the tail is zeroed).
static hipError_t Im2Col(OpKernelContext* ctx, const Tensor& x,
                         const ConvGeom& g, const StfConvGeom& sg, int64_t ld,
                         Tensor* col, hipStream_t s) {
  *col = ctx->allocate_temp(DT_BFLOAT16, TensorShape({g.M(), ld}));
  if (ld != g.RSC()) {
    hipError_t e = hipMemsetAsync(col->raw_data(), 0, g.M() * ld * 2, s);
    if (e != hipSuccess) return e;
  }
  return stf_im2col_bf16(x.raw_data(), col->raw_data(), &sg, ld, s);
}

// dst[cols, rows] = src[rows, cols]^T into a fresh bf16 temp.
static hipError_t TransposeBf16(OpKernelContext* ctx, const void* src,
                                int64_t rows, int64_t cols, Tensor* dst,
                                hipStream_t s) {
  *dst = ctx->allocate_temp(DT_BFLOAT16, TensorShape({cols, rows}));
  return stf_transpose2d(2, src, dst->raw_data(), rows, cols, s);
}

// Also _Conv2DBnStats (stats): the same conv, plus output 1 = float[2K], the
// per-output-channel sum and sum of squares of the bf16 y, for the batch norm
// that follows. On the 8-phase paths they come out of the GEMM epilogue;
// every other path runs the conv as for Conv2D and then reads y once.
class GpuConv2DOp : public OpKernel {
 public:
  explicit GpuConv2DOp(OpKernelConstruction* c, bool stats = false)
      : OpKernel(c), stats_(stats), attrs_(c) {}
  void Compute(OpKernelContext* ctx) override {
    hipStream_t s = GPU_STREAM(ctx);
    // ---- geometry ----
    Tensor x = ctx->input(0);
    Tensor w = ctx->input(1);
    ConvGeom g;
    StfConvGeom sg;
    OP_REQUIRES_OK(ctx, MakeConvGeom(x.shape(), w.shape(), attrs_, &g, &sg));
    Tensor* y = ctx->allocate_output(0, TensorShape({g.N, g.P, g.Q, g.K}));
    float* sums = nullptr;
    if (stats_) {
      sums = ctx->allocate_output(1, TensorShape({2 * g.K}))->flat<float>();
      OP_HIP_OK(ctx, ZeroF32(sums, 2 * g.K, s));
    }
    if (!g.is_1x1_s1() && (g.C % 8) != 0 && x.dtype() == DT_BFLOAT16) {
      // stem: pad the channels of x and of w (zero in both)
      int64_t c = g.C;
      Tensor xp, wp;
      OP_HIP_OK(ctx, PadChannels(ctx, x, &g, &sg, &xp, s));
      wp = ctx->allocate_temp(DT_BFLOAT16, TensorShape({g.RSC(), g.K}));
      OP_HIP_OK(ctx, stf_block_pad(1, w.raw_data(), wp.raw_data(), g.R * g.S,
                                   c * g.K, g.C * g.K, s));
      x = xp;
      w = wp;
    }
    int64_t rsc = g.RSC();
    // 1x1/s1 uses x directly as the GEMM A (ld = C) — no padding there.
    int64_t rscp = g.is_1x1_s1() ? rsc : g.RSCp();
    // weights stay [RSC(p), K] and are read contraction-major by the GEMM
    // (b_km staging). Zero-pad the RSC dim only when it is not 64-aligned
    // (conv1's 147 -> 192); rows [rsc, rscp) are zero, matching the
    // zero-padded columns.
    if (rscp != rsc) {
      Tensor wz = ctx->allocate_temp(DT_BFLOAT16, TensorShape({rscp, g.K}));
      OP_HIP_OK(ctx, hipMemsetAsync(wz.raw_data(), 0, rscp * g.K * 2, s));
      OP_HIP_OK(ctx, hipMemcpyAsync(wz.raw_data(), w.raw_data(),
                                    rsc * g.K * 2, hipMemcpyDeviceToDevice,
                                    s));
      w = wz;
    }

    // ---- pick the path ----
    bool fits_8ph = stf_gemm_bf16_8ph_ok(g.M(), g.K, rscp);
    bool implicit = ImplicitConvEnabled() && !g.is_1x1_s1() && (g.C % 8) == 0;
    enum { kImplicit8Ph, kImplicitNT, kIm2ColGemm } path =
        implicit && fits_8ph && ZeroPage()         ? kImplicit8Ph
        : implicit && (g.K & 7) == 0 && ZeroPage() ? kImplicitNT
                                                   : kIm2ColGemm;

    // ---- run it ----
    Tensor wt;  // [K, rscp], for the NT kernels
    // stats_ on an 8-phase path: the GEMM leaves partial[M/256][2][K] f32,
    // whose column sums are the statistics
    Tensor partial;
    float* pt = nullptr;
    auto sum_partials = [&]() {
      return stf_bn_partial_sums(pt, sums, g.M() / 256, (int)(2 * g.K), s);
    };
    if (path == kImplicit8Ph) {
      OP_HIP_OK(ctx, TransposeBf16(ctx, w.raw_data(), rscp, g.K, &wt, s));
      if (stats_) {
        pt = TilePartials(ctx, g, &partial);
        OP_HIP_OK(ctx, stf_conv2d_fwd_8ph_stats(x.raw_data(), wt.raw_data(),
                                                y->raw_data(), pt, ZeroPage(),
                                                &sg, rscp, s));
        OP_HIP_OK(ctx, sum_partials());
        return;
      }
      OP_HIP_OK(ctx, stf_conv2d_fwd_8ph(x.raw_data(), wt.raw_data(),
                                        y->raw_data(), ZeroPage(), &sg, rscp,
                                        s));
      return;
    }
    if (path == kImplicitNT) {
      // shapes the 8-phase kernel cannot take (e.g. Inception's
      // 48/96/288-cout convs)
      OP_HIP_OK(ctx, stf_conv2d_fwd_nt(x.raw_data(), w.raw_data(),
                                       y->raw_data(), ZeroPage(), &sg, rscp,
                                       s));
    } else {
      Tensor col = x;  // 1x1/s1: x is the column matrix
      if (!g.is_1x1_s1())
        OP_HIP_OK(ctx, Im2Col(ctx, x, g, sg, rscp, &col, s));
      if (!fits_8ph && (g.K & 7) == 0) {
        OP_HIP_OK(ctx, stf_gemm_bf16(col.raw_data(), w.raw_data(),
                                     y->raw_data(), g.M(), g.K, rscp, rscp,
                                     g.K, 0, 1, s));
      } else {
        // 8-phase-eligible shape (one small weight transpose buys the NT
        // fast path for the big M=NPQ GEMM), or a cout the K-major staging
        // cannot load 16B-aligned.
        OP_HIP_OK(ctx, TransposeBf16(ctx, w.raw_data(), rscp, g.K, &wt, s));
        // the gate under which stf_gemm_bf16_nt takes the 8-phase kernel
        if (stats_ && fits_8ph && getenv("STF_NO_8PH") == nullptr) {
          pt = TilePartials(ctx, g, &partial);
          OP_HIP_OK(ctx, stf_gemm_bf16_8ph_stats(col.raw_data(),
                                                 wt.raw_data(), y->raw_data(),
                                                 pt, g.M(), g.K, rscp, rscp,
                                                 rscp, s));
          OP_HIP_OK(ctx, sum_partials());
          return;
        }
        OP_HIP_OK(ctx, stf_gemm_bf16_nt(col.raw_data(), wt.raw_data(),
                                        y->raw_data(), g.M(), g.K, rscp, s));
      }
    }
    // every other path: one read of y, as BatchNormMi would do
    if (stats_)
      OP_HIP_OK(ctx, stf_bn_sums(1, y->raw_data(), sums, g.M(), (int)g.K, s));
  }

 private:
  static float* TilePartials(OpKernelContext* ctx, const ConvGeom& g,
                             Tensor* t) {
    *t = ctx->allocate_temp(DT_FLOAT, TensorShape({g.M() / 256, 2 * g.K}));
    return t->flat<float>();
  }

  bool stats_;
  ConvAttrs attrs_;
};
REGISTER_KERNEL_BUILDER(Name("Conv2D").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuConv2DOp);

class GpuConv2DBnStatsOp : public GpuConv2DOp {
 public:
  explicit GpuConv2DBnStatsOp(OpKernelConstruction* c)
      : GpuConv2DOp(c, true) {}
};
REGISTER_KERNEL_BUILDER(Name("_Conv2DBnStats").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuConv2DBnStatsOp);

class GpuConv2DBackpropInputOp : public OpKernel {
 public:
  explicit GpuConv2DBackpropInputOp(OpKernelConstruction* c, bool side = false)
      : OpKernel(c), attrs_(c), side_(side) {
    // STF_NO_IMPLICIT_DX (A/B runs) sends every dx back through GEMM +
    // col2im. Read per kernel, so a new graph sees a changed setting.
    implicit_dx_ = getenv("STF_NO_IMPLICIT_DX") == nullptr;
  }
  void Compute(OpKernelContext* ctx) override {
    auto in_sizes = IntVector(ctx->input(0));
    const Tensor& w = ctx->input(1);
    const Tensor& dy = ctx->input(2);
    hipStream_t s = GPU_STREAM(ctx);
    TensorShape x_shape(in_sizes);
    ConvGeom g;
    StfConvGeom sg;
    OP_REQUIRES_OK(ctx, MakeConvGeom(x_shape, w.shape(), attrs_, &g, &sg));
    Tensor* dx = ctx->allocate_output(0, x_shape);
    const void* side = nullptr;
    if (side_) {
      const Tensor& sd = ctx->input(3);
      OP_REQUIRES(ctx, sd.NumElements() == dx->NumElements(),
                  errors::InvalidArgument(
                      "Conv2DBackpropInputAdd: side shape mismatch"));
      side = sd.raw_data();
    }
    // dcol[M, RSC] = dy[M, K] x w[RSC, K]^T  (filter layout is already NT B)
    if (g.is_1x1_s1() && side && stf_gemm_bf16_8ph_ok(g.M(), g.RSC(), g.K)) {
      // residual-gradient accumulation fused into the GEMM epilogue: the
      // separate full-tensor add pass (and its 3x-bandwidth cost) vanishes
      OP_HIP_OK(ctx, stf_gemm_bf16_8ph_side(dy.raw_data(), w.raw_data(),
                                            dx->raw_data(), side, g.M(),
                                            g.RSC(), g.K, g.K, g.K, s));
      return;
    }
    // Stride 1: dx is itself a stride-1 convolution of dy with the flipped,
    // channel-swapped filter, so it runs on the implicit-GEMM 8-phase kernel
    // and the R*S-times-wider dcol is never written or read back. Shapes
    // outside the 8-phase gate keep GEMM + col2im: through the general NT
    // template the implicit dx measured 3% slower end to end on Inception v3.
    int64_t nhw = g.N * g.H * g.W;
    int64_t rskp = (g.R * g.S * g.K + 63) & ~int64_t(63);
    bool implicit = implicit_dx_ && g.sh == 1 && g.sw == 1 &&
                    !g.is_1x1_s1() && (g.K % 8) == 0 && ZeroPage();
    if (implicit && stf_gemm_bf16_8ph_ok(nhw, g.C, rskp)) {
      Tensor wt = ctx->allocate_temp(DT_BFLOAT16, TensorShape({g.C, rskp}));
      OP_HIP_OK(ctx, stf_conv_dx_filter(w.raw_data(), wt.raw_data(), (int)g.R,
                                        (int)g.S, (int)g.C, g.K, rskp, s));
      OP_HIP_OK(ctx, stf_conv2d_dx_8ph(dy.raw_data(), wt.raw_data(),
                                       dx->raw_data(), side, ZeroPage(), &sg,
                                       rskp, s));
      return;
    }
    if (g.is_1x1_s1()) {
      OP_HIP_OK(ctx, stf_gemm_bf16_nt(dy.raw_data(), w.raw_data(),
                                      dx->raw_data(), g.M(), g.RSC(), g.K, s));
    } else {
      Tensor dcol = ctx->allocate_temp(DT_BFLOAT16,
                                       TensorShape({g.M(), g.RSC()}));
      OP_HIP_OK(ctx, stf_gemm_bf16_nt(dy.raw_data(), w.raw_data(),
                                      dcol.raw_data(), g.M(), g.RSC(), g.K,
                                      s));
      // col2im writes every dx element once and takes side in that store
      OP_HIP_OK(ctx, stf_col2im_bf16(dcol.raw_data(), side, dx->raw_data(),
                                     &sg, s));
      return;
    }
    if (side)  // 1x1/s1 outside the 8-phase gate
      OP_HIP_OK(ctx, stf_binary(B_ADD, DtypeCode(DT_BFLOAT16), dx->raw_data(),
                                side, dx->raw_data(), dx->NumElements(), s));
  }

 private:
  ConvAttrs attrs_;
  bool side_;
  bool implicit_dx_;
};
REGISTER_KERNEL_BUILDER(Name("Conv2DBackpropInput").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T").HostMemory("input_sizes"), GpuConv2DBackpropInputOp);

class GpuConv2DBackpropInputAddOp : public GpuConv2DBackpropInputOp {
 public:
  explicit GpuConv2DBackpropInputAddOp(OpKernelConstruction* c)
      : GpuConv2DBackpropInputOp(c, true) {}
};
REGISTER_KERNEL_BUILDER(Name("Conv2DBackpropInputAdd").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T").HostMemory("input_sizes"), GpuConv2DBackpropInputAddOp);

// dW[RSC, K] = col[M, RSC]^T x dy[M, K], contraction over the output pixels.
class GpuConv2DBackpropFilterOp : public OpKernel {
 public:
  explicit GpuConv2DBackpropFilterOp(OpKernelConstruction* c)
      : OpKernel(c), attrs_(c) {}
  void Compute(OpKernelContext* ctx) override {
    hipStream_t s = GPU_STREAM(ctx);
    // ---- geometry ----
    const Tensor& x = ctx->input(0);
    auto f_sizes = IntVector(ctx->input(1));
    const Tensor& dy = ctx->input(2);
    TensorShape f_shape(f_sizes);
    ConvGeom g;
    StfConvGeom sg;
    OP_REQUIRES_OK(ctx, MakeConvGeom(x.shape(), f_shape, attrs_, &g, &sg));
    Tensor* dw = ctx->allocate_output(0, f_shape);
    int64_t rsc = g.RSC();

    // ---- pick the path ----
    // kImplicit: column matrix generated inside the K-major A staging.
    // kKMajorGemm: both operands are contraction (M-)major as stored, so
    //   the GEMM's K-major staging reads them directly, no transposes.
    // kTransposeGemm: cout (or a 1x1's C) not a multiple of 8, which the
    //   K-major 16B loads need: transpose both operands to NT form.
    bool pad_c = (g.C % 8) != 0 && x.dtype() == DT_BFLOAT16;  // stem
    enum { kImplicit, kKMajorGemm, kTransposeGemm } path =
        ImplicitConvEnabled() && !g.is_1x1_s1() &&
                ((g.C % 8) == 0 || pad_c) && (g.K & 7) == 0 &&
                (g.M() & 63) == 0 && ZeroPage()
            ? kImplicit
        : (g.K & 7) == 0 && (!g.is_1x1_s1() || (g.C & 7) == 0)
            ? kKMajorGemm
            : kTransposeGemm;

    // ---- run it ----
    if (path == kImplicit) {
      // Stem: run at C8 on a channel-padded x into a [R*S*C8, K] temp, then
      // drop the padded filter rows (their gradient is exactly zero).
      ConvGeom gi = g;
      StfConvGeom si = sg;
      Tensor xp, dwp;
      const void* xdata = x.raw_data();
      void* out = dw->raw_data();
      if (pad_c) {
        OP_HIP_OK(ctx, PadChannels(ctx, x, &gi, &si, &xp, s));
        dwp = ctx->allocate_temp(DT_BFLOAT16, TensorShape({gi.RSC(), g.K}));
        xdata = xp.raw_data();
        out = dwp.raw_data();
      }
      int sk = PickSplitK(gi.RSC(), g.K, g.M());
      OP_HIP_OK(ctx, SplitKInto(ctx, gi.RSC() * g.K, [&](float* acc) {
        return stf_conv2d_dw_splitk(xdata, dy.raw_data(), acc, ZeroPage(),
                                    &si, sk, s);
      }, out));
      if (pad_c)
        OP_HIP_OK(ctx, stf_block_pad(1, dwp.raw_data(), dw->raw_data(),
                                     g.R * g.S, gi.C * g.K, g.C * g.K, s));
      return;
    }
    if (path == kKMajorGemm) {
      Tensor col = x;  // 1x1/s1: x is the column matrix, ld = C
      int64_t lda = g.C;
      if (!g.is_1x1_s1()) {
        lda = g.RSCp();
        OP_HIP_OK(ctx, Im2Col(ctx, x, g, sg, lda, &col, s));
      }
      OP_HIP_OK(ctx, GemmBf16AutoEx(ctx, col.raw_data(), dy.raw_data(),
                                    dw->raw_data(), rsc, g.K, g.M(), lda,
                                    g.K, 1, 1, s));
      return;
    }
    Tensor col = x, colT, dyT;
    if (!g.is_1x1_s1()) OP_HIP_OK(ctx, Im2Col(ctx, x, g, sg, rsc, &col, s));
    OP_HIP_OK(ctx, TransposeBf16(ctx, col.raw_data(), g.M(), rsc, &colT, s));
    OP_HIP_OK(ctx, TransposeBf16(ctx, dy.raw_data(), g.M(), g.K, &dyT, s));
    OP_HIP_OK(ctx, GemmBf16AutoEx(ctx, colT.raw_data(), dyT.raw_data(),
                                  dw->raw_data(), rsc, g.K, g.M(), g.M(),
                                  g.M(), 0, 0, s));
  }

 private:
  ConvAttrs attrs_;
};
REGISTER_KERNEL_BUILDER(Name("Conv2DBackpropFilter").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T").HostMemory("filter_sizes"), GpuConv2DBackpropFilterOp);

// ---------------------------------------------------------------------------
// depthwise conv (reference depthwise_conv_op_gpu.cu.cc family); g.K is the
// channel multiplier of the [R, S, C, mult] filter
// ---------------------------------------------------------------------------
class GpuDepthwiseConvOp : public OpKernel {
 public:
  explicit GpuDepthwiseConvOp(OpKernelConstruction* c)
      : OpKernel(c), attrs_(c) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    const Tensor& w = ctx->input(1);
    ConvGeom g;
    StfConvGeom sg;
    OP_REQUIRES_OK(ctx, MakeConvGeom(x.shape(), w.shape(), attrs_, &g, &sg));
    OP_REQUIRES_OK(ctx, FitInt(attrs_.op, {g.K}));  // passed as int mult
    Tensor* y = ctx->allocate_output(
        0, TensorShape({g.N, g.P, g.Q, g.C * g.K}));
    OP_HIP_OK(ctx, stf_depthwise_fwd(x.raw_data(), w.raw_data(), y->raw_data(),
                                     &sg, (int)g.K, GPU_STREAM(ctx)));
  }

 private:
  ConvAttrs attrs_;
};
REGISTER_KERNEL_BUILDER(Name("DepthwiseConv2dNative").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T"), GpuDepthwiseConvOp);

class GpuDepthwiseConvBackpropInputOp : public OpKernel {
 public:
  explicit GpuDepthwiseConvBackpropInputOp(OpKernelConstruction* c)
      : OpKernel(c), attrs_(c) {}
  void Compute(OpKernelContext* ctx) override {
    auto in_sizes = IntVector(ctx->input(0));
    const Tensor& w = ctx->input(1);
    const Tensor& dy = ctx->input(2);
    TensorShape x_shape(in_sizes);
    ConvGeom g;
    StfConvGeom sg;
    OP_REQUIRES_OK(ctx, MakeConvGeom(x_shape, w.shape(), attrs_, &g, &sg));
    OP_REQUIRES_OK(ctx, FitInt(attrs_.op, {g.K}));
    Tensor* dx = ctx->allocate_output(0, x_shape);
    OP_HIP_OK(ctx, stf_depthwise_bwd_input(dy.raw_data(), w.raw_data(),
                                           dx->raw_data(), &sg, (int)g.K,
                                           GPU_STREAM(ctx)));
  }

 private:
  ConvAttrs attrs_;
};
REGISTER_KERNEL_BUILDER(Name("DepthwiseConv2dNativeBackpropInput").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T").HostMemory("input_sizes"), GpuDepthwiseConvBackpropInputOp);

class GpuDepthwiseConvBackpropFilterOp : public OpKernel {
 public:
  explicit GpuDepthwiseConvBackpropFilterOp(OpKernelConstruction* c)
      : OpKernel(c), attrs_(c) {}
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    auto f_sizes = IntVector(ctx->input(1));
    const Tensor& dy = ctx->input(2);
    TensorShape f_shape(f_sizes);
    ConvGeom g;
    StfConvGeom sg;
    OP_REQUIRES_OK(ctx, MakeConvGeom(x.shape(), f_shape, attrs_, &g, &sg));
    OP_REQUIRES_OK(ctx, FitInt(attrs_.op, {g.K}));
    hipStream_t s = GPU_STREAM(ctx);
    Tensor* dw = ctx->allocate_output(0, f_shape);
    Tensor scratch = ctx->allocate_temp(
        DT_FLOAT, TensorShape({f_shape.num_elements()}));
    OP_HIP_OK(ctx, ZeroF32(scratch.raw_data(), f_shape.num_elements(), s));
    OP_HIP_OK(ctx, stf_depthwise_bwd_filter(x.raw_data(), dy.raw_data(),
                                            scratch.flat<float>(), &sg,
                                            (int)g.K, s));
    OP_HIP_OK(ctx, stf_cast(0, CastCode(dw->dtype()), scratch.raw_data(),
                            dw->raw_data(), f_shape.num_elements(), s));
  }

 private:
  ConvAttrs attrs_;
};
REGISTER_KERNEL_BUILDER(Name("DepthwiseConv2dNativeBackpropFilter").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T").HostMemory("filter_sizes"), GpuDepthwiseConvBackpropFilterOp);

}  // namespace
}  // namespace stf
