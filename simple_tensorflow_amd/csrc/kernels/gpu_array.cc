// GPU OpKernels: reduce, tile, transpose, concat/split/pack/unpack, gather,
// segment-sum, slice, random.
#include "kernels/gpu_common.h"

#include <mutex>

namespace stf {
namespace {

// Views t as [outer, mid, inner]: outer is the product of the dims before
// `begin`, inner the product of the dims from `end` on.
void OuterInner(const Tensor& t, int begin, int end, int64_t* outer,
                int64_t* inner) {
  *outer = *inner = 1;
  for (int i = 0; i < begin; ++i) *outer *= t.dim_size(i);
  for (int i = end; i < t.dims(); ++i) *inner *= t.dim_size(i);
}

// ---------------------------------------------------------------------------
// reductions: Sum / Mean / Max (all-axes, trailing-axes, or leading-axes)
// ---------------------------------------------------------------------------
class GpuReduceOp : public OpKernel {
 public:
  GpuReduceOp(OpKernelConstruction* c, StfReduce red, bool mean)
      : OpKernel(c), red_(red), mean_(mean) {
    c->GetAttr("keep_dims", &keep_dims_);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    auto axes_v = IntVector(ctx->input(1));
    int rank = x.dims();
    std::vector<bool> reduce(rank, false);
    for (auto a : axes_v) reduce[a < 0 ? a + rank : a] = true;
    hipStream_t s = GPU_STREAM(ctx);
    int dt = DtypeCode(x.dtype());
    TensorShape out_shape;
    int64_t count = 1;
    for (int i = 0; i < rank; ++i) {
      if (reduce[i]) {
        count *= x.dim_size(i);
        if (keep_dims_) out_shape.AddDim(1);
      } else {
        out_shape.AddDim(x.dim_size(i));
      }
    }
    int64_t out_n = out_shape.num_elements();
    if (axes_v.empty()) {
      // no reduction: reshape copy
      Tensor* out = ctx->allocate_output(0, out_shape);
      OP_HIP_OK(ctx, hipMemcpyAsync(out->raw_data(), x.raw_data(),
                                    x.TotalBytes(), hipMemcpyDeviceToDevice,
                                    s));
      return;
    }
    Tensor f32_out = ctx->allocate_temp(DT_FLOAT, TensorShape({out_n}));
    // classify
    bool all_red = count == x.NumElements();
    int first_keep = -1, last_red = -1, first_red = rank, contiguous = 1;
    for (int i = 0; i < rank; ++i) {
      if (reduce[i]) {
        if (i < first_red) first_red = i;
        last_red = i;
      }
    }
    bool trailing = last_red == rank - 1;
    bool leading = first_red == 0;
    for (int i = first_red; i <= last_red && i >= 0; ++i)
      if (!reduce[i]) contiguous = 0;
    if (all_red) {
      OP_HIP_OK(ctx, stf_fill_f32(f32_out.raw_data(), StfReduceIdentity(red_),
                                  1, 0, s));
      OP_HIP_OK(ctx, stf_full_reduce(dt, red_, x.raw_data(),
                                     f32_out.flat<float>(), x.NumElements(),
                                     s));
    } else if (trailing && contiguous) {
      OP_HIP_OK(ctx, stf_row_reduce(dt, red_, x.raw_data(),
                                    f32_out.flat<float>(), out_n, count, s));
    } else if (leading && contiguous) {
      OP_HIP_OK(ctx, stf_col_reduce(dt, red_, x.raw_data(),
                                    f32_out.flat<float>(), count, out_n, s));
    } else {
      OP_REQUIRES(ctx, false,
                  errors::Unimplemented(
                      "GPU reduce supports all/leading/trailing axes"));
    }
    if (mean_ && count > 0) {
      OP_HIP_OK(ctx, stf_scale(0, f32_out.raw_data(), f32_out.raw_data(),
                               out_n, 1.f / (float)count, s));
    }
    Tensor* out = ctx->allocate_output(0, out_shape);
    OP_HIP_OK(ctx, stf_cast(0, CastCode(out->dtype()), f32_out.raw_data(),
                            out->raw_data(), out_n, s));
  }

 private:
  StfReduce red_;
  bool mean_;
  bool keep_dims_ = false;
};
class SumGpu : public GpuReduceOp {
 public:
  explicit SumGpu(OpKernelConstruction* c)
      : GpuReduceOp(c, STF_REDUCE_SUM, false) {}
};
class MeanGpu : public GpuReduceOp {
 public:
  explicit MeanGpu(OpKernelConstruction* c)
      : GpuReduceOp(c, STF_REDUCE_SUM, true) {}
};
class MaxGpu : public GpuReduceOp {
 public:
  explicit MaxGpu(OpKernelConstruction* c)
      : GpuReduceOp(c, STF_REDUCE_MAX, false) {}
};
class MinGpu : public GpuReduceOp {
 public:
  explicit MinGpu(OpKernelConstruction* c)
      : GpuReduceOp(c, STF_REDUCE_MIN, false) {}
};
#define REG_GPU_REDUCE(OP, CLS)                                                \
  REGISTER_KERNEL_BUILDER(Name(OP).Device(DEVICE_GPU).TypeConstraint<float>("T").HostMemory("reduction_indices"), CLS); \
  REGISTER_KERNEL_BUILDER(Name(OP).Device(DEVICE_GPU).TypeConstraint<bfloat16>("T").HostMemory("reduction_indices"), CLS);
REG_GPU_REDUCE("Sum", SumGpu)
REG_GPU_REDUCE("Mean", MeanGpu)
REG_GPU_REDUCE("Max", MaxGpu)
REG_GPU_REDUCE("Min", MinGpu)
#undef REG_GPU_REDUCE

// ---------------------------------------------------------------------------
// Tile (broadcast only: tiled dims must have input size 1) + Transpose
// ---------------------------------------------------------------------------
class GpuTileOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    auto mult = IntVector(ctx->input(1));
    int rank = x.dims();
    OP_REQUIRES(ctx, rank <= kStfMaxPermuteRank,
                errors::Unimplemented("GPU Tile: rank above ",
                                      kStfMaxPermuteRank));
    TensorShape out_shape;
    std::vector<int64_t> strides(rank), dims(rank);
    int64_t s_acc = 1;
    for (int i = rank - 1; i >= 0; --i) {
      strides[i] = x.dim_size(i) == 1 ? 0 : s_acc;
      s_acc *= x.dim_size(i);
    }
    for (int i = 0; i < rank; ++i) {
      OP_REQUIRES(ctx, mult[i] == 1 || x.dim_size(i) == 1,
                  errors::Unimplemented("GPU Tile: only broadcast tiling"));
      dims[i] = x.dim_size(i) * mult[i];
      out_shape.AddDim(dims[i]);
    }
    Tensor* y = ctx->allocate_output(0, out_shape);
    // a permute whose source stride is 0 on the tiled dims: broadcast
    OP_HIP_OK(ctx, stf_permute((int)DataTypeSize(x.dtype()), x.raw_data(),
                               y->raw_data(), out_shape.num_elements(), rank,
                               dims.data(), strides.data(), GPU_STREAM(ctx)));
  }
};
REGISTER_KERNEL_BUILDER(Name("Tile").Device(DEVICE_GPU).HostMemory("multiples"), GpuTileOp);

class GpuTransposeOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& x = ctx->input(0);
    auto perm = IntVector(ctx->input(1));
    int rank = x.dims();
    OP_REQUIRES(ctx, rank <= kStfMaxPermuteRank,
                errors::Unimplemented("GPU Transpose: rank above ",
                                      kStfMaxPermuteRank));
    TensorShape out_shape;
    std::vector<int64_t> in_strides(rank, 1), src_strides(rank), dims(rank);
    for (int i = rank - 2; i >= 0; --i)
      in_strides[i] = in_strides[i + 1] * x.dim_size(i + 1);
    for (int i = 0; i < rank; ++i) {
      dims[i] = x.dim_size((int)perm[i]);
      src_strides[i] = in_strides[(int)perm[i]];
      out_shape.AddDim(dims[i]);
    }
    Tensor* y = ctx->allocate_output(0, out_shape);
    if (rank == 2 && perm[0] == 1) {
      OP_HIP_OK(ctx, stf_transpose2d((int)DataTypeSize(x.dtype()),
                                     x.raw_data(), y->raw_data(),
                                     x.dim_size(0), x.dim_size(1),
                                     GPU_STREAM(ctx)));
      return;
    }
    OP_HIP_OK(ctx, stf_permute((int)DataTypeSize(x.dtype()), x.raw_data(),
                               y->raw_data(), out_shape.num_elements(), rank,
                               dims.data(), src_strides.data(),
                               GPU_STREAM(ctx)));
  }
};
REGISTER_KERNEL_BUILDER(Name("Transpose").Device(DEVICE_GPU).HostMemory("perm"), GpuTransposeOp);

// ---------------------------------------------------------------------------
// random
// ---------------------------------------------------------------------------
class GpuRandomOp : public OpKernel {
 public:
  GpuRandomOp(OpKernelConstruction* c, int kind) : OpKernel(c), kind_(kind) {
    int64_t seed = 0, seed2 = 0;
    c->GetAttr("seed", &seed);
    c->GetAttr("seed2", &seed2);
    if (seed == 0 && seed2 == 0) seed = 0x9E3779B9;
    seed_ = ((uint64_t)seed << 32) | (uint32_t)seed2;
  }
  void Compute(OpKernelContext* ctx) override {
    auto dims = IntVector(ctx->input(0));
    Tensor* y = ctx->allocate_output(0, TensorShape(dims));
    int64_t n = y->NumElements();
    int bf16 = y->dtype() == DT_BFLOAT16;
    hipStream_t s = GPU_STREAM(ctx);
    {
      std::lock_guard<std::mutex> l(mu_);
      if (!ctr_.IsInitialized()) {
        // device-resident philox offset (advanced in-graph so hipGraph
        // replays still draw fresh numbers)
        ctr_ = Tensor(ctx->device()->allocator(), DT_INT64, TensorShape({1}));
        OP_HIP_OK(ctx, hipMemsetAsync(ctr_.raw_data(), 0, 8, s));
      }
    }
    if (kind_ == 0) {
      OP_HIP_OK(ctx, stf_random_uniform(seed_, ctr_.raw_data(), y->raw_data(),
                                        n, bf16, s));
    } else {
      OP_HIP_OK(ctx, stf_random_normal(seed_, ctr_.raw_data(), y->raw_data(),
                                       n, bf16, kind_ == 2, s));
    }
  }

 private:
  int kind_;
  uint64_t seed_;
  std::mutex mu_;
  Tensor ctr_;
};
class RandomUniformGpu : public GpuRandomOp {
 public:
  explicit RandomUniformGpu(OpKernelConstruction* c) : GpuRandomOp(c, 0) {}
};
class RandomNormalGpu : public GpuRandomOp {
 public:
  explicit RandomNormalGpu(OpKernelConstruction* c) : GpuRandomOp(c, 1) {}
};
class TruncatedNormalGpu : public GpuRandomOp {
 public:
  explicit TruncatedNormalGpu(OpKernelConstruction* c) : GpuRandomOp(c, 2) {}
};
REGISTER_KERNEL_BUILDER(Name("RandomUniform").Device(DEVICE_GPU).HostMemory("shape"), RandomUniformGpu);
REGISTER_KERNEL_BUILDER(Name("RandomStandardNormal").Device(DEVICE_GPU).HostMemory("shape"), RandomNormalGpu);
REGISTER_KERNEL_BUILDER(Name("TruncatedNormal").Device(DEVICE_GPU).HostMemory("shape"), TruncatedNormalGpu);

// ---------------------------------------------------------------------------
// concat / split / pack / unpack / gather / segment sum / slice
// ---------------------------------------------------------------------------
class GpuConcatV2Op : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    int n = num_inputs() - 1;
    int64_t axis = IntVector(ctx->input(n))[0];
    const Tensor& first = ctx->input(0);
    if (axis < 0) axis += first.dims();
    TensorShape out_shape = first.shape();
    int64_t total = 0;
    for (int k = 0; k < n; ++k) total += ctx->input(k).dim_size((int)axis);
    out_shape.set_dim((int)axis, total);
    Tensor* y = ctx->allocate_output(0, out_shape);
    int64_t outer, inner;
    OuterInner(first, (int)axis, (int)axis + 1, &outer, &inner);
    hipStream_t s = GPU_STREAM(ctx);
    int es = (int)DataTypeSize(first.dtype());
    int64_t off = 0;
    for (int k = 0; k < n; ++k) {
      const Tensor& t = ctx->input(k);
      int64_t rows = t.dim_size((int)axis);
      OP_HIP_OK(ctx, stf_strided_copy(es, 1, t.raw_data(), y->raw_data(),
                                      outer, rows, inner, total, off, s));
      off += rows;
    }
  }
};
REGISTER_KERNEL_BUILDER(Name("ConcatV2").Device(DEVICE_GPU).HostMemory("axis"), GpuConcatV2Op);

class GpuSplitOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    int64_t axis = IntVector(ctx->input(0))[0];
    const Tensor& in = ctx->input(1);
    if (axis < 0) axis += in.dims();
    int n = num_outputs();
    OP_REQUIRES(ctx, in.dim_size((int)axis) % n == 0,
                errors::InvalidArgument("Split axis not divisible"));
    int64_t part = in.dim_size((int)axis) / n;
    TensorShape out_shape = in.shape();
    out_shape.set_dim((int)axis, part);
    int64_t outer, inner;
    OuterInner(in, (int)axis, (int)axis + 1, &outer, &inner);
    hipStream_t s = GPU_STREAM(ctx);
    int es = (int)DataTypeSize(in.dtype());
    for (int k = 0; k < n; ++k) {
      Tensor* y = ctx->allocate_output(k, out_shape);
      OP_HIP_OK(ctx, stf_strided_copy(es, 0, in.raw_data(), y->raw_data(),
                                      outer, part, inner,
                                      in.dim_size((int)axis), k * part, s));
    }
  }
};
REGISTER_KERNEL_BUILDER(Name("Split").Device(DEVICE_GPU).HostMemory("split_dim"), GpuSplitOp);

class GpuPackOp : public OpKernel {
 public:
  explicit GpuPackOp(OpKernelConstruction* c) : OpKernel(c) {
    c->GetAttr("axis", &axis_);
  }
  void Compute(OpKernelContext* ctx) override {
    int n = num_inputs();
    const Tensor& first = ctx->input(0);
    int axis = axis_ < 0 ? (int)(axis_ + first.dims() + 1) : (int)axis_;
    TensorShape out_shape = first.shape();
    out_shape.InsertDim(axis, n);
    Tensor* y = ctx->allocate_output(0, out_shape);
    int64_t outer, inner;
    OuterInner(first, axis, axis, &outer, &inner);
    hipStream_t s = GPU_STREAM(ctx);
    int es = (int)DataTypeSize(first.dtype());
    for (int k = 0; k < n; ++k) {
      OP_HIP_OK(ctx, stf_strided_copy(es, 1, ctx->input(k).raw_data(),
                                      y->raw_data(), outer, 1, inner, n, k,
                                      s));
    }
  }

 private:
  int64_t axis_ = 0;
};
REGISTER_KERNEL_BUILDER(Name("Pack").Device(DEVICE_GPU), GpuPackOp);

class GpuUnpackOp : public OpKernel {
 public:
  explicit GpuUnpackOp(OpKernelConstruction* c) : OpKernel(c) {
    c->GetAttr("axis", &axis_);
  }
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    int axis = axis_ < 0 ? (int)(axis_ + in.dims()) : (int)axis_;
    int n = num_outputs();
    TensorShape out_shape = in.shape();
    out_shape.RemoveDim(axis);
    int64_t outer, inner;
    OuterInner(in, axis, axis + 1, &outer, &inner);
    hipStream_t s = GPU_STREAM(ctx);
    int es = (int)DataTypeSize(in.dtype());
    for (int k = 0; k < n; ++k) {
      Tensor* y = ctx->allocate_output(k, out_shape);
      OP_HIP_OK(ctx, stf_strided_copy(es, 0, in.raw_data(), y->raw_data(),
                                      outer, 1, inner, n, k, s));
    }
  }

 private:
  int64_t axis_ = 0;
};
REGISTER_KERNEL_BUILDER(Name("Unpack").Device(DEVICE_GPU), GpuUnpackOp);

class GpuGatherOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& params = ctx->input(0);
    const Tensor& idx = ctx->input(1);
    TensorShape out_shape = idx.shape();
    int64_t row = 1;
    for (int i = 1; i < params.dims(); ++i) {
      out_shape.AddDim(params.dim_size(i));
      row *= params.dim_size(i);
    }
    Tensor* y = ctx->allocate_output(0, out_shape);
    OP_HIP_OK(ctx, stf_gather_rows(DtypeCode(params.dtype()),
                                   idx.dtype() == DT_INT32, params.raw_data(),
                                   idx.raw_data(), y->raw_data(),
                                   idx.NumElements(), row, params.dim_size(0),
                                   GPU_STREAM(ctx)));
  }
};
REGISTER_KERNEL_BUILDER(Name("Gather").Device(DEVICE_GPU).TypeConstraint<float>("Tparams"), GpuGatherOp);
REGISTER_KERNEL_BUILDER(Name("Gather").Device(DEVICE_GPU).TypeConstraint<bfloat16>("Tparams"), GpuGatherOp);

class GpuUnsortedSegmentSumOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& data = ctx->input(0);
    const Tensor& ids = ctx->input(1);
    int64_t nseg = IntVector(ctx->input(2))[0];
    TensorShape out_shape({nseg});
    int64_t row = 1;
    for (int i = ids.dims(); i < data.dims(); ++i) {
      out_shape.AddDim(data.dim_size(i));
      row *= data.dim_size(i);
    }
    Tensor* y = ctx->allocate_output(0, out_shape);
    hipStream_t s = GPU_STREAM(ctx);
    Tensor scratch = ctx->allocate_temp(DT_FLOAT, TensorShape({nseg * row}));
    OP_HIP_OK(ctx, ZeroF32(scratch.raw_data(), nseg * row, s));
    OP_HIP_OK(ctx, stf_segment_sum(DtypeCode(data.dtype()),
                                   ids.dtype() == DT_INT32, data.raw_data(),
                                   ids.raw_data(), scratch.flat<float>(),
                                   ids.NumElements(), row, nseg, s));
    OP_HIP_OK(ctx, stf_cast(0, CastCode(y->dtype()), scratch.raw_data(),
                            y->raw_data(), nseg * row, s));
  }
};
REGISTER_KERNEL_BUILDER(Name("UnsortedSegmentSum").Device(DEVICE_GPU).TypeConstraint<float>("T").HostMemory("num_segments"), GpuUnsortedSegmentSumOp);
REGISTER_KERNEL_BUILDER(Name("UnsortedSegmentSum").Device(DEVICE_GPU).TypeConstraint<bfloat16>("T").HostMemory("num_segments"), GpuUnsortedSegmentSumOp);

// Slice on GPU (single sliced dim; degenerate = plain copy)
class GpuSliceOp : public OpKernel {
 public:
  using OpKernel::OpKernel;
  void Compute(OpKernelContext* ctx) override {
    const Tensor& in = ctx->input(0);
    auto begin = IntVector(ctx->input(1));
    auto size = IntVector(ctx->input(2));
    int rank = in.dims();
    for (int i = 0; i < rank; ++i)
      if (size[i] == -1) size[i] = in.dim_size(i) - begin[i];
    Tensor* y = ctx->allocate_output(0, TensorShape(size));
    int cut = -1;
    for (int i = 0; i < rank; ++i) {
      if (begin[i] != 0 || size[i] != in.dim_size(i)) {
        OP_REQUIRES(ctx, cut == -1,
                    errors::Unimplemented("GPU Slice: one sliced dim"));
        cut = i;
      }
    }
    hipStream_t s = GPU_STREAM(ctx);
    if (cut == -1) {
      OP_HIP_OK(ctx, hipMemcpyAsync(y->raw_data(), in.raw_data(),
                                    in.TotalBytes(), hipMemcpyDeviceToDevice,
                                    s));
      return;
    }
    int64_t outer, inner;
    OuterInner(in, cut, cut + 1, &outer, &inner);
    OP_HIP_OK(ctx, stf_strided_copy((int)DataTypeSize(in.dtype()), 0,
                                    in.raw_data(), y->raw_data(), outer,
                                    size[cut], inner, in.dim_size(cut),
                                    begin[cut], s));
  }
};
REGISTER_KERNEL_BUILDER(Name("Slice").Device(DEVICE_GPU).HostMemory("begin").HostMemory("size"), GpuSliceOp);

}  // namespace
}  // namespace stf
