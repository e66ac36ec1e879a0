// The C ABI between the host op layer (kernels/gpu_*.cc, rccl/rccl_ops.cc)
// and the HIP kernel files (kernels/hip/*.hip). Every extern "C" stf_* entry
// point is declared here exactly once; both the defining .hip file and every
// caller include this header, so a signature drift is a compile error instead
// of silently corrupted arguments at run time.
//
// Conventions: dtype codes are 0 = f32, 1 = bf16 (stf_cast: 0 f32, 1 bf16,
// 2 f16, 3 i32, 4 i64, 5 bool; no f16 kernel exists, so a pair with code 2,
// like any pair it does not list, returns hipErrorInvalidValue); all launches
// are asynchronous on `stream`.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

// Conv2D geometry, NHWC input / RSCK filter. p,q = output height/width.
struct StfConvGeom {
  int n, h, w, c;
  int r, s;
  int sh, sw, ph, pw;
  int p, q;
  int64_t cout;
};

// Pooling geometry, NHWC. P,Q = output height/width. Passed by value to the
// pooling kernels.
struct StfPoolGeom {
  int N, H, W, C, kh, kw, sh, sw, ph, pw, P, Q;
};

// Largest rank stf_permute takes.
constexpr int kStfMaxPermuteRank = 6;

// Reduction kinds of stf_full_reduce / stf_row_reduce / stf_col_reduce, and
// the value each kind starts from (stf_full_reduce expects out_f32 pre-filled
// with it).
enum StfReduce { STF_REDUCE_SUM = 0, STF_REDUCE_MAX = 1, STF_REDUCE_MIN = 2 };
constexpr float StfReduceIdentity(StfReduce kind) {
  return kind == STF_REDUCE_SUM ? 0.f
         : kind == STF_REDUCE_MAX ? -3.4e38f : 3.4e38f;
}

extern "C" {

// ---- gemm_bf16.hip / gemm_bf16_8ph.hip / gemm_f32.hip ----
// C[M,N] bf16 = A * B^T. a_km/b_km: operand stored contraction-major
// ([K,M] / [K,N]); lda/ldb are the row strides of the stored layouts.
hipError_t stf_gemm_bf16(const void* A, const void* B, void* C, int64_t M,
                         int64_t N, int64_t K, int64_t lda, int64_t ldb,
                         int a_km, int b_km, hipStream_t stream);
// NT shorthand: A [M,K], B [N,K], lda = ldb = K.
hipError_t stf_gemm_bf16_nt(const void* A, const void* B, void* C, int64_t M,
                            int64_t N, int64_t K, hipStream_t stream);
// Atomically accumulates into a pre-zeroed f32 C.
hipError_t stf_gemm_bf16_splitk(const void* A, const void* B, void* C_f32,
                                int64_t M, int64_t N, int64_t K, int64_t lda,
                                int64_t ldb, int a_km, int b_km, int splitk,
                                hipStream_t stream);
int stf_gemm_bf16_8ph_ok(int64_t M, int64_t N, int64_t K);
// 8-phase NT GEMM, bf16 out; side_bf16 (optional [M,N]) is added in the
// epilogue.
hipError_t stf_gemm_bf16_8ph_side(const void* A, const void* B, void* C,
                                  const void* side_bf16, int64_t M, int64_t N,
                                  int64_t K, int64_t lda, int64_t ldb,
                                  hipStream_t stream);
// 8-phase NT GEMM, bf16 out, that also writes each 256-row tile's column
// sums of the rounded C: partial[M/256][2][N] f32 ([t][0] = sum, [t][1] =
// sum of squares), every element written. stf_bn_partial_sums adds them up.
hipError_t stf_gemm_bf16_8ph_stats(const void* A, const void* B, void* C,
                                   float* partial, int64_t M, int64_t N,
                                   int64_t K, int64_t lda, int64_t ldb,
                                   hipStream_t stream);
hipError_t stf_gemm_f32_nt(const void* A, const void* B, void* C, int64_t M,
                           int64_t N, int64_t K, hipStream_t stream);

// ---- implicit-GEMM conv (gemm_bf16*.hip) and im2col (conv_im2col.hip) ----
// zero16: >= 16 zeroed device bytes (padding loads). rscp: K extent of the
// weight matrix (r*s*c rounded up to 64).
hipError_t stf_conv2d_fwd_8ph(const void* x, const void* wt, void* y,
                              const void* zero16, const StfConvGeom* g,
                              int64_t rscp, hipStream_t stream);
// stf_conv2d_fwd_8ph with the column sums of y, as stf_gemm_bf16_8ph_stats:
// partial[n*p*q/256][2][cout].
hipError_t stf_conv2d_fwd_8ph_stats(const void* x, const void* wt, void* y,
                                    float* partial, const void* zero16,
                                    const StfConvGeom* g, int64_t rscp,
                                    hipStream_t stream);
hipError_t stf_conv2d_fwd_nt(const void* x, const void* w, void* y,
                             const void* zero16, const StfConvGeom* g,
                             int64_t rscp, hipStream_t stream);
hipError_t stf_conv2d_dw_splitk(const void* x, const void* dy, void* dw_f32,
                                const void* zero16, const StfConvGeom* g,
                                int splitk, hipStream_t stream);
hipError_t stf_im2col_bf16(const void* x, void* col, const StfConvGeom* g,
                           int64_t ld, hipStream_t stream);
// dx = col2im(dcol) (+ side, optional [n,h,w,c] bf16, added after the sum is
// rounded to bf16).
hipError_t stf_col2im_bf16(const void* dcol, const void* side, void* dx,
                           const StfConvGeom* g, hipStream_t stream);
// Implicit-GEMM backward-input of a stride-1 conv: dx[NHW, C] = conv(dy,
// flipped filter), no column buffer. g is the forward geometry; k = cout must
// be a multiple of 8. The filter operand comes from stf_conv_dx_filter:
// w[r,s,c,k] -> wt[c][(r'*s + s')*k + kk] = w[r-1-r'][s-1-s'][c][kk], zero
// for columns in [r*s*k, rscp). rscp = r*s*k rounded up to 64.
hipError_t stf_conv_dx_filter(const void* w, void* wt, int r, int s, int c,
                              int64_t k, int64_t rscp, hipStream_t stream);
// side: optional [NHW, C] bf16 added in the epilogue. Needs
// stf_gemm_bf16_8ph_ok(NHW, c, rscp).
hipError_t stf_conv2d_dx_8ph(const void* dy, const void* wt, void* dx,
                             const void* side, const void* zero16,
                             const StfConvGeom* g, int64_t rscp,
                             hipStream_t stream);

// ---- gemm_i8.hip ----
// Quantized quint8 x quint8 -> qint32 on the i8 MFMA. Ranges are device f32
// scalars: zero points are derived on the device, min_out/max_out are
// written by the kernel. Operands reach the MFMA as s8 = u8 ^ 0x80, k
// contiguous, K rounded up to Kp = a multiple of 64 with a zero tail.
//
// Packs a u8 matrix whose element (row, k) is src[row * row_stride +
// k * k_stride] into dst_s8 [rows][Kp]. sums (optional, zeroed int32):
// [0][row] = sum over k of the packed row; with taps > 1 the buffer is
// [1 + taps][rows] and [1 + t][row] is the part of that sum in k-range
// [t * K/taps, (t+1) * K/taps).
hipError_t stf_pack_i8(const void* src_u8, int64_t row_stride,
                       int64_t k_stride, int64_t rows, int64_t K,
                       void* dst_s8, int32_t* sums, int taps,
                       hipStream_t stream);
// NHWC u8 image -> packed column matrix [n*p*q][kp], kp = r*s*c rounded up
// to 64; out-of-image taps are 0 in the s8 domain.
hipError_t stf_im2col_i8(const void* x_u8, void* col_s8, const StfConvGeom* g,
                         int64_t kp, hipStream_t stream);
// C[M,N] = sum_k (A - z_a)(B - z_b) mod 2^32. A: packed [M][Kp] (a_packed),
// or raw u8 [M][K] with K % 16 == 0. Bp: packed [N][Kp]; bsums: its sums.
hipError_t stf_gemm_i8(const void* A, int a_packed, const void* Bp,
                       const int32_t* bsums, const float* min_a,
                       const float* max_a, const float* min_b,
                       const float* max_b, int32_t* C, float* min_out,
                       float* max_out, int64_t M, int64_t N, int64_t K,
                       hipStream_t stream);
// Conv2D over the in-image taps only. implicit: x_or_col is the NHWC u8
// image (c % 16 == 0) and the column matrix is generated in staging; else
// it is the stf_im2col_i8 matrix. wp: the [r*s*c, cout] filter packed to
// [cout][Kp]; wsums: its sums with taps = r*s.
hipError_t stf_conv2d_i8(const void* x_or_col, int implicit, const void* wp,
                         const int32_t* wsums, const float* min_x,
                         const float* max_x, const float* min_w,
                         const float* max_w, int32_t* y, float* min_out,
                         float* max_out, const StfConvGeom* g,
                         hipStream_t stream);

// ---- quantized.hip ----
// Bit-equal to the CPU kernels (kernels/cpu_quantized.cc). Ranges are device
// f32 scalars in and out.
hipError_t stf_quantize_v2(const float* x, const float* mn, const float* mx,
                           uint8_t* y, float* out_mn, float* out_mx,
                           int64_t n, hipStream_t stream);
// in_i32: qint32 carrier, else quint8.
hipError_t stf_dequantize(int in_i32, const void* x, const float* mn,
                          const float* mx, float* y, int64_t n,
                          hipStream_t stream);
hipError_t stf_quantized_relu(const uint8_t* x, const float* mn,
                              const float* mx, uint8_t* y, float* out_mn,
                              float* out_mx, int64_t n, hipStream_t stream);
// lohi: int32[2] scratch that receives min(0, min x) and max(0, max x).
hipError_t stf_requantization_range(const int32_t* x, const float* mn,
                                    const float* mx, int32_t* lohi,
                                    float* out_mn, float* out_mx, int64_t n,
                                    hipStream_t stream);
hipError_t stf_quantize_down(const int32_t* x, const float* mn,
                             const float* mx, int32_t* lohi, uint8_t* y,
                             float* out_mn, float* out_mx, int64_t n,
                             hipStream_t stream);
// stf_quantize_down's second pass with the range [req_mn, req_mx] given.
hipError_t stf_requantize(const int32_t* x, const float* mn, const float* mx,
                          const float* req_mn, const float* req_mx,
                          uint8_t* y, float* out_mn, float* out_mx, int64_t n,
                          hipStream_t stream);
// x: quint8 [rows, C], bias: quint8 [C] -> y: qint32 [rows, C].
hipError_t stf_quantized_bias_add(const uint8_t* x, const uint8_t* bias,
                                  const float* min_x, const float* max_x,
                                  const float* min_b, const float* max_b,
                                  int32_t* y, float* out_mn, float* out_mx,
                                  int64_t rows, int64_t C,
                                  hipStream_t stream);
// NHWC quint8 max over the in-image taps; the range is copied through.
hipError_t stf_quantized_max_pool(const uint8_t* x, const float* mn,
                                  const float* mx, uint8_t* y, float* out_mn,
                                  float* out_mx, const StfPoolGeom* g,
                                  hipStream_t stream);
// NHWC quint8 integer mean over the in-image taps (sum / tap count,
// truncating); the range is copied through.
hipError_t stf_quantized_avg_pool(const uint8_t* x, const float* mn,
                                  const float* mx, uint8_t* y, float* out_mn,
                                  float* out_mx, const StfPoolGeom* g,
                                  hipStream_t stream);
hipError_t stf_quantized_relu6(const uint8_t* x, const float* mn,
                               const float* mx, uint8_t* y, float* out_mn,
                               float* out_mx, int64_t n, hipStream_t stream);
// QuantizedConcat takes its inputs in chunks of at most kStfQuantConcatMax,
// one table per chunk, passed by value to the kernels. Input k is viewed as
// [outer, inner[k]] and lands at column off[k] of the [outer, out_row]
// output; mn[k] / mx[k] are its device range scalars.
constexpr int kStfQuantConcatMax = 16;
struct StfQuantConcatArgs {
  const uint8_t* src[kStfQuantConcatMax];
  const float* mn[kStfQuantConcatMax];
  const float* mx[kStfQuantConcatMax];
  int64_t inner[kStfQuantConcatMax];
  int64_t off[kStfQuantConcatMax];
  int n;
};
// Folds the chunk's ranges into out_mn / out_mx: first starts the fold at
// [min(0, mn[0]), mx[0]], later chunks continue from the stored values. Call
// it for every chunk, in order, before the first stf_quantized_concat_copy.
hipError_t stf_quantized_concat_range(const StfQuantConcatArgs* a, int first,
                                      float* out_mn, float* out_mx,
                                      hipStream_t stream);
// Writes the chunk's columns of y. out_mn / out_mx hold the final range.
hipError_t stf_quantized_concat_copy(const StfQuantConcatArgs* a,
                                     const float* out_mn, const float* out_mx,
                                     uint8_t* y, int64_t outer,
                                     int64_t out_row, hipStream_t stream);

// ---- depthwise.hip ----
// Filter is [r, s, c, mult]; g->cout is unused.
hipError_t stf_depthwise_fwd(const void* x, const void* w, void* y,
                             const StfConvGeom* g, int mult,
                             hipStream_t stream);
hipError_t stf_depthwise_bwd_input(const void* dy, const void* w, void* dx,
                                   const StfConvGeom* g, int mult,
                                   hipStream_t stream);
hipError_t stf_depthwise_bwd_filter(const void* x, const void* dy,
                                    float* dw_f32, const StfConvGeom* g,
                                    int mult, hipStream_t stream);

// ---- elementwise.hip ----
hipError_t stf_unary(int op, int dtype, const void* x, void* y, int64_t n,
                     hipStream_t stream);
hipError_t stf_binary(int op, int dtype, const void* a, const void* b,
                      void* y, int64_t n, hipStream_t stream);
hipError_t stf_binary_scalar(int op, int dtype, const void* a,
                             const void* scalar, void* y, int64_t n,
                             int scalar_left, hipStream_t stream);
hipError_t stf_binary_bcast(int op, int dtype, const void* a, const void* b,
                            void* y, int64_t n, int rank,
                            const int64_t* out_dims, const int64_t* sa,
                            const int64_t* sb, hipStream_t stream);
hipError_t stf_cast(int sdt, int ddt, const void* x, void* y, int64_t n,
                    hipStream_t stream);
// Casts f32 -> bf16 and re-zeroes the source (split-K arena drain).
hipError_t stf_cast_f32_bf16_zero(void* src_f32, void* dst_bf16, int64_t n,
                                  hipStream_t stream);
hipError_t stf_fill_f32(void* y, float v, int64_t n, int as_bf16,
                        hipStream_t stream);
hipError_t stf_scale(int dtype, const void* x, void* y, int64_t n,
                     float factor, hipStream_t stream);
hipError_t stf_fused_elementwise(int dtype, const void** inputs,
                                 const uint8_t* scalar_flags, int n_in,
                                 const int64_t* prog, int n_prog, void* out,
                                 int64_t n, hipStream_t stream);

// ---- lrn.hip ----
hipError_t stf_lrn_fwd(const void* x, void* y, int64_t rows, int c,
                       int radius, float bias, float alpha, float beta,
                       hipStream_t stream);

// ---- loss.hip ----
hipError_t stf_bias_add(int dtype, const void* x, const void* bias, void* y,
                        int64_t n, int c, hipStream_t stream);
// db_f32 must be zeroed.
hipError_t stf_bias_grad(int dtype, const void* dy, void* db_f32,
                         int64_t rows, int c, hipStream_t stream);
hipError_t stf_softmax(int dtype, int log_sm, const void* x, void* y,
                       int64_t rows, int cols, hipStream_t stream);
hipError_t stf_sparse_xent(int dtype, const void* logits, const void* labels,
                           int labels_i32, void* loss_f32, void* backprop,
                           int64_t rows, int cols, hipStream_t stream);
hipError_t stf_xent(int dtype, const void* logits, const void* labels,
                    void* loss_f32, void* backprop, int64_t rows, int cols,
                    hipStream_t stream);

// ---- bn.hip ----
// x is [rows, c]. acc: zeroed f32 [2c]; mean/var/inv_std: f32 [c] outputs.
hipError_t stf_bn_fwd(int dtype, const void* x, const void* scale,
                      const void* offset, float* acc, float* mean, float* var,
                      float* inv_std, void* y, int64_t rows, int c, float eps,
                      int fuse_relu, hipStream_t stream);
// The statistics half of stf_bn_fwd (stf_bn_add_relu normalizes after it).
hipError_t stf_bn_stats_only(int dtype, const void* x, float* acc,
                             float* mean, float* var, float* inv_std,
                             int64_t rows, int c, float eps,
                             hipStream_t stream);
// y = relu(bn(x) + side); bf16 only, c % 8 == 0.
hipError_t stf_bn_add_relu(const void* x, const void* side, const float* mean,
                           const float* inv_std, const void* scale,
                           const void* offset, void* y, int64_t rows, int c,
                           hipStream_t stream);
// The forward from statistics that are already summed: acc is f32 [2c] =
// per-channel sum, then sum of squares, of x (read only). stf_bn_fwd_acc is
// stf_bn_fwd, and stf_bn_add_relu_acc is stf_bn_stats_only + stf_bn_add_relu,
// without the pass that reads x to fill acc.
hipError_t stf_bn_fwd_acc(int dtype, const void* x, const void* scale,
                          const void* offset, const float* acc, float* mean,
                          float* var, float* inv_std, void* y, int64_t rows,
                          int c, float eps, int fuse_relu,
                          hipStream_t stream);
hipError_t stf_bn_add_relu_acc(const void* x, const void* side,
                               const float* acc, float* mean, float* var,
                               float* inv_std, const void* scale,
                               const void* offset, void* y, int64_t rows,
                               int c, float eps, hipStream_t stream);
// The first pass of stf_bn_fwd alone: adds the column sums and sums of
// squares of x into acc (zeroed f32 [2c]).
hipError_t stf_bn_sums(int dtype, const void* x, float* acc, int64_t rows,
                       int c, hipStream_t stream);
// acc[j] += sum over t of partial[t][j], j < cols (zeroed f32 acc). With
// cols = 2 * cout this turns the partial[tiles][2][cout] of the *_8ph_stats
// GEMMs into the acc layout above.
hipError_t stf_bn_partial_sums(const float* partial, float* acc,
                               int64_t tiles, int cols, hipStream_t stream);
// sum_dy (= doffset) and sum_dy_xhat (= dscale) are zeroed f32 [c] and are
// accumulated in place. dside (optional, fuse_relu only): also receives the
// ReLU-masked dy, y_relu > 0 ? dy : 0, the gradient of the residual branch.
hipError_t stf_bn_bwd(int dtype, const void* dy, const void* x,
                      const void* y_relu, const float* mean,
                      const float* inv_std, const void* scale, float* sum_dy,
                      float* sum_dy_xhat, void* dx, void* dside, int64_t rows,
                      int c, int fuse_relu, hipStream_t stream);

// ---- pool.hip ----
hipError_t stf_pool_fwd(int dtype, int is_max, const void* x, void* y,
                        const StfPoolGeom* g, hipStream_t stream);
// dx_f32: zeroed scratch [N*H*W*C]; the caller casts it to the output dtype.
hipError_t stf_max_pool_bwd(int dtype, const void* x, const void* dy,
                            float* dx_f32, const StfPoolGeom* g,
                            hipStream_t stream);
// bf16, C % 8 == 0: writes dx directly, no scratch.
hipError_t stf_max_pool_bwd_v8(const void* x, const void* dy, void* dx_bf16,
                               const StfPoolGeom* g, hipStream_t stream);
hipError_t stf_avg_pool_bwd(int dtype, const void* dy, void* dx,
                            const StfPoolGeom* g, hipStream_t stream);

// ---- lstm.hip ----
hipError_t stf_lstm_gates(int dtype, const void* gates, const void* c_prev,
                          float forget_bias, void* i_out, void* f_out,
                          void* o_out, void* ci_out, void* cs_out,
                          void* co_out, void* h_out, int64_t batch, int H,
                          hipStream_t stream);
hipError_t stf_lstm_gates_grad(int dtype, const void* c_prev, const void* i_,
                               const void* f_, const void* o_,
                               const void* ci_, const void* co_,
                               const void* dh, const void* dcs_next,
                               void* dgates, void* dc_prev, int64_t batch,
                               int H, hipStream_t stream);

// ---- layout.hip ----
// elem_size is 2, 4 or 8 bytes: these copy bits whatever the dtype.
hipError_t stf_transpose2d(int elem_size, const void* in, void* out,
                           int64_t rows, int64_t cols, hipStream_t stream);
// out[i] = in[sum_d coord_d(i) * src_strides[d]] over out_dims; a stride of 0
// broadcasts that dim. hipErrorInvalidValue unless
// 0 <= rank <= kStfMaxPermuteRank.
hipError_t stf_permute(int elem_size, const void* in, void* out, int64_t n,
                       int rank, const int64_t* out_dims,
                       const int64_t* src_strides, hipStream_t stream);
hipError_t stf_block_pad(int dtype, const void* src, void* dst,
                         int64_t nblocks, int64_t in_block, int64_t out_block,
                         hipStream_t stream);
// Moves [outer, rows, inner] between a contiguous side and rows
// [row_off, row_off + rows) of a [outer, big_stride, inner] side; scatter:
// contiguous src -> strided dst.
hipError_t stf_strided_copy(int elem_size, int scatter, const void* src,
                            void* dst, int64_t outer, int64_t rows,
                            int64_t inner, int64_t big_stride,
                            int64_t row_off, hipStream_t stream);

// ---- reduce.hip ----
// Accumulates 0.5 * sum(x^2) into a zeroed out_f32.
hipError_t stf_l2loss(int dtype, const void* x, float* out_f32, int64_t n,
                      hipStream_t stream);
hipError_t stf_full_reduce(int dtype, StfReduce red, const void* x,
                           float* out_f32, int64_t n, hipStream_t stream);
hipError_t stf_row_reduce(int dtype, StfReduce red, const void* x, float* y,
                          int64_t rows, int64_t inner, hipStream_t stream);
hipError_t stf_col_reduce(int dtype, StfReduce red, const void* x, float* y,
                          int64_t outer, int64_t inner, hipStream_t stream);

// ---- optimizer.hip ----
// f32 variables and slots; hyper-parameters are device f32 scalars.
hipError_t stf_apply_sgd(int grad_bf16, void* var, const void* lr,
                         const void* grad, int64_t n, hipStream_t stream);
hipError_t stf_apply_momentum(int grad_bf16, void* var, void* accum,
                              const void* lr, const void* grad,
                              const void* momentum, int nesterov, int64_t n,
                              hipStream_t stream);
hipError_t stf_apply_adam(int grad_bf16, void* var, void* m, void* v,
                          const void* b1p, const void* b2p, const void* lr,
                          const void* b1, const void* b2, const void* eps,
                          const void* grad, int64_t n, hipStream_t stream);

// ---- random.hip ----
// ctr_dev: device uint64 Philox offset, advanced by each call.
hipError_t stf_random_uniform(uint64_t seed, void* ctr_dev, void* out,
                              int64_t n, int as_bf16, hipStream_t stream);
hipError_t stf_random_normal(uint64_t seed, void* ctr_dev, void* out,
                             int64_t n, int as_bf16, int truncated,
                             hipStream_t stream);

// ---- embedding.hip ----
hipError_t stf_gather_rows(int dtype, int idx_i32, const void* params,
                           const void* indices, void* out, int64_t nidx,
                           int64_t row, int64_t nrows, hipStream_t stream);
// out_f32 must be zeroed.
hipError_t stf_segment_sum(int dtype, int idx_i32, const void* data,
                           const void* ids, float* out_f32, int64_t nidx,
                           int64_t row, int64_t nseg, hipStream_t stream);

// ---- comm_pack.hip ----
int stf_comm_max_segments();
hipError_t stf_comm_pack(int nseg, const void* const* ptrs,
                         const int64_t* ends, const unsigned char* is_bf16,
                         float* dst, int64_t total, hipStream_t stream);
hipError_t stf_comm_unpack(int nseg, void* const* ptrs, const int64_t* ends,
                           const unsigned char* is_bf16, const float* src,
                           float scale, int64_t total, hipStream_t stream);

}  // extern "C"
