// Layout copies: LDS-tiled 2D transpose, generic strided permute (Transpose
// and broadcast Tile), blocked channel pad, strided block copy for
// concat/split/pack/unpack/slice. They move bits, so all but the pad are
// typed by element size only. (Replaces reference transpose_functor_gpu,
// tile_ops_gpu, concat_lib_gpu, split_lib_gpu — wave64-native designs.)
#include "hip_common.h"

namespace {

// ---- 2D transpose: out[j,i] = in[i,j]; LDS 64x64 tile with +1-pad ----
template <typename T>
__global__ void Transpose2DKernel(const T* __restrict__ in, T* __restrict__ out,
                                  int64_t rows, int64_t cols) {
  __shared__ T tile[64][65];
  int64_t tiles_c = (cols + 63) / 64;
  int64_t bid = blockIdx.x;
  int64_t br = bid / tiles_c, bc = bid % tiles_c;
  int64_t r0 = br * 64, c0 = bc * 64;
  int tx = threadIdx.x & 63;   // col within tile
  int ty = threadIdx.x >> 6;   // 4 rows per pass
  for (int p = 0; p < 16; ++p) {
    int64_t r = r0 + ty + p * 4;
    int64_t c = c0 + tx;
    if (r < rows && c < cols) tile[ty + p * 4][tx] = in[r * cols + c];
  }
  __syncthreads();
  for (int p = 0; p < 16; ++p) {
    int64_t r = c0 + ty + p * 4;  // output row = input col
    int64_t c = r0 + tx;          // output col = input row
    if (r < cols && c < rows) out[r * rows + c] = tile[tx][ty + p * 4];
  }
}

// ---- generic permute: out[i] = in[sum_d coord_d(i) * src_strides[d]] ----
struct PermArgs {
  int rank;
  int64_t out_dims[kStfMaxPermuteRank];
  int64_t src_strides[kStfMaxPermuteRank];  // stride in src for each out dim
};

template <typename T>
__global__ void PermuteKernel(const T* __restrict__ in, T* __restrict__ out,
                              int64_t n, PermArgs args) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int64_t rem = i, src = 0;
    for (int d = args.rank - 1; d >= 0; --d) {
      int64_t c = rem % args.out_dims[d];
      rem /= args.out_dims[d];
      src += c * args.src_strides[d];
    }
    out[i] = in[src];
  }
}

// Blocked channel pad/unpad: view src as [nblocks, in_block] and dst as
// [nblocks, out_block]; elements past in_block zero-fill (pad mode when
// out_block > in_block, truncate when smaller). Lets C%8!=0 convolutions
// (the ResNet/Inception stems, C=3) take the 8-channel implicit-GEMM path.
template <typename T>
__global__ void BlockPadKernel(const T* __restrict__ src, T* __restrict__ dst,
                               int64_t nblocks, int64_t in_block,
                               int64_t out_block) {
  int64_t total = nblocks * out_block;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    int64_t b = i / out_block;
    int64_t off = i - b * out_block;
    dst[i] = off < in_block ? src[b * in_block + off] : (T)0;
  }
}

// strided block copy for concat/split: moves [outer, rows, inner] between a
// contiguous side and a strided side (dst_stride rows, dst_off row offset).
template <typename T, bool SCATTER>  // SCATTER: contiguous src -> strided dst
__global__ void StridedCopyKernel(const T* __restrict__ src,
                                  T* __restrict__ dst, int64_t outer,
                                  int64_t rows, int64_t inner,
                                  int64_t big_stride, int64_t row_off,
                                  int64_t n) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n;
       idx += stride) {
    int64_t i = idx % inner;
    int64_t rem = idx / inner;
    int64_t a = rem % rows;
    int64_t o = rem / rows;
    int64_t small = (o * rows + a) * inner + i;
    int64_t big = (o * big_stride + row_off + a) * inner + i;
    if (SCATTER) dst[big] = src[small];
    else dst[small] = src[big];
  }
}

}  // namespace

extern "C" {

hipError_t stf_transpose2d(int elem_size, const void* in, void* out,
                           int64_t rows, int64_t cols, hipStream_t stream) {
  int64_t blocks = ((rows + 63) / 64) * ((cols + 63) / 64);
  DispatchElemSize(elem_size, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((Transpose2DKernel<T>), dim3((uint32_t)blocks),
                       dim3(256), 0, stream, (const T*)in, (T*)out, rows,
                       cols);
  });
  return hipGetLastError();
}

hipError_t stf_permute(int elem_size, const void* in, void* out, int64_t n,
                       int rank, const int64_t* out_dims,
                       const int64_t* src_strides, hipStream_t stream) {
  if (rank < 0 || rank > kStfMaxPermuteRank) return hipErrorInvalidValue;
  PermArgs args;
  args.rank = rank;
  for (int i = 0; i < rank; ++i) {
    args.out_dims[i] = out_dims[i];
    args.src_strides[i] = src_strides[i];
  }
  DispatchElemSize(elem_size, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((PermuteKernel<T>), ElemwiseGrid(n, 256, 4), dim3(256),
                       0, stream, (const T*)in, (T*)out, n, args);
  });
  return hipGetLastError();
}

hipError_t stf_block_pad(int dtype, const void* src, void* dst,
                         int64_t nblocks, int64_t in_block,
                         int64_t out_block, hipStream_t stream) {
  DispatchDtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(BlockPadKernel<T>,
                       ElemwiseGrid(nblocks * out_block, 256, 4), dim3(256),
                       0, stream, (const T*)src, (T*)dst, nblocks, in_block,
                       out_block);
  });
  return hipGetLastError();
}

hipError_t stf_strided_copy(int elem_size, int scatter, const void* src,
                            void* dst, int64_t outer, int64_t rows,
                            int64_t inner, int64_t big_stride, int64_t row_off,
                            hipStream_t stream) {
  int64_t n = outer * rows * inner;
  DispatchElemSize(elem_size, [&](auto t) {
    using T = typename decltype(t)::type;
    DispatchBool(scatter, [&](auto sc) {
      hipLaunchKernelGGL((StridedCopyKernel<T, decltype(sc)::value>),
                         ElemwiseGrid(n, 256, 4), dim3(256), 0, stream,
                         (const T*)src, (T*)dst, outer, rows, inner,
                         big_stride, row_off, n);
    });
  });
  return hipGetLastError();
}

}  // extern "C"
