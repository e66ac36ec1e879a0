// Stateful helpers shared by the GPU OpKernel files. Defined here, once, so
// the process has exactly one split-K arena map and one zero page.
#include "kernels/gpu_common.h"

#include <map>
#include <mutex>

namespace stf {

int PickSplitK(int64_t M, int64_t N, int64_t K) {
  // guide: blocks ~= 0.5-2x CU count
  int64_t tiles = ((M + 127) / 128) * ((N + 127) / 128);
  if (tiles >= 256 || K < 1024) return 1;
  // Measured optimum keeps ~48 K-chunks (of 64) per block: enough work to
  // amortize the prologue, enough blocks to hide staging latency
  // (576x64x802816: 725us @ sk=102 -> 605us @ sk~260).
  static const int64_t target = [] {
    const char* e = getenv("STF_SPLITK_TARGET");
    return e ? atoll(e) : 0;
  }();
  int64_t want;
  if (target > 0) {
    want = target / (tiles ? tiles : 1);
  } else {
    want = 512 / (tiles ? tiles : 1);
    // Very skinny outputs with huge K (the 7x7 stem dW: 392x64x3.2M):
    // deepen the split to ~2048 blocks (sweep: 3.14ms @1044 blocks ->
    // 2.39ms @2048; flat beyond). Keep >=48 K-chunks per block.
    int64_t kt = K / 64;
    if (tiles <= 6 && kt / (tiles * want) > 96) {
      want = 2048 / tiles;
      if (want > kt / 48) want = kt / 48;
      if (tiles * want > 4096) want = 4096 / tiles;
    }
  }
  int64_t maxk = K / 512;  // keep >= 8 K-iters per slice
  if (maxk < 1) maxk = 1;
  int64_t sk = std::min(want, maxk);
  return (int)(sk < 1 ? 1 : sk);
}

// Every split-K GEMM atomically accumulates into the arena and the fused
// cast-and-rezero epilogue restores the all-zero invariant while draining
// the result — the per-GEMM hipMemset launch disappears. All compute runs
// on one stream and SplitKInto enqueues each use's accumulation and drain
// under one lock, so consecutive uses are ordered; growth leaks the old
// buffer deliberately (in-flight work and captured hipGraphs may still
// reference it).
float* SplitKArena(int ordinal, int64_t elems, hipStream_t s) {
  if (elems * 4 > (1ll << 28)) return nullptr;  // >256 MB: use a temp
  static std::mutex mu;
  static std::map<int, std::pair<float*, int64_t>> arenas;
  std::lock_guard<std::mutex> l(mu);
  auto& a = arenas[ordinal];
  if (a.second < elems) {
    int64_t cap = a.second * 2 > elems ? a.second * 2 : elems;
    if (cap < (1 << 20)) cap = 1 << 20;
    float* p = nullptr;
    if (hipMalloc(&p, cap * 4) != hipSuccess) return nullptr;
    if (hipMemsetAsync(p, 0, cap * 4, s) != hipSuccess) return nullptr;
    a = {p, cap};
  }
  return a.first;
}

// Allocated once per process (one GPU per process under the data-parallel
// model).
const void* ZeroPage() {
  static const void* page = [] {
    void* p = nullptr;
    if (hipMalloc(&p, 256) != hipSuccess) return (void*)nullptr;
    (void)hipMemset(p, 0, 256);
    return p;
  }();
  return page;
}

hipError_t SplitKInto(OpKernelContext* ctx, int64_t elems,
                      const std::function<hipError_t(float*)>& launch,
                      void* out_bf16) {
  hipStream_t s = GPU_STREAM(ctx);
  // The executor runs independent ops on pool threads, all enqueueing on
  // the one compute stream. The accumulation and the drain that re-zeroes
  // the arena must reach the stream back to back: were another split-K
  // op's accumulation enqueued between them, the first drain would hand out
  // the sum of both and the second one zeros. Held for two enqueues only.
  static std::mutex enqueue_mu;
  std::unique_lock<std::mutex> l(enqueue_mu);
  if (float* arena = SplitKArena(ctx->device()->gpu_ordinal(), elems, s)) {
    hipError_t e = launch(arena);
    if (e != hipSuccess) return e;
    return stf_cast_f32_bf16_zero(arena, out_bf16, elems, s);
  }
  l.unlock();
  Tensor scratch = ctx->allocate_temp(DT_FLOAT, TensorShape({elems}));
  hipError_t e = ZeroF32(scratch.raw_data(), elems, s);
  if (e != hipSuccess) return e;
  e = launch(scratch.flat<float>());
  if (e != hipSuccess) return e;
  return stf_cast(0, 1, scratch.raw_data(), out_bf16, elems, s);
}

hipError_t GemmBf16AutoEx(OpKernelContext* ctx, const void* A, const void* B,
                          void* C_bf16, int64_t M, int64_t N, int64_t K,
                          int64_t lda, int64_t ldb, int a_km, int b_km,
                          hipStream_t s) {
  int sk = PickSplitK(M, N, K);
  if (sk <= 1)
    return stf_gemm_bf16(A, B, C_bf16, M, N, K, lda, ldb, a_km, b_km, s);
  return SplitKInto(ctx, M * N, [&](float* acc) {
    return stf_gemm_bf16_splitk(A, B, acc, M, N, K, lda, ldb, a_km, b_km, sk,
                                s);
  }, C_bf16);
}

}  // namespace stf
