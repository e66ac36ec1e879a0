// Tall-skinny Conv2D backprop-filter for cout = 64 on gfx950:
//   dW[(r,s,c), k] += sum over output pixels of x[window] * dy[pixel, k]
// as f32 atomics into a zeroed accumulator (the SplitKInto contract).
//
// One 4-wave block holds the whole [r*s*c, 64] output in registers: the 16-row
// tiles are dealt round-robin to the waves, TPW tiles x 4 column tiles each.
// The blocks split the output pixels, so dy is read from global memory once
// per launch and x once per filter row (the halo rows of consecutive output
// rows overlap; a block owns a contiguous range of steps, so those re-reads
// are its own recent lines).
//
// A step is a run of kW = 32 output pixels of one output row (n, p). Per step
// the block copies into LDS, with global_load_lds, in natural NHWC layout:
//   dy tile   [32 pixels][64]                       (zero rows past q)
//   x halo    [r rows][(kW-1)*sw + s columns][c]    (zero outside the image)
// The r*s filter taps are shifted views of the halo; nothing is expanded.
// Both MFMA operands want the pixel index contiguous per lane while LDS has
// the channels contiguous: ds_read_b64_tr_b16 transposes on the read
// (FragTr in conv_dw_frag.h). Three LDS buffers: the loads of step t+2 are
// issued before the MFMAs of step t.
#include "conv_dw_frag.h"
#include "hip_common.h"
#include "stf_kernels.h"

#include <type_traits>

namespace {

using namespace stf_dw;  // FragK, FragRow, FragTr, Glds16, WaitLoads

constexpr int kW = 32;             // output pixels per step = one MFMA K
constexpr int kCout = 64;
constexpr int kDySlots = kW * 8;   // 16B slots of the dy tile
constexpr int kThreads = 256;
constexpr int kMaxRsc = 576;       // 36 row tiles: 9 per wave
constexpr int kMaxLds = 160 * 1024;
constexpr int kBufs = 3;            // LDS buffers: loads run two steps ahead

// Test kernel: tile is [32 k][16 rows] u16; out[lane][e] is what the MFMA
// operand register of that lane holds.
__global__ void FragTrProbe(const uint16_t* tile, uint16_t* out) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[32 * 16];
  int lane = threadIdx.x;
  for (int i = lane; i < 32 * 16; i += 64) lds[i] = tile[i];
  __syncthreads();
  bf16x8 f = FragTr(lds + FragK(lane, 0) * 16 + FragRow(lane),
                    lds + FragK(lane, 1) * 16 + FragRow(lane));
  s16x8 v = __builtin_bit_cast(s16x8, f);
#pragma unroll
  for (int e = 0; e < 8; ++e) out[lane * 8 + e] = (uint16_t)v[e];
}

// ---------------------------------------------------------------------------
// Launch-constant geometry.
// ---------------------------------------------------------------------------
struct DwTallArgs {
  const uint16_t* x;
  const uint16_t* dy;
  float* dw;
  const uint16_t* zero16;
  int H, W, C, S, sh, sw, ph, pw, P, Q;
  int rsc;          // r*s*c, rows of dW
  int cpp;          // 16B chunks per pixel = c / 8
  int swz;          // chunk swizzle mask: (largest power of 2 in cpp, <= 8) - 1
  int wcols;        // halo columns
  int row_slots;    // wcols * cpp
  int x_slots;      // r * row_slots
  int x_slots_pad;  // rounded up to kThreads
  int qsteps;       // steps per output row
  int nsteps;       // n * p * qsteps
  int per_block;    // steps per block
  int loads;        // global_load_lds per thread and step
  U32Div div_row_slots, div_cpp, div_c, div_s, div_qsteps, div_p;
};

// Staging of one step. LDS slot i of a wave's 64-slot group comes from lane
// i, so every lane stays active: slots past the tile (x_slots_pad rounds up)
// read the zero page into padding. Chunk c of halo column col lands at chunk
// c ^ (col & swz) of that pixel (the source carries the swizzle); the dy tile
// has 8 chunks per pixel and swizzles with pixel & 7.
//
// Which halo slot (row, column, chunk) a thread's k-th load fills does not
// depend on the step, so the first kPre of them are decoded once, before the
// loop; a step then costs a bounds test and an add per load. With one wave
// per SIMD the address arithmetic is not hidden behind another wave: decoding
// per step (two magic divisions per load) cost 10 % of the kernel's time.
constexpr int kPre = 6;

struct Stager {
  int rc[kPre];   // halo row | column << 12; -1: padding slot
  int off[kPre];  // (row * W + column) * C + chunk * 8, in elements
  int dy_pix, dy_off;

  static __device__ __forceinline__ void Decode(const DwTallArgs& a, int idx,
                                                int* rc, int* off) {
    uint32_t rr = a.div_row_slots.div((uint32_t)idx);
    uint32_t j = a.div_row_slots.mod((uint32_t)idx, rr);
    uint32_t col = a.div_cpp.div(j);
    uint32_t ch = a.div_cpp.mod(j, col) ^ (col & (uint32_t)a.swz);
    *rc = (int)(rr | (col << 12));
    *off = ((int)rr * a.W + (int)col) * a.C + (int)ch * 8;
  }

  __device__ __forceinline__ void Init(const DwTallArgs& a, int tid) {
#pragma unroll
    for (int k = 0; k < kPre; ++k) {
      int idx = tid + k * kThreads;
      rc[k] = -1;
      off[k] = 0;
      if (idx < a.x_slots) Decode(a, idx, &rc[k], &off[k]);
    }
    dy_pix = tid >> 3;
    dy_off = dy_pix * kCout + ((tid & 7) ^ (dy_pix & 7)) * 8;
  }

  __device__ __forceinline__ void Issue(const DwTallArgs& a, int step,
                                        uint16_t* xbuf, uint16_t* dybuf,
                                        int tid) const {
    uint32_t np = a.div_qsteps.div((uint32_t)step);
    int q0 = (int)a.div_qsteps.mod((uint32_t)step, np) * kW;
    uint32_t n = a.div_p.div(np);
    int p = (int)a.div_p.mod(np, n);
    int h0 = p * a.sh - a.ph, w0 = q0 * a.sw - a.pw;
    // element (h0, w0, 0) of image n; outside the image when padding is hit,
    // and then only added to, never read
    const uint16_t* origin =
        a.x + (((int64_t)n * a.H + h0) * a.W + w0) * a.C;
    auto load = [&](int rck, int offk, int idx) {
      const uint16_t* src = a.zero16;
      int h = h0 + (rck & 0xfff), w = w0 + (rck >> 12);
      if (rck >= 0 && h >= 0 && h < a.H && w >= 0 && w < a.W)
        src = origin + offk;
      Glds16(src, xbuf + (idx - (tid & 63)) * 8);
    };
#pragma unroll
    for (int k = 0; k < kPre; ++k)
      if (k * kThreads < a.x_slots_pad) load(rc[k], off[k], tid + k * kThreads);
    for (int idx = tid + kPre * kThreads; idx < a.x_slots_pad;
         idx += kThreads) {
      int rck = -1, offk = 0;
      if (idx < a.x_slots) Decode(a, idx, &rck, &offk);
      load(rck, offk, idx);
    }
    const uint16_t* src = a.zero16;
    if (q0 + dy_pix < a.Q)
      src = a.dy + ((int64_t)np * a.Q + q0) * kCout + dy_off;
    Glds16(src, dybuf + (tid & ~63) * 8);
  }
};

// TPW = row tiles per wave; wave w owns tiles t*4 + w. A tile past the filter
// (only in the last round) is computed on valid addresses and not stored: a
// branch around it would move the accumulators between register files.
template <int TPW>
__launch_bounds__(kThreads) __global__ void ConvDwTall(DwTallArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
  int tid = threadIdx.x;
  int lane = tid & 63;
  int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  int buf_elems = (a.x_slots_pad + kDySlots) * 8;
  auto xbuf = [&](int b) { return lds + b * buf_elems; };
  auto dybuf = [&](int b) { return lds + b * buf_elems + a.x_slots_pad * 8; };

  // Step-invariant LDS offsets (in elements) of this lane's two reads per
  // fragment. A: rows = (tap, channel) of the filter, k = pixel of the step;
  // a 4-row run stays inside one tap because c % 8 == 0.
  int a_off[TPW][2];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    int row = (t * 4 + wid) * 16 + FragRow(lane);
    if (row >= a.rsc) row = 0;  // rows past the filter: read anything valid
    uint32_t tap = a.div_c.div((uint32_t)row);
    int ch = (int)a.div_c.mod((uint32_t)row, tap);
    uint32_t fr = a.div_s.div(tap);
    int fs = (int)a.div_s.mod(tap, fr);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      int col = fs + FragK(lane, h) * a.sw;
      a_off[t][h] = (((int)fr * a.wcols + col) * a.cpp +
                     ((ch >> 3) ^ (col & a.swz))) * 8 + (ch & 7);
    }
  }
  int b_off[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int cout = j * 16 + FragRow(lane);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      int pix = FragK(lane, h);
      b_off[j][h] = (pix * 8 + ((cout >> 3) ^ (pix & 7))) * 8 + (cout & 7);
    }
  }

  f32x4 acc[TPW][4];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[t][j] = {0.f, 0.f, 0.f, 0.f};

  int step = blockIdx.x * a.per_block;
  int end = min(a.nsteps, step + a.per_block);
  // Three buffers, loads two steps ahead: the loads of step t+2 are issued
  // after the barrier of step t (their buffer was read in step t-1) and have
  // two steps of MFMAs to land. Each thread issues a.loads loads per step and
  // they complete in order, so "at most a.loads outstanding" means step t's
  // have landed.
  Stager st;
  st.Init(a, tid);
  st.Issue(a, step, xbuf(0), dybuf(0), tid);
  if (step + 1 < end) st.Issue(a, step + 1, xbuf(1), dybuf(1), tid);
  int cur = 0;
  for (; step < end; ++step) {
    WaitLoads(step + 1 < end ? a.loads : 0);
    __builtin_amdgcn_s_barrier();
    int nxt = cur == 0 ? 2 : cur - 1;
    if (step + 2 < end) st.Issue(a, step + 2, xbuf(nxt), dybuf(nxt), tid);
    const uint16_t* xt = xbuf(cur);
    const uint16_t* dt = dybuf(cur);
    bf16x8 bfrag[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      bfrag[j] = FragTr(dt + b_off[j][0], dt + b_off[j][1]);
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      bf16x8 afrag = FragTr(xt + a_off[t][0], xt + a_off[t][1]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            afrag, bfrag[j], acc[t][j], 0, 0, 0);
    }
    cur = cur == 2 ? 0 : cur + 1;
  }

#pragma unroll
  for (int t = 0; t < TPW; ++t) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int col = j * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int row = (t * 4 + wid) * 16 + (lane >> 4) * 4 + i;
        if (row < a.rsc) atomicAdd(a.dw + row * kCout + col, acc[t][j][i]);
      }
    }
  }
}

// Host-side geometry; false when the gate does not hold.
bool MakeArgs(const StfConvGeom& g, DwTallArgs* a) {
  int64_t M = (int64_t)g.n * g.p * g.q;
  int64_t rsc = (int64_t)g.r * g.s * g.c;
  if (g.cout != kCout || (g.c % 8) != 0 || rsc > kMaxRsc || (M % 64) != 0 ||
      M < 768)
    return false;
  int64_t wcols = (int64_t)(kW - 1) * g.sw + g.s;
  int64_t x_slots = g.r * wcols * (g.c / 8);
  int64_t x_slots_pad = (x_slots + kThreads - 1) / kThreads * kThreads;
  if (kBufs * (x_slots_pad + kDySlots) * 16 > kMaxLds) return false;
  int qsteps = (g.q + kW - 1) / kW;
  int64_t nsteps = (int64_t)g.n * g.p * qsteps;
  // 32-bit step counter and in-image element offsets
  if (nsteps >= (1ll << 31) || (int64_t)g.h * g.w * g.c >= (1ll << 31) ||
      g.r >= (1 << 12))
    return false;
  a->H = g.h; a->W = g.w; a->C = g.c; a->S = g.s;
  a->sh = g.sh; a->sw = g.sw; a->ph = g.ph; a->pw = g.pw;
  a->P = g.p; a->Q = g.q;
  a->rsc = (int)rsc;
  a->cpp = g.c / 8;
  int pow2 = a->cpp & -a->cpp;
  a->swz = (pow2 > 8 ? 8 : pow2) - 1;
  a->wcols = (int)wcols;
  a->row_slots = (int)(wcols * a->cpp);
  a->x_slots = (int)x_slots;
  a->x_slots_pad = (int)x_slots_pad;
  a->loads = (int)(x_slots_pad / kThreads) + 1;
  a->qsteps = qsteps;
  a->nsteps = (int)nsteps;
  a->div_row_slots.init((uint32_t)a->row_slots);
  a->div_cpp.init((uint32_t)a->cpp);
  a->div_c.init((uint32_t)g.c);
  a->div_s.init((uint32_t)g.s);
  a->div_qsteps.init((uint32_t)qsteps);
  a->div_p.init((uint32_t)g.p);
  return true;
}

}  // namespace

extern "C" {

int stf_conv2d_dw_tall_ok(const StfConvGeom* g) {
  DwTallArgs a;
  return MakeArgs(*g, &a);
}

hipError_t stf_conv2d_dw_tall(const void* x, const void* dy, void* dw_f32,
                              const void* zero16, const StfConvGeom* g,
                              hipStream_t stream) {
  DwTallArgs a;
  if (!MakeArgs(*g, &a)) return hipErrorInvalidValue;
  a.x = (const uint16_t*)x;
  a.dy = (const uint16_t*)dy;
  a.dw = (float*)dw_f32;
  a.zero16 = (const uint16_t*)zero16;
  // about one block per CU, each on a contiguous range of steps
  int blocks = a.nsteps < STF_NUM_CU ? a.nsteps : STF_NUM_CU;
  a.per_block = (a.nsteps + blocks - 1) / blocks;
  blocks = (a.nsteps + a.per_block - 1) / a.per_block;
  size_t shmem = kBufs * (size_t)(a.x_slots_pad + kDySlots) * 16;
  int tiles = (a.rsc + 15) / 16;
  int tpw = (tiles + 3) / 4;
  auto launch = [&](auto tpw_c) {
    constexpr int TPW = decltype(tpw_c)::value;
    hipLaunchKernelGGL(ConvDwTall<TPW>, dim3((uint32_t)blocks),
                       dim3(kThreads), shmem, stream, a);
  };
  switch (tpw) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    case 5: launch(std::integral_constant<int, 5>{}); break;
    case 6: launch(std::integral_constant<int, 6>{}); break;
    case 7: launch(std::integral_constant<int, 7>{}); break;
    case 8: launch(std::integral_constant<int, 8>{}); break;
    default: launch(std::integral_constant<int, 9>{}); break;
  }
  return hipGetLastError();
}

hipError_t stf_conv2d_dw_tall_frag_probe(const void* tile_u16, void* out_u16,
                                         hipStream_t stream) {
  hipLaunchKernelGGL(FragTrProbe, dim3(1), dim3(64), 0, stream,
                     (const uint16_t*)tile_u16, (uint16_t*)out_u16);
  return hipGetLastError();
}

}  // extern "C"
