// Wide Conv2D backprop-filter for cout = 64*k on gfx950, for the shapes whose
// [r*s*c, cout] output does not fit one block's registers (conv_dw_tall.hip):
//   dW[(r,s,c), k] += sum over output pixels of x[window] * dy[pixel, k]
// as f32 atomics into a zeroed accumulator (the SplitKInto contract).
//
// The output is cut into (channel slice) x (cout slice) pieces. A block of 8
// waves owns all r*s taps of CS channels (r*s*CS <= 576 rows, 36 row tiles)
// by 128 columns, and a contiguous range of steps; blocks of the same slice
// add into the same piece of dW. Wave (wr, wc), wr = 0..3, wc = 0..1, holds
// row tiles t*4 + wr by column tiles wc*4..wc*4+3: TPW x 4 accumulator tiles,
// as a wave of the tall kernel, while every staged byte feeds twice the MFMAs.
//
// A step is a patch of PH x PW = 32 output pixels of one image, PW = 32, 16
// or 8, chosen to waste the fewest pixels of a p x q output (7x7 fills 8x4
// patches to 87.5 %; a 32-pixel run of one row would be 22 % full). MFMA k
// index k is patch pixel (k / PW, k % PW). Per step the block copies into
// LDS, with global_load_lds, in NHWC order:
//   dy tile  [32 pixels][128]       (zero rows past p or q, zero columns
//                                    past cout in a half-empty last slice)
//   x halo   [HR rows][HC columns][CS]            (zero outside the image)
// with HR = (PH-1)*sh + r, HC = (PW-1)*sw + s. On an axis where the filter
// extent is 1 only the sampled pixels are staged (HR = PH resp. HC = PW; the
// global pitch is the stride and the LDS pitch 1): a stride-2 1x1 would
// otherwise stage four times what it reads. The r*s taps are shifted views
// of the halo. Fragment reads, the three LDS buffers and the counted vmcnt
// are those of the tall kernel (conv_dw_frag.h).
#include "conv_dw_frag.h"
#include "hip_common.h"
#include "stf_kernels.h"

#include <type_traits>

namespace {

using namespace stf_dw;  // FragK, FragRow, FragTr, Glds16, WaitLoads

constexpr int kK = 32;              // output pixels per step = one MFMA K
constexpr int kCoutSlice = 128;
constexpr int kThreads = 512;
constexpr int kDySlots = kK * (kCoutSlice / 8);  // 16B slots: one per thread
constexpr int kMaxRows = 576;       // 36 row tiles: 9 per wave row
constexpr int kMaxLds = 160 * 1024;
constexpr int kBufs = 3;            // LDS buffers: loads run two steps ahead
// halo loads per thread and step; the LDS budget allows no more:
// 3 * 16 * (5 * 512 + 512) = 144 KiB, and 6 * 512 slots would be 168 KiB
constexpr int kPre = 5;
static_assert(kBufs * 16 * ((kPre + 1) * kThreads + kDySlots) > kMaxLds, "");

struct DwWideArgs {
  const uint16_t* x;
  const uint16_t* dy;
  float* dw;
  const uint16_t* zero16;
  int H, W, C, Cout, S, sh, sw, ph, pw, P, Q;
  int CS;           // channels of a slice
  int cpp;          // 16B chunks per halo pixel = CS / 8
  int swz;          // chunk swizzle mask: (largest power of 2 in cpp, <= 8) - 1
  int lgpw;         // PW = 1 << lgpw, PH = 32 >> lgpw
  int gh, gw;       // image rows / columns per halo row / column
  int lh, lw;       // halo rows / columns per patch row / column
  int hcols;        // HC
  int rows;         // r*s*CS, rows of dW in a slice
  int x_slots;      // HR * HC * cpp
  int x_slots_pad;  // rounded up to kThreads
  int loads;        // global_load_lds per thread and step
  int cslices, coslices;
  int ppw, pph;     // patches per image along q and p
  int nsteps;       // n * pph * ppw
  int per_block;    // steps per block
  U32Div div_row_slots, div_cpp, div_cs, div_s, div_ppw, div_pp, div_cslices;
};

// Staging of one step, as in the tall kernel: LDS slot i of a wave's 64-slot
// group comes from lane i, slots past the halo read the zero page into
// padding, chunk ch of halo column col lands at chunk ch ^ (col & swz). The
// dy tile has 16 chunks per pixel and 256-byte rows, so the 4 pixels that 16
// lanes of a transposing read touch would share their banks: chunk ch of
// pixel k lands at ch ^ 2 * (k & 7), which moves each pixel's 32-byte run of
// one column tile to banks of its own.
//
// Which halo slot a thread's k-th load fills does not depend on the step: it
// is decoded once, and a step costs a bounds test and an add per load.
struct Stager {
  int rc[kPre];   // image row | column << 12 relative to the halo origin;
                  // -1: padding slot
  int off[kPre];  // (row * W + column) * C + chunk * 8, in elements
  int dy_py, dy_px, dy_off;  // dy_off < 0: column past cout

  __device__ __forceinline__ void Init(const DwWideArgs& a, int tid, int co0) {
#pragma unroll
    for (int k = 0; k < kPre; ++k) {
      int idx = tid + k * kThreads;
      rc[k] = -1;
      off[k] = 0;
      if (idx < a.x_slots) {
        uint32_t rr = a.div_row_slots.div((uint32_t)idx);
        uint32_t j = a.div_row_slots.mod((uint32_t)idx, rr);
        uint32_t col = a.div_cpp.div(j);
        uint32_t ch = a.div_cpp.mod(j, col) ^ (col & (uint32_t)a.swz);
        int ih = (int)rr * a.gh, iw = (int)col * a.gw;
        rc[k] = ih | (iw << 12);
        off[k] = (ih * a.W + iw) * a.C + (int)ch * 8;
      }
    }
    int pix = tid >> 4;
    int ch = (tid & 15) ^ ((pix & 7) * 2);
    dy_py = pix >> a.lgpw;
    dy_px = pix & ((1 << a.lgpw) - 1);
    dy_off = co0 + ch * 8 < a.Cout
                 ? (dy_py * a.Q + dy_px) * a.Cout + ch * 8 : -1;
  }

  // c0, co0: first channel and first column of the block's slice
  __device__ __forceinline__ void Issue(const DwWideArgs& a, int step, int c0,
                                        int co0, uint16_t* xbuf,
                                        uint16_t* dybuf, int tid) const {
    uint32_t n = a.div_pp.div((uint32_t)step);
    uint32_t pp = a.div_pp.mod((uint32_t)step, n);
    uint32_t pyb = a.div_ppw.div(pp);
    int p0 = (int)pyb * (kK >> a.lgpw);
    int q0 = (int)a.div_ppw.mod(pp, pyb) << a.lgpw;
    int h0 = p0 * a.sh - a.ph, w0 = q0 * a.sw - a.pw;
    // element (h0, w0, c0) of image n; outside the image when padding is
    // hit, and then only added to, never read
    const uint16_t* origin =
        a.x + (((int64_t)n * a.H + h0) * a.W + w0) * a.C + c0;
#pragma unroll
    for (int k = 0; k < kPre; ++k) {
      if (k * kThreads < a.x_slots_pad) {
        const uint16_t* src = a.zero16;
        int h = h0 + (rc[k] & 0xfff), w = w0 + (rc[k] >> 12);
        if (rc[k] >= 0 && h >= 0 && h < a.H && w >= 0 && w < a.W)
          src = origin + off[k];
        Glds16(src, xbuf + (tid + k * kThreads - (tid & 63)) * 8);
      }
    }
    const uint16_t* src = a.zero16;
    if (dy_off >= 0 && p0 + dy_py < a.P && q0 + dy_px < a.Q)
      src = a.dy + (((int64_t)n * a.P + p0) * a.Q + q0) * a.Cout + co0 +
            dy_off;
    Glds16(src, dybuf + (tid & ~63) * 8);
  }
};

// TPW = row tiles per wave; wave (wr, wc) owns row tiles t*4 + wr. A tile
// past the slice's rows, and the column tiles of a half-empty cout slice, are
// computed on valid LDS and not stored: a branch around them would move the
// accumulators between register files.
template <int TPW>
__launch_bounds__(kThreads) __global__ void ConvDwWide(DwWideArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
  int tid = threadIdx.x;
  int lane = tid & 63;
  int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  int wr = wid & 3, wc = wid >> 2;
  int co_i = (int)a.div_cslices.div(blockIdx.y);
  int c0 = (int)a.div_cslices.mod(blockIdx.y, (uint32_t)co_i) * a.CS;
  int co0 = co_i * kCoutSlice;
  int buf_elems = (a.x_slots_pad + kDySlots) * 8;
  auto xbuf = [&](int b) { return lds + b * buf_elems; };
  auto dybuf = [&](int b) { return lds + b * buf_elems + a.x_slots_pad * 8; };

  // Step-invariant LDS offsets (in elements) of this lane's two reads per
  // fragment. A: rows = (tap, channel of the slice), k = pixel of the patch;
  // a 4-row run stays inside one tap and one chunk because CS % 8 == 0.
  int pwm = (1 << a.lgpw) - 1;
  int a_off[TPW][2];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    int row = (t * 4 + wr) * 16 + FragRow(lane);
    if (row >= a.rows) row = 0;  // rows past the slice: read anything valid
    uint32_t tap = a.div_cs.div((uint32_t)row);
    int ch = (int)a.div_cs.mod((uint32_t)row, tap);
    uint32_t fr = a.div_s.div(tap);
    int fs = (int)a.div_s.mod(tap, fr);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      int k = FragK(lane, h);
      int hrow = (k >> a.lgpw) * a.lh + (int)fr;
      int hcol = (k & pwm) * a.lw + fs;
      a_off[t][h] = ((hrow * a.hcols + hcol) * a.cpp +
                     ((ch >> 3) ^ (hcol & a.swz))) * 8 + (ch & 7);
    }
  }
  int b_off[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int col = (wc * 4 + j) * 16 + FragRow(lane);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      int pix = FragK(lane, h);
      b_off[j][h] = (pix * 16 + ((col >> 3) ^ ((pix & 7) * 2))) * 8 + (col & 7);
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
  // after the barrier of step t (their buffer was read in step t-1). Each
  // thread issues a.loads loads per step and they complete in order, so "at
  // most a.loads outstanding" means step t's have landed.
  Stager st;
  st.Init(a, tid, co0);
  st.Issue(a, step, c0, co0, xbuf(0), dybuf(0), tid);
  if (step + 1 < end) st.Issue(a, step + 1, c0, co0, xbuf(1), dybuf(1), tid);
  int cur = 0;
  for (; step < end; ++step) {
    WaitLoads(step + 1 < end ? a.loads : 0);
    __builtin_amdgcn_s_barrier();
    int nxt = cur == 0 ? 2 : cur - 1;
    if (step + 2 < end)
      st.Issue(a, step + 2, c0, co0, xbuf(nxt), dybuf(nxt), tid);
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
    for (int i = 0; i < 4; ++i) {
      int row = (t * 4 + wr) * 16 + (lane >> 4) * 4 + i;
      uint32_t tap = a.div_cs.div((uint32_t)row);
      // row of the whole dW: tap * C + channel
      int grow = (int)tap * a.C + c0 + (int)a.div_cs.mod((uint32_t)row, tap);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int col = co0 + (wc * 4 + j) * 16 + (lane & 15);
        if (row < a.rows && col < a.Cout)
          atomicAdd(a.dw + grow * a.Cout + col, acc[t][j][i]);
      }
    }
  }
}

int RoundUp(int64_t v, int to) { return (int)((v + to - 1) / to * to); }

// Host-side geometry; false when the gate does not hold.
bool MakeArgs(const StfConvGeom& g, DwWideArgs* a) {
  int64_t M = (int64_t)g.n * g.p * g.q;
  if (g.cout <= 0 || (g.cout % 64) != 0 || (g.c % 8) != 0 || (M % 64) != 0 ||
      M < 768 || stf_conv2d_dw_tall_ok(&g))
    return false;
  // patch: the fewest pixels covered, ties to the wider one
  int lgpw = 0;
  int64_t best = 0;
  for (int lg = 5; lg >= 3; --lg) {
    int pw = 1 << lg, ph = kK >> lg;
    int64_t cover = (int64_t)RoundUp(g.q, pw) * RoundUp(g.p, ph);
    if (lgpw == 0 || cover < best) { lgpw = lg; best = cover; }
  }
  int PW = 1 << lgpw, PH = kK >> lgpw;
  int lh = g.r == 1 ? 1 : g.sh, gh = g.r == 1 ? g.sh : 1;
  int lw = g.s == 1 ? 1 : g.sw, gw = g.s == 1 ? g.sw : 1;
  int64_t HR = (int64_t)(PH - 1) * lh + g.r, HC = (int64_t)(PW - 1) * lw + g.s;
  if (HR * gh >= (1 << 12) || HC * gw >= (1 << 12)) return false;
  // channel slice: the largest divisor of c that is a multiple of 8, keeps
  // the rows within 36 tiles and the three LDS buffers within 160 KiB
  int64_t rs = (int64_t)g.r * g.s;
  int CS = 0;
  int64_t x_slots = 0, x_slots_pad = 0;
  for (int cs = (int)(kMaxRows / rs < g.c ? kMaxRows / rs : g.c) & ~7; cs >= 8;
       cs -= 8) {
    if (g.c % cs) continue;
    x_slots = HR * HC * (cs / 8);
    x_slots_pad = RoundUp(x_slots, kThreads);
    if (kBufs * (x_slots_pad + kDySlots) * 16 <= kMaxLds) { CS = cs; break; }
  }
  if (CS == 0) return false;
  int pph = (g.p + PH - 1) / PH, ppw = (g.q + PW - 1) / PW;
  int64_t nsteps = (int64_t)g.n * pph * ppw;
  int64_t cslices = g.c / CS, coslices = (g.cout + kCoutSlice - 1) / kCoutSlice;
  // 32-bit step counter, in-image and in-patch element offsets, dW index
  if (nsteps >= (1ll << 31) || (int64_t)g.h * g.w * g.c >= (1ll << 31) ||
      (HR * gh + 1) * g.w * g.c >= (1ll << 31) ||
      (int64_t)(PH + 1) * g.q * g.cout >= (1ll << 31) ||
      rs * g.c * g.cout >= (1ll << 31) || cslices * coslices > 65535)
    return false;
  a->H = g.h; a->W = g.w; a->C = g.c; a->Cout = (int)g.cout; a->S = g.s;
  a->sh = g.sh; a->sw = g.sw; a->ph = g.ph; a->pw = g.pw;
  a->P = g.p; a->Q = g.q;
  a->CS = CS;
  a->cpp = CS / 8;
  int pow2 = a->cpp & -a->cpp;
  a->swz = (pow2 > 8 ? 8 : pow2) - 1;
  a->lgpw = lgpw;
  a->gh = gh; a->gw = gw; a->lh = lh; a->lw = lw;
  a->hcols = (int)HC;
  a->rows = (int)rs * CS;
  a->x_slots = (int)x_slots;
  a->x_slots_pad = (int)x_slots_pad;
  a->loads = (int)(x_slots_pad / kThreads) + 1;
  a->cslices = (int)cslices;
  a->coslices = (int)coslices;
  a->ppw = ppw; a->pph = pph;
  a->nsteps = (int)nsteps;
  a->div_row_slots.init((uint32_t)(HC * a->cpp));
  a->div_cpp.init((uint32_t)a->cpp);
  a->div_cs.init((uint32_t)CS);
  a->div_s.init((uint32_t)g.s);
  a->div_ppw.init((uint32_t)ppw);
  a->div_pp.init((uint32_t)(pph * ppw));
  a->div_cslices.init((uint32_t)cslices);
  return true;
}

size_t LdsBytes(const DwWideArgs& a) {
  return kBufs * (size_t)(a.x_slots_pad + kDySlots) * 16;
}

}  // namespace

extern "C" {

int stf_conv2d_dw_wide_ok(const StfConvGeom* g) {
  DwWideArgs a;
  return MakeArgs(*g, &a);
}

int stf_conv2d_dw_wide_plan(const StfConvGeom* g, int plan[6]) {
  DwWideArgs a;
  if (!MakeArgs(*g, &a)) return 0;
  plan[0] = a.CS;
  plan[1] = 1 << a.lgpw;
  plan[2] = kK >> a.lgpw;
  plan[3] = a.cslices;
  plan[4] = a.coslices;
  plan[5] = (int)LdsBytes(a);
  return 1;
}

hipError_t stf_conv2d_dw_wide(const void* x, const void* dy, void* dw_f32,
                              const void* zero16, const StfConvGeom* g,
                              hipStream_t stream) {
  DwWideArgs a;
  if (!MakeArgs(*g, &a)) return hipErrorInvalidValue;
  a.x = (const uint16_t*)x;
  a.dy = (const uint16_t*)dy;
  a.dw = (float*)dw_f32;
  a.zero16 = (const uint16_t*)zero16;
  // slices x step blocks, about one block per CU in all, each block on a
  // contiguous range of steps
  int slices = a.cslices * a.coslices;
  int blocks = (STF_NUM_CU + slices / 2) / slices;
  if (blocks < 1) blocks = 1;
  if (blocks > a.nsteps) blocks = a.nsteps;
  a.per_block = (a.nsteps + blocks - 1) / blocks;
  blocks = (a.nsteps + a.per_block - 1) / a.per_block;
  int tpw = ((a.rows + 15) / 16 + 3) / 4;
  auto launch = [&](auto tpw_c) {
    constexpr int TPW = decltype(tpw_c)::value;
    hipLaunchKernelGGL(ConvDwWide<TPW>,
                       dim3((uint32_t)blocks, (uint32_t)slices),
                       dim3(kThreads), LdsBytes(a), stream, a);
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

}  // extern "C"
