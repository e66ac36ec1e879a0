// Quantized depthwise conv: one tiled kernel family DwQ8<VEC, K, EPI>. NHWC
// quint8 x, [R][S][C][mult] quint8 filter, output channel cm = c*mult + m,
// qint32 out (EPI = kI32) or bias + activation + requantize to quint8 (EPI =
// a stf::QuantActivation). Bit-equal to kernels/cpu_quantized.cc: integer
// sums modulo 2^32 and the one f32 formula of kernels/quantized_util.h.
//
// Depthwise has no contraction over channels, so no MFMA. At one byte per
// element the op is no longer bound by HBM alone: a loop that unpacks bytes
// and multiplies them one by one spends two or more VALU instructions per
// multiply-add. The design reads x once and spends one VALU instruction per
// multiply-add on the common path.
//
// Work split. 256 threads. A block owns a slice of 64 output channels and a
// patch of tp x TQ output pixels of one image (TQ = 8 or 16, tp up to
// 128 / TQ; the host halves tp until the block's LDS fits kLdsBudget). Lanes
// are channel-fastest. VEC = 4: 16 channel lanes, each a group of 4 channels
// = one dword of x per pixel, and 16 pixel lanes. VEC = 1: 64 channel lanes
// of one output channel, 4 pixel lanes. A thread computes runs of 4 outputs
// along q. The block index is decoded once per block; pixels are walked with
// shifts and carry counters, no division per element.
//
// LDS. The x halo, ((tp-1)*sh + R) x ((TQ-1)*sw + S) pixels of the slice's
// 64 input bytes, is staged as raw bytes (16-byte global loads when C % 16
// == 0, dwords when C % 4 == 0, bytes otherwise), zero wherever the halo
// leaves the image or the slice leaves the channels: the tap loops carry no
// bounds checks, partial patches and the last slice are masked at the stores
// only. A staged pixel is `pitch` dwords, 16 of data and a pad. A wave of
// VEC = 4 holds 4 pixel lanes whose runs start 4*sw pixels apart, each
// reading 16 consecutive dwords; the host picks the smallest pitch >= 16 with
// 4*sw*pitch = 16 or 48 (mod 64), which puts the four groups on four
// disjoint sets of 16 banks (pitch 20 for sw 1, 18 for sw 2; 17 where no
// such pitch exists). This assumes 64 LDS banks of 4 bytes; with 32 banks
// the same pitch keeps the two groups of a half-wave apart. VEC = 1 reads 64
// consecutive bytes of one pixel per wave.
// Behind the halo: w32[R*S][64], the filter slice as int32 w' = w - z_w, and
// wpk[(R*S+1)/2][64], taps (2i, 2i+1) of a channel as two int16 in a dword
// (an odd tap count pads with 0).
// kLdsBudget = 64 KiB, so at least two blocks fit a CU's 160 KiB. TQ = 16:
//   3x3 stride 1, tp 8   10*18*80 + 9*256 + 5*256   = 17.6 KiB
//   3x3 stride 2, tp 8   17*33*72 + 14*256          = 42.9 KiB
//   5x5 stride 1, tp 8   12*20*80 + 25*256 + 13*256 = 28.3 KiB
//
// Inner loop (VEC = 4, z_w narrow). Two x dwords, taps t and t+1 of the
// lane's 4 channels, feed four v_perm_b32 that build [0, x_{t+1}, 0, x_t]
// per channel (selector byte 0x0c inserts the zeros), then four
// v_dot2_i32_i16 against the packed w' pairs: 8 instructions, 8 exact
// multiply-adds, with the raw unsigned x. K = 1 and K = 2 (3x3, sw = K)
// hold the 5 pair dwords per channel (20 VGPRs) and the three
// ((4-1)*K + 3)-wide row windows in registers for the whole run; K = 0 takes
// any filter and stride with pairs and x read from LDS.
//
// Zero point of x. acc = sum_halo x*w' - z_x * sum_{taps in the image} w'.
// The zero fill makes the first sum right everywhere. The second factor is
// the full per-channel filter sum (VEC registers) for an interior pixel, and
// the sum over the in-image tap rectangle [r0,r1) x [s0,s1), read from w32,
// for a border pixel; only border pixels run that loop. The multiply by z_x
// is unsigned, so it wraps as the CPU's int64 -> int32 truncation does.
//
// Wide zero points. z_w comes from device scalars. When some w - z_w could
// leave int16 (z_w outside [-32512, 32768]) the launch takes the generic
// path instead: one 32-bit multiply-add per byte against w32. The test is
// uniform over the launch; both paths are in every VEC = 4 kernel. VEC = 1
// (mult > 1, C % 4 != 0 or unaligned bases) always runs the generic path.
//
// Epilogue. kI32 stores the accumulators (16 bytes per VEC = 4 lane). The
// fused forms build QuantFusedScale once per thread from the device scalars,
// read bias[cm] once, apply QuantFusedU8<ACT> and store one dword per lane
// and pixel. Thread 0 of block 0 writes min_out / max_out. An empty output
// runs one block that writes the two range scalars and nothing else.
//
// Offsets: a 64-bit image base per block plus 32-bit offsets inside one
// image; stf_depthwise_q8_ok is the guard.
//
// VGPRs (hipcc -O3, gfx950; each VEC = 4 kernel holds both zero-point
// paths), kI32 / None / Relu / Relu6: VEC 4, K 1 and K 2: 124 / 136 / 136 /
// 128; VEC 4, K 0: 106 / 116 / 116 / 122; VEC 1, K 0: 34 / 37 / 37 / 37. No
// spills, no scratch; every multiply-add of the narrow path is one
// v_perm_b32 and one v_dot2c_i32_i16. Dynamic LDS as listed above. Measured
// times are in profiles/quantized_depthwise.md: the kernel is 8 to 29 times
// faster than the float chain it replaces and still slower than the f32
// depthwise kernel at the stride-1 layers; TODO.md lists what is suspected.
#include <algorithm>
#include <climits>

#include "hip_common.h"
#include "kernels/quantized_util.h"
#include "stf_kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSlice = 64;             // output channels and x bytes of a block
constexpr int kRun = 4;                // outputs per thread along q
constexpr int kLdsBudget = 64 * 1024;  // bytes per block
constexpr int kI32 = -1;               // EPI: qint32 out

using i16x2 = __attribute__((ext_vector_type(2))) short;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

struct Params {
  const uint8_t* x;
  const uint8_t* w;
  const float* bias;
  const float *min_x, *max_x, *min_w, *max_w, *req_min, *req_max;
  void* y;
  float *min_out, *max_out;
  int h, w_, c;    // one image of x
  int oh, ow, cm;  // one image of y; cm = c * mult
  int r, s, sh, sw, ph, pw, mult;
  int tp, tql;     // patch: tp rows of 1 << tql pixels
  int hr, hc;      // staged rows and columns of x
  int pitch;       // dwords per staged pixel
  int xdw;         // dwords of the staged halo, a multiple of 4
  int prs, pcs, slices;
  int blocks;      // 0: an empty output, one block writes the ranges
  int ld16;        // VEC 4: stage with 16-byte loads
};

extern __shared__ u32x4 dw_q8_smem[];

// The x halo: rows x cols pixels from (row0, col0) of the image, 64 bytes
// from channel c_lo each, zeros outside the image and past channel c.
template <int VEC>
__device__ __forceinline__ void StageX(uint32_t* xs, const uint8_t* img,
                                       int row0, int col0, const Params& p,
                                       int c_lo, int tid) {
  const int npix = p.hr * p.hc;
  if (VEC == 4 && p.ld16) {
    int pix = tid >> 2, ch = tid & 3;
    int row = pix / p.hc, col = pix - row * p.hc;
    for (; pix < npix; pix += kThreads / 4) {
      int ih = row0 + row, iw = col0 + col, cc = c_lo + ch * 16;
      u32x4 v = {0u, 0u, 0u, 0u};
      if ((unsigned)ih < (unsigned)p.h && (unsigned)iw < (unsigned)p.w_ &&
          cc < p.c)
        v = *reinterpret_cast<const u32x4*>(img + ((ih * p.w_ + iw) * p.c + cc));
      uint32_t* d = xs + pix * p.pitch + ch * 4;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      col += kThreads / 4;
      while (col >= p.hc) { col -= p.hc; ++row; }
    }
  } else {
    int pix = tid >> 4, ch = tid & 15;
    int row = pix / p.hc, col = pix - row * p.hc;
    for (; pix < npix; pix += kThreads / 16) {
      int ih = row0 + row, iw = col0 + col, cc = c_lo + ch * 4;
      uint32_t v = 0;
      if ((unsigned)ih < (unsigned)p.h && (unsigned)iw < (unsigned)p.w_) {
        const uint8_t* g = img + ((ih * p.w_ + iw) * p.c + cc);
        if constexpr (VEC == 4) {
          if (cc < p.c) v = *reinterpret_cast<const uint32_t*>(g);
        } else {
#pragma unroll
          for (int b = 0; b < 4; ++b)
            if (cc + b < p.c) v |= (uint32_t)g[b] << (8 * b);
        }
      }
      xs[pix * p.pitch + ch] = v;
      col += kThreads / 16;
      while (col >= p.hc) { col -= p.hc; ++row; }
    }
  }
}

// [0, b_j, 0, a_j]: byte j of a and of b as two u16.
template <int J>
__device__ __forceinline__ uint32_t BytePair(uint32_t a, uint32_t b) {
  return __builtin_amdgcn_perm(b, a, 0x0c000c00u | J | ((4u + J) << 16));
}

__device__ __forceinline__ uint32_t Dot2(uint32_t xpair, uint32_t wpair,
                                         uint32_t acc) {
  return (uint32_t)__builtin_amdgcn_sdot2(__builtin_bit_cast(i16x2, xpair),
                                          __builtin_bit_cast(i16x2, wpair),
                                          (int)acc, false);
}

// The four channels of x dwords a (tap t) and b (tap t + 1) against the four
// packed pairs wp.
__device__ __forceinline__ void PairMac(uint32_t (&acc)[4], uint32_t a,
                                        uint32_t b, const uint32_t (&wp)[4]) {
  acc[0] = Dot2(BytePair<0>(a, b), wp[0], acc[0]);
  acc[1] = Dot2(BytePair<1>(a, b), wp[1], acc[1]);
  acc[2] = Dot2(BytePair<2>(a, b), wp[2], acc[2]);
  acc[3] = Dot2(BytePair<3>(a, b), wp[3], acc[3]);
}

// K: 0 any filter; 1 / 2: 3x3 with sw = K, pairs and row windows in
// registers. EPI: kI32 or a stf::QuantActivation.
template <int VEC, int K, int EPI>
__global__ __launch_bounds__(kThreads) void DwQ8(Params p) {
  static_assert(VEC == 4 || K == 0, "register taps need the dword lanes");
  constexpr int kCL = kSlice / VEC, kPL = kThreads / kCL;
  const int tid = threadIdx.x;
  const float mnx = p.min_x[0], mxx = p.max_x[0];
  const float mnw = p.min_w[0], mxw = p.max_w[0];
  stf::QuantFusedScale sc = {};
  if constexpr (EPI != kI32)
    sc = stf::MakeQuantFusedScale(mnx, mxx, mnw, mxw, p.req_min[0],
                                  p.req_max[0]);
  if (blockIdx.x == 0 && tid == 0) {
    if constexpr (EPI == kI32) {
      float sx = stf::QuantStep(mnx, mxx), sf = stf::QuantStep(mnw, mxw);
      p.min_out[0] = stf::QuantProductMin(sx, sf);
      p.max_out[0] = stf::QuantProductMax(sx, sf);
    } else {
      p.min_out[0] = sc.mn;
      p.max_out[0] = sc.mx;
    }
  }
  if (p.blocks == 0) return;
  const int32_t zx = stf::QuantZeroPoint(mnx, mxx);
  const int32_t zw = stf::QuantZeroPoint(mnw, mxw);
  // every w - z_w, w in 0..255, is an int16
  const bool narrow = VEC == 4 && zw >= -32512 && zw <= 32768;

  uint32_t* xs = reinterpret_cast<uint32_t*>(dw_q8_smem);
  uint32_t* w32 = xs + p.xdw;
  const int rs = p.r * p.s, npairs = (rs + 1) >> 1;
  uint32_t* wpk = w32 + rs * kSlice;

  int bid = blockIdx.x;
  int slice = bid % p.slices; bid /= p.slices;
  int pc = bid % p.pcs; bid /= p.pcs;
  int pr = bid % p.prs;
  int n = bid / p.prs;
  const int cm0 = slice * kSlice, c_lo = cm0 / p.mult;
  const int p0 = pr * p.tp, q0 = pc << p.tql;

  StageX<VEC>(xs, p.x + (int64_t)n * p.h * p.w_ * p.c, p0 * p.sh - p.ph,
              q0 * p.sw - p.pw, p, c_lo, tid);
  for (int i = tid; i < rs * kSlice; i += kThreads) {
    int t = i >> 6, ch = cm0 + (i & 63);
    w32[i] = ch < p.cm ? (uint32_t)((int32_t)p.w[t * p.cm + ch] - zw) : 0u;
  }
  if (VEC == 4)
    for (int i = tid; i < npairs * kSlice; i += kThreads) {
      int t = (i >> 6) * 2, ch = cm0 + (i & 63);
      uint32_t lo = 0, hi = 0;
      if (ch < p.cm) {
        lo = (uint32_t)((int32_t)p.w[t * p.cm + ch] - zw);
        if (t + 1 < rs) hi = (uint32_t)((int32_t)p.w[(t + 1) * p.cm + ch] - zw);
      }
      wpk[i] = (lo & 0xffffu) | (hi << 16);
    }
  __syncthreads();

  const int cl = tid % kCL, pl = tid / kCL;
  const int mycm = cm0 + cl * VEC;
  // VEC 4: this lane's dword of a staged pixel. VEC 1: its byte; tail lanes
  // read byte 0.
  const int xoff = VEC == 4 ? cl : (mycm < p.cm ? mycm / p.mult - c_lo : 0);
  const uint8_t* xb = reinterpret_cast<const uint8_t*>(xs);
  const uint32_t* wme = w32 + cl * VEC;

  uint32_t wfull[VEC];  // the whole filter's sum of w'
#pragma unroll
  for (int j = 0; j < VEC; ++j) wfull[j] = 0;
  for (int t = 0; t < rs; ++t)
#pragma unroll
    for (int j = 0; j < VEC; ++j) wfull[j] += wme[t * kSlice + j];

  uint32_t wreg[K ? 5 : 1][4];
  if constexpr (K != 0) {
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      u32x4 v = *reinterpret_cast<const u32x4*>(wpk + i * kSlice + cl * 4);
      wreg[i][0] = v.x; wreg[i][1] = v.y; wreg[i][2] = v.z; wreg[i][3] = v.w;
    }
  }
  float bias[VEC];
  if constexpr (EPI != kI32) {
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      bias[j] = mycm + j < p.cm ? p.bias[mycm + j] : 0.f;
  }

  const int gl = p.tql - 2;  // log2 of the runs per patch row
  const int units = p.tp << gl;
  const int64_t ybase = (int64_t)n * p.oh * p.ow * p.cm;
  for (int u = pl; u < units; u += kPL) {
    const int ty = u >> gl, tx = (u & ((1 << gl) - 1)) * kRun;
    const int bpix = (ty * p.sh) * p.hc + tx * p.sw;
    uint32_t acc[kRun][VEC];
#pragma unroll
    for (int o = 0; o < kRun; ++o)
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[o][j] = 0;

    if (narrow) {
      if constexpr (VEC == 4 && K != 0) {
        constexpr int kWin = (kRun - 1) * K + 3;
        uint32_t win[3][kWin];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int j = 0; j < kWin; ++j)
            win[r][j] = xs[(bpix + r * p.hc + j) * p.pitch + xoff];
#pragma unroll
        for (int o = 0; o < kRun; ++o)
#pragma unroll
          for (int i = 0; i < 5; ++i) {
            constexpr int kNone = 9;
            const int ta = 2 * i, tb = 2 * i + 1;
            uint32_t a = win[ta / 3][o * K + ta % 3];
            uint32_t b = tb < kNone ? win[(tb % kNone) / 3][o * K + tb % 3] : 0u;
            PairMac(acc[o], a, b, wreg[i]);
          }
      } else if constexpr (VEC == 4) {
        int ra = 0, sa = 0;
        for (int i = 0; i < npairs; ++i) {
          int rb = ra, sb = sa + 1;
          if (sb == p.s) { sb = 0; ++rb; }
          const bool has_b = rb < p.r;
          u32x4 v = *reinterpret_cast<const u32x4*>(wpk + i * kSlice + cl * 4);
          const uint32_t wp[4] = {v.x, v.y, v.z, v.w};
          const int pa = bpix + ra * p.hc + sa;
          const int pb = has_b ? bpix + rb * p.hc + sb : pa;
#pragma unroll
          for (int o = 0; o < kRun; ++o) {
            uint32_t a = xs[(pa + o * p.sw) * p.pitch + xoff];
            uint32_t b = xs[(pb + o * p.sw) * p.pitch + xoff];
            PairMac(acc[o], a, has_b ? b : 0u, wp);
          }
          sa = sb + 1; ra = rb;
          if (sa == p.s) { sa = 0; ++ra; }
        }
      }
    } else {
      int t = 0;
      for (int r = 0; r < p.r; ++r)
        for (int s = 0; s < p.s; ++s, ++t) {
          uint32_t wv[VEC];
#pragma unroll
          for (int j = 0; j < VEC; ++j) wv[j] = wme[t * kSlice + j];
          const int pa = bpix + r * p.hc + s;
#pragma unroll
          for (int o = 0; o < kRun; ++o) {
            if constexpr (VEC == 4) {
              uint32_t a = xs[(pa + o * p.sw) * p.pitch + xoff];
#pragma unroll
              for (int j = 0; j < 4; ++j)
                acc[o][j] += ((a >> (8 * j)) & 255u) * wv[j];
            } else {
              acc[o][0] +=
                  (uint32_t)xb[(pa + o * p.sw) * p.pitch * 4 + xoff] * wv[0];
            }
          }
        }
    }

    const int py = p0 + ty;
    const int ih0 = py * p.sh - p.ph;
    const int r0 = max(0, -ih0), r1 = min(p.r, p.h - ih0);
#pragma unroll
    for (int o = 0; o < kRun; ++o) {
      const int qx = q0 + tx + o;
      const int iw0 = qx * p.sw - p.pw;
      const int s0 = max(0, -iw0), s1 = min(p.s, p.w_ - iw0);
      uint32_t ws[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) ws[j] = wfull[j];
      if (r0 != 0 || r1 != p.r || s0 != 0 || s1 != p.s) {  // a border pixel
#pragma unroll
        for (int j = 0; j < VEC; ++j) ws[j] = 0;
        for (int r = r0; r < r1; ++r)
          for (int s = s0; s < s1; ++s)
#pragma unroll
            for (int j = 0; j < VEC; ++j)
              ws[j] += wme[(r * p.s + s) * kSlice + j];
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[o][j] -= (uint32_t)zx * ws[j];
      if (py >= p.oh || qx >= p.ow || mycm >= p.cm) continue;
      const int off = (py * p.ow + qx) * p.cm + mycm;
      if constexpr (EPI == kI32) {
        uint32_t* y = reinterpret_cast<uint32_t*>(p.y) + ybase + off;
        if constexpr (VEC == 4) {
          u32x4 v = {acc[o][0], acc[o][1], acc[o][2], acc[o][3]};
          *reinterpret_cast<u32x4*>(y) = v;
        } else {
          *y = acc[o][0];
        }
      } else {
        uint8_t* y = reinterpret_cast<uint8_t*>(p.y) + ybase + off;
        uint32_t q[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          q[j] = stf::QuantFusedU8<EPI>((int32_t)acc[o][j], bias[j], sc);
        if constexpr (VEC == 4)
          *reinterpret_cast<uint32_t*>(y) =
              q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
        else
          *y = (uint8_t)q[0];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
bool Aligned16(const void* ptr) { return ((uintptr_t)ptr & 15) == 0; }

int64_t CeilDiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The smallest pitch >= 16 dwords that spreads the four pixel lanes of a
// wave, kRun * sw pixels apart, over disjoint sets of 16 banks; 17 if none.
int PickPitch(int sw) {
  for (int pitch = 16; pitch < 32; ++pitch) {
    int64_t m = ((int64_t)kRun * sw * pitch) % 64;
    if (m == 16 || m == 48) return pitch;
  }
  return 17;
}

// Patch, halo and LDS size; false when a count leaves an int or one patch
// row's halo with the filter slice does not fit kLdsBudget.
bool PickTile(const StfConvGeom& g, int mult, Params* p, size_t* lds) {
  const int64_t lim = INT_MAX - 64;
  if (mult < 1 || g.r < 1 || g.s < 1 || g.sh < 1 || g.sw < 1 || g.n < 0 ||
      g.h < 0 || g.w < 0 || g.c < 0 || g.p < 0 || g.q < 0)
    return false;
  int64_t cm = (int64_t)g.c * mult, rs = (int64_t)g.r * g.s;
  if (cm > lim || (int64_t)g.h * g.w * g.c > lim ||
      (int64_t)g.p * g.q * cm > lim || rs > lim || rs * cm > lim)
    return false;
  p->h = g.h; p->w_ = g.w; p->c = g.c;
  p->oh = g.p; p->ow = g.q; p->cm = (int)cm;
  p->r = g.r; p->s = g.s; p->sh = g.sh; p->sw = g.sw;
  p->ph = g.ph; p->pw = g.pw; p->mult = mult;
  p->slices = (int)CeilDiv(cm, kSlice);
  p->tql = g.q <= 8 ? 3 : 4;
  p->pitch = PickPitch(g.sw);
  int tq = 1 << p->tql;
  int64_t tp = std::max(1, std::min(128 / tq, g.p));
  int64_t wdw = (rs + (rs + 1) / 2) * kSlice;
  for (;; tp /= 2) {
    int64_t hr = (tp - 1) * g.sh + g.r;
    int64_t hc = (int64_t)(tq - 1) * g.sw + g.s;
    int64_t xdw = (hr * hc * p->pitch + 3) & ~int64_t(3);
    if ((xdw + wdw) * 4 <= kLdsBudget) {
      p->tp = (int)tp; p->hr = (int)hr; p->hc = (int)hc; p->xdw = (int)xdw;
      *lds = (size_t)(xdw + wdw) * 4;
      break;
    }
    if (tp == 1) return false;
  }
  p->prs = (int)CeilDiv(g.p, p->tp);
  p->pcs = (int)CeilDiv(g.q, tq);
  int64_t blocks = (int64_t)g.n * p->prs * p->pcs * p->slices;
  if (blocks > lim) return false;  // gridDim.x
  p->blocks = (int)blocks;
  return true;
}

template <int VEC, int EPI>
void LaunchK(const Params& p, size_t lds, hipStream_t stream) {
  dim3 grid((uint32_t)std::max(1, p.blocks)), block(kThreads);
  if constexpr (VEC == 4) {
    if (p.r == 3 && p.s == 3 && p.sw == 1) {
      hipLaunchKernelGGL((DwQ8<4, 1, EPI>), grid, block, lds, stream, p);
      return;
    }
    if (p.r == 3 && p.s == 3 && p.sw == 2) {
      hipLaunchKernelGGL((DwQ8<4, 2, EPI>), grid, block, lds, stream, p);
      return;
    }
  }
  hipLaunchKernelGGL((DwQ8<VEC, 0, EPI>), grid, block, lds, stream, p);
}

template <int EPI>
hipError_t Launch(Params& p, const StfConvGeom* g, int mult,
                  hipStream_t stream) {
  size_t lds;
  if (!PickTile(*g, mult, &p, &lds)) return hipErrorInvalidValue;
  bool vec = mult == 1 && g->c % 4 == 0 && Aligned16(p.x) && Aligned16(p.y);
  p.ld16 = vec && g->c % 16 == 0;
  if (vec) LaunchK<4, EPI>(p, lds, stream);
  else LaunchK<1, EPI>(p, lds, stream);
  return hipGetLastError();
}

}  // namespace

extern "C" int stf_depthwise_q8_ok(const StfConvGeom* g, int mult) {
  Params p;
  size_t lds;
  return PickTile(*g, mult, &p, &lds);
}

extern "C" hipError_t stf_depthwise_q8_i32(
    const void* x, const void* w, const float* min_x, const float* max_x,
    const float* min_w, const float* max_w, int32_t* y, float* min_out,
    float* max_out, const StfConvGeom* g, int mult, hipStream_t stream) {
  Params p = {};
  p.x = (const uint8_t*)x; p.w = (const uint8_t*)w;
  p.min_x = min_x; p.max_x = max_x; p.min_w = min_w; p.max_w = max_w;
  p.y = y; p.min_out = min_out; p.max_out = max_out;
  return Launch<kI32>(p, g, mult, stream);
}

extern "C" hipError_t stf_depthwise_q8_fused(
    const void* x, const void* w, const float* bias, const float* min_x,
    const float* max_x, const float* min_w, const float* max_w,
    const float* req_min, const float* req_max, int activation, uint8_t* y,
    float* min_out, float* max_out, const StfConvGeom* g, int mult,
    hipStream_t stream) {
  Params p = {};
  p.x = (const uint8_t*)x; p.w = (const uint8_t*)w; p.bias = bias;
  p.min_x = min_x; p.max_x = max_x; p.min_w = min_w; p.max_w = max_w;
  p.req_min = req_min; p.req_max = req_max;
  p.y = y; p.min_out = min_out; p.max_out = max_out;
  switch (activation) {
    case stf::kQuantActNone:
      return Launch<stf::kQuantActNone>(p, g, mult, stream);
    case stf::kQuantActRelu:
      return Launch<stf::kQuantActRelu>(p, g, mult, stream);
    case stf::kQuantActRelu6:
      return Launch<stf::kQuantActRelu6>(p, g, mult, stream);
  }
  return hipErrorInvalidValue;
}
