// float32 depthwise conv, backprop-input and backprop-filter: one tiled
// kernel family DwF32<MODE, VEC, K>. NHWC x and dy, [R][S][C][mult] filter,
// output channel cm = c*mult + m.
//
// Depthwise has no contraction over channels: an output is R*S FMAs on its
// own channel, there is no matrix to feed an MFMA, and the op is bound by
// HBM bandwidth. So no matrix instructions here. The design is about reading
// x (or dy) from HBM once, moving 16 bytes per lane along the channel axis,
// and keeping index arithmetic and atomics out of the per-element work.
//
// Work split. 256 threads. A block owns a slice of 32 channels and a patch of
// tp x TQ pixels of one image (TQ = 8 or 16, tp up to 128 / TQ; the host
// shrinks tp until the block's LDS fits kLdsBudget). Lanes are channel-fastest:
// VEC = 4 has 8 channel lanes of one quad each and 32 pixel lanes, VEC = 1 has
// 32 channel lanes and 8 pixel lanes. Consecutive lanes so touch consecutive
// 16-byte (4-byte) chunks both in global memory and in LDS, where a pixel is
// 32 floats: no bank conflicts at stride 1. The block index is decoded to
// (image, patch, slice) once per block (per patch in DW); a thread walks its
// pixels with shifts and a carry counter, never a division per element.
//
// LDS. Stage() copies the patch's input halo, hr x hc pixels of the slice,
// with zeros wherever the halo leaves the image (SAME padding, partial
// patches) or the slice leaves the channels, so the inner loops have no
// bounds checks; edge patches and the last slice are masked at the stores
// only. The filter slice is staged once per block by the same routine, as a
// 1 x R*S image.
//
//   FWD  halo ((tp-1)*sh + R) x ((TQ-1)*sw + S) of x; a thread computes a run
//        of 4 outputs along q for its channel quad. K = 1 (3x3, sw 1) and
//        K = 2 (3x3, sw 2) hold the 9 taps in registers and load the
//        (3*sw + 3)-wide input window of a filter row from LDS once for the
//        whole run; K = 0 takes any filter and stride with the taps read from
//        LDS. Stride-1 DX with mult 1 is this kernel over dy with the filter
//        flipped and the padding R-1-ph, S-1-pw.
//   DX   (any stride, any mult) the block owns a patch of dx pixels and stages
//        the dy pixels they touch, ((tp+R-2)/sh + 2) x ((TQ+S-2)/sw + 2).
//        A thread derives its first tap (ih+ph) % sh and the dy row of that
//        tap once per pixel, then steps taps by the stride and dy rows by -1:
//        only taps of the right phase, no % in the loops. Sums over m.
//   DW   persistent blocks: grid = slices x workers, a worker loops over its
//        patches, staging the x halo and the dy patch. A thread owns a channel
//        quad and every 32nd (8th) pixel of the patch and keeps K taps x VEC
//        partial sums in registers across all its patches: K = 9 (36 VGPRs at
//        VEC 4) or K = 25 (100). That is the register budget: a filter with
//        more than 25 taps makes ceil(R*S / 25) passes over its patches. At
//        the end the pixel lanes of a wave are reduced with shuffles, the four
//        waves through LDS, and the block issues one store (one worker) or
//        one atomicAdd (several; the caller zero-fills) per filter element.
//
// VEC = 4 needs mult == 1, C % 4 == 0 and 16-byte aligned bases. VEC = 1 is
// the same code with a lane per output channel, its x channel cm / mult
// computed once per thread; it takes every other shape.
//
// Offsets: a 64-bit image base per block plus 32-bit offsets inside one image;
// stf_depthwise_f32_ok is the guard.
//
// LDS budget per block: kLdsBudget = 64 KiB, so at least two blocks fit a
// CU's 160 KiB. A staged pixel is 128 bytes; TQ = 16:
//   FWD 3x3 stride 1, tp 8   (10*18 + 9) * 128           = 23.6 KiB
//   FWD 3x3 stride 2, tp 4   ( 9*33 + 9) * 128           = 38.3 KiB
//                            (tp 8 would need 17*33*128 = 70 KiB)
//   FWD 5x5 stride 1, tp 8   (12*20 + 25) * 128          = 33.1 KiB
//   DX  3x3 stride 2, tp 8   ( 6*10 + 9) * 128           =  8.6 KiB
//   DW  3x3 stride 1, tp 8   (10*18 + 8*16) * 128        = 38.5 KiB
//   DW  3x3 stride 2, tp 4   ( 9*33 + 4*16) * 128        = 45.1 KiB
//   DW  5x5 stride 1, tp 8   (12*20 + 8*16) * 128        = 46.0 KiB
// DW's reduction buffer (4 waves x taps x 32 floats, 12.5 KiB at 25 taps)
// reuses the tiles. VGPR counts are in profiles/depthwise_f32.md.
#include <algorithm>
#include <climits>

#include "hip_common.h"
#include "stf_kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSlice = 32;             // channels of a block, floats per pixel
constexpr int kRun = 4;                // FWD outputs per thread along q
constexpr int kLdsBudget = 64 * 1024;  // bytes per block
constexpr int kMaxTapsInRegs = 25;     // DW accumulator budget

enum Mode { FWD = 0, DX = 1, DW = 2 };

struct Params {
  const float* a;  // staged with a halo: FWD x, DX dy, DW x
  const float* b;  // FWD w, DX w, DW dy
  float* out;      // FWD y, DX dx, DW dw
  int ah, aw, ac;  // one image of a
  int oh, ow, oc;  // one image of out (FWD, DX) or of dy (DW)
  int r, s, sh, sw, ph, pw, mult;
  int cm;          // c * mult, the filter's channel extent
  int flip;        // FWD: tap t reads filter tap r*s - 1 - t
  int tp, tql;     // patch: tp rows of 1 << tql pixels
  int hr, hc;      // staged rows and columns of a
  int pitch;       // floats per staged pixel of a (DX: and of the filter)
  int csl;         // DX: input channels per slice
  int prs, pcs, slices;  // patches down and across an image, channel slices
  int npatch;            // DW: n * prs * pcs
  int workers;           // DW
};

template <int VEC>
struct Vec {
  float v[VEC];
};

template <int VEC>
__device__ __forceinline__ Vec<VEC> Zero() {
  Vec<VEC> r;
#pragma unroll
  for (int i = 0; i < VEC; ++i) r.v[i] = 0.f;
  return r;
}

template <int VEC>
__device__ __forceinline__ Vec<VEC> Ld(const float* p) {
  Vec<VEC> r;
  if constexpr (VEC == 4) {
    f32x4 t = *reinterpret_cast<const f32x4*>(p);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int VEC>
__device__ __forceinline__ void St(float* p, const Vec<VEC>& a) {
  if constexpr (VEC == 4) {
    f32x4 t = {a.v[0], a.v[1], a.v[2], a.v[3]};
    *reinterpret_cast<f32x4*>(p) = t;
  } else {
    *p = a.v[0];
  }
}

template <int VEC>
__device__ __forceinline__ void Fma(Vec<VEC>& acc, const Vec<VEC>& a,
                                    const Vec<VEC>& b) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc.v[i] = fmaf(a.v[i], b.v[i], acc.v[i]);
}

// Thread layout: cl is the channel lane, pl the pixel lane.
template <int VEC>
struct Lanes {
  static constexpr int kCL = kSlice / VEC;
  static constexpr int kPL = kThreads / kCL;
};

// Copies rows x cols pixels starting at (row0, col0) of the h x w x c image
// `src`, channels [c_lo, c_lo + pitch), to dst[pixel][pitch]; zeros outside
// the image and past channel c. VEC 4: c, c_lo and pitch are multiples of 4.
template <int VEC>
__device__ __forceinline__ void Stage(float* dst, const float* src, int row0,
                                      int col0, int rows, int cols, int h,
                                      int w, int c, int c_lo, int pitch,
                                      int cl, int pl) {
  constexpr int kCL = Lanes<VEC>::kCL, kPL = Lanes<VEC>::kPL;
  int npix = rows * cols;
  int row = pl / cols, col = pl - row * cols;
  for (int i = pl; i < npix; i += kPL) {
    int ih = row0 + row, iw = col0 + col;
    bool in = (unsigned)ih < (unsigned)h && (unsigned)iw < (unsigned)w;
    const float* g = src + ((ih * w + iw) * c + c_lo);  // read only if `in`
    float* d = dst + i * pitch;
    for (int ch = cl * VEC; ch < pitch; ch += kCL * VEC) {
      Vec<VEC> v = Zero<VEC>();
      if (in && c_lo + ch < c) v = Ld<VEC>(g + ch);
      St<VEC>(d + ch, v);
    }
    col += kPL;
    while (col >= cols) { col -= cols; ++row; }
  }
}

// floor(a / b), b > 0
__device__ __forceinline__ int FloorDiv(int a, int b) {
  return a >= 0 ? a / b : -((b - 1 - a) / b);
}

extern __shared__ f32x4 dw_f32_smem[];

// K: 0 any filter; 1 / 2: 3x3 with sw = K, taps and row window in registers.
template <int VEC, int K>
__device__ __forceinline__ void Forward(const Params& p) {
  constexpr int kCL = Lanes<VEC>::kCL, kPL = Lanes<VEC>::kPL;
  float* xs = reinterpret_cast<float*>(dw_f32_smem);
  float* wl = xs + p.hr * p.hc * kSlice;
  int cl = threadIdx.x % kCL, pl = threadIdx.x / kCL;
  int bid = blockIdx.x;
  int slice = bid % p.slices; bid /= p.slices;
  int pc = bid % p.pcs; bid /= p.pcs;
  int pr = bid % p.prs;
  int n = bid / p.prs;
  int cm0 = slice * kSlice, c_lo = cm0 / p.mult;
  int p0 = pr * p.tp, q0 = pc << p.tql;
  int rs = p.r * p.s;
  Stage<VEC>(xs, p.a + (int64_t)n * p.ah * p.aw * p.ac, p0 * p.sh - p.ph,
             q0 * p.sw - p.pw, p.hr, p.hc, p.ah, p.aw, p.ac, c_lo, kSlice, cl,
             pl);
  Stage<VEC>(wl, p.b, 0, 0, 1, rs, 1, rs, p.cm, cm0, kSlice, cl, pl);
  __syncthreads();

  int mycm = cm0 + cl * VEC;
  // this lane's x channel inside the tile; tail lanes read zeros of lane 0
  int xoff = mycm < p.cm ? mycm / p.mult - c_lo : 0;
  const float* wme = wl + cl * VEC;
  Vec<VEC> taps[K ? 9 : 1];
  if constexpr (K != 0) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
      taps[t] = Ld<VEC>(wme + (p.flip ? 8 - t : t) * kSlice);
  }
  int gl = p.tql - 2;  // log2 of the runs per patch row
  int units = p.tp << gl;
  float* out = p.out + (int64_t)n * p.oh * p.ow * p.oc;
  for (int u = pl; u < units; u += kPL) {
    int ty = u >> gl, tx = (u & ((1 << gl) - 1)) * kRun;
    const float* base = xs + ((ty * p.sh) * p.hc + tx * p.sw) * kSlice + xoff;
    Vec<VEC> acc[kRun];
#pragma unroll
    for (int o = 0; o < kRun; ++o) acc[o] = Zero<VEC>();
    if constexpr (K != 0) {
      constexpr int kWin = (kRun - 1) * K + 3;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float* row = base + r * p.hc * kSlice;
        Vec<VEC> win[kWin];
#pragma unroll
        for (int j = 0; j < kWin; ++j) win[j] = Ld<VEC>(row + j * kSlice);
#pragma unroll
        for (int o = 0; o < kRun; ++o)
#pragma unroll
          for (int s = 0; s < 3; ++s)
            Fma<VEC>(acc[o], win[o * K + s], taps[r * 3 + s]);
      }
    } else {
      int t = 0;
      for (int r = 0; r < p.r; ++r) {
        const float* row = base + r * p.hc * kSlice;
        for (int s = 0; s < p.s; ++s, ++t) {
          Vec<VEC> wv = Ld<VEC>(wme + (p.flip ? rs - 1 - t : t) * kSlice);
#pragma unroll
          for (int o = 0; o < kRun; ++o)
            Fma<VEC>(acc[o], Ld<VEC>(row + (o * p.sw + s) * kSlice), wv);
        }
      }
    }
    int py = p0 + ty;
    if (py < p.oh && mycm < p.cm) {
#pragma unroll
      for (int o = 0; o < kRun; ++o) {
        int qx = q0 + tx + o;
        if (qx < p.ow) St<VEC>(out + ((py * p.ow + qx) * p.oc + mycm), acc[o]);
      }
    }
  }
}

template <int VEC>
__device__ __forceinline__ void BackpropInput(const Params& p) {
  constexpr int kCL = Lanes<VEC>::kCL, kPL = Lanes<VEC>::kPL;
  float* ds = reinterpret_cast<float*>(dw_f32_smem);
  float* wl = ds + p.hr * p.hc * p.pitch;
  int cl = threadIdx.x % kCL, pl = threadIdx.x / kCL;
  int bid = blockIdx.x;
  int slice = bid % p.slices; bid /= p.slices;
  int pc = bid % p.pcs; bid /= p.pcs;
  int pr = bid % p.prs;
  int n = bid / p.prs;
  int c0 = slice * p.csl, cm_lo = c0 * p.mult;
  int ih0 = pr * p.tp, iw0 = pc << p.tql;
  int rs = p.r * p.s;
  // first dy row and column any pixel of the patch touches
  int pt0 = FloorDiv(ih0 + p.ph - (p.r - 1), p.sh);
  int qt0 = FloorDiv(iw0 + p.pw - (p.s - 1), p.sw);
  Stage<VEC>(ds, p.a + (int64_t)n * p.ah * p.aw * p.ac, pt0, qt0, p.hr, p.hc,
             p.ah, p.aw, p.ac, cm_lo, p.pitch, cl, pl);
  Stage<VEC>(wl, p.b, 0, 0, 1, rs, 1, rs, p.cm, cm_lo, p.pitch, cl, pl);
  __syncthreads();

  if (cl * VEC >= p.csl) return;  // mult > 1: fewer channels than lanes
  int myc = c0 + cl * VEC;
  int loff = cl * VEC * p.mult;
  float* out = p.out + (int64_t)n * p.oh * p.ow * p.oc;
  int npix = p.tp << p.tql;
  for (int i = pl; i < npix; i += kPL) {
    int ih = ih0 + (i >> p.tql), iw = iw0 + (i & ((1 << p.tql) - 1));
    int ay = ih + p.ph, ax = iw + p.pw;
    int py = ay / p.sh, qx = ax / p.sw;
    int r0 = ay - py * p.sh, s0 = ax - qx * p.sw;  // first tap of the phase
    py -= pt0;
    qx -= qt0;
    Vec<VEC> acc = Zero<VEC>();
    for (int r = r0, yy = py; r < p.r; r += p.sh, --yy)
      for (int s = s0, xx = qx; s < p.s; s += p.sw, --xx) {
        const float* d = ds + (yy * p.hc + xx) * p.pitch + loff;
        const float* w = wl + (r * p.s + s) * p.pitch + loff;
        if constexpr (VEC == 4) {
          Fma<VEC>(acc, Ld<VEC>(d), Ld<VEC>(w));
        } else {
          for (int m = 0; m < p.mult; ++m)
            acc.v[0] = fmaf(d[m], w[m], acc.v[0]);
        }
      }
    if (ih < p.oh && iw < p.ow && myc < p.oc)
      St<VEC>(out + ((ih * p.ow + iw) * p.oc + myc), acc);
  }
}

// NT taps of the filter per pass in registers.
template <int VEC, int NT>
__device__ __forceinline__ void BackpropFilter(const Params& p) {
  constexpr int kCL = Lanes<VEC>::kCL, kPL = Lanes<VEC>::kPL;
  float* xs = reinterpret_cast<float*>(dw_f32_smem);
  float* dys = xs + p.hr * p.hc * kSlice;
  float* red = xs;  // [wave][NT][kSlice], after the last patch of a pass
  int cl = threadIdx.x % kCL, pl = threadIdx.x / kCL;
  int slice = blockIdx.x % p.slices, worker = blockIdx.x / p.slices;
  int cm0 = slice * kSlice, c_lo = cm0 / p.mult;
  int mycm = cm0 + cl * VEC;
  int xoff = mycm < p.cm ? mycm / p.mult - c_lo : 0;
  int rs = p.r * p.s;
  int npix = p.tp << p.tql;
  for (int t0 = 0; t0 < rs; t0 += NT) {
    int off[NT];  // tap t0 + k inside the halo; 0 past the last tap
    int tr = t0 / p.s, ts = t0 - tr * p.s;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      off[k] = t0 + k < rs ? (tr * p.hc + ts) * kSlice : 0;
      if (++ts == p.s) { ts = 0; ++tr; }
    }
    Vec<VEC> acc[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) acc[k] = Zero<VEC>();
    for (int pid = worker; pid < p.npatch; pid += p.workers) {
      int pc = pid % p.pcs, rest = pid / p.pcs;
      int pr = rest % p.prs, n = rest / p.prs;
      int p0 = pr * p.tp, q0 = pc << p.tql;
      __syncthreads();  // the previous patch (or pass) is read
      Stage<VEC>(xs, p.a + (int64_t)n * p.ah * p.aw * p.ac, p0 * p.sh - p.ph,
                 q0 * p.sw - p.pw, p.hr, p.hc, p.ah, p.aw, p.ac, c_lo, kSlice,
                 cl, pl);
      Stage<VEC>(dys, p.b + (int64_t)n * p.oh * p.ow * p.oc, p0, q0, p.tp,
                 1 << p.tql, p.oh, p.ow, p.oc, cm0, kSlice, cl, pl);
      __syncthreads();
      for (int i = pl; i < npix; i += kPL) {
        int py = i >> p.tql, qx = i & ((1 << p.tql) - 1);
        Vec<VEC> g = Ld<VEC>(dys + i * kSlice + cl * VEC);
        const float* xb =
            xs + ((py * p.sh) * p.hc + qx * p.sw) * kSlice + xoff;
#pragma unroll
        for (int k = 0; k < NT; ++k) Fma<VEC>(acc[k], Ld<VEC>(xb + off[k]), g);
      }
    }
    __syncthreads();  // the tiles are read: red may overwrite them
    int lane = threadIdx.x & (STF_WAVE - 1), wave = threadIdx.x / STF_WAVE;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        for (int m = kCL; m < STF_WAVE; m <<= 1)
          acc[k].v[j] += __shfl_xor(acc[k].v[j], m, STF_WAVE);
      if (lane < kCL)
        St<VEC>(red + ((wave * NT + k) * kSlice + cl * VEC), acc[k]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NT * kSlice; i += kThreads) {
      int k = i / kSlice, ch = i % kSlice;
      if (t0 + k >= rs || cm0 + ch >= p.cm) continue;
      float v = 0.f;
#pragma unroll
      for (int wv = 0; wv < kThreads / STF_WAVE; ++wv)
        v += red[(wv * NT + k) * kSlice + ch];
      float* dst = p.out + ((t0 + k) * p.cm + cm0 + ch);
      if (p.workers > 1) atomicAdd(dst, v);
      else *dst = v;
    }
  }
}

template <int MODE, int VEC, int K>
__global__ __launch_bounds__(kThreads) void DwF32(Params p) {
  if constexpr (MODE == FWD) Forward<VEC, K>(p);
  else if constexpr (MODE == DX) BackpropInput<VEC>(p);
  else BackpropFilter<VEC, K>(p);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
bool Aligned16(const void* ptr) { return ((uintptr_t)ptr & 15) == 0; }

int64_t CeilDiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The geometry of one launch before its tile is chosen.
struct Shape {
  int n, ah, aw, ac, oh, ow, oc, r, s, sh, sw, ph, pw, mult, cm;
};

// Patch, halo and LDS size of a mode; false when even one patch row does not
// fit kLdsBudget or a count leaves an int.
bool PickTile(int mode, const Shape& g, Params* p, size_t* lds) {
  p->ah = g.ah; p->aw = g.aw; p->ac = g.ac;
  p->oh = g.oh; p->ow = g.ow; p->oc = g.oc;
  p->r = g.r; p->s = g.s; p->sh = g.sh; p->sw = g.sw;
  p->ph = g.ph; p->pw = g.pw; p->mult = g.mult; p->cm = g.cm;
  p->flip = 0;
  p->workers = 1;
  const int64_t lim = INT_MAX - 64;
  int64_t rs = (int64_t)g.r * g.s;
  if (g.mult < 1 || g.r < 1 || g.s < 1 || g.sh < 1 || g.sw < 1) return false;
  if ((int64_t)g.ah * g.aw * g.ac > lim || (int64_t)g.oh * g.ow * g.oc > lim ||
      rs > lim || rs * g.cm > lim)
    return false;
  // DX slices the input channels so that a slice's mult outputs stay together
  p->csl = g.mult == 1 ? kSlice : (g.mult < kSlice ? kSlice / g.mult : 1);
  p->pitch = mode == DX ? p->csl * g.mult : kSlice;
  p->slices = (int)(mode == DX ? CeilDiv(g.oc, p->csl) : CeilDiv(g.cm, kSlice));
  p->tql = g.ow <= 8 ? 3 : 4;
  int tq = 1 << p->tql;
  int64_t tp = std::max(1, std::min(128 / tq, g.oh));
  for (;; tp /= 2) {
    int64_t hr, hc, floats;
    if (mode == DX) {
      hr = (tp + g.r - 2) / g.sh + 2;
      hc = (tq + g.s - 2) / g.sw + 2;
      floats = (hr * hc + rs) * p->pitch;
    } else {
      hr = (tp - 1) * g.sh + g.r;
      hc = (int64_t)(tq - 1) * g.sw + g.s;
      floats = hr * hc * kSlice;
      if (mode == FWD) floats += rs * kSlice;
      else floats = std::max<int64_t>(
          floats + tp * tq * kSlice,
          (int64_t)(kThreads / STF_WAVE) * kMaxTapsInRegs * kSlice);
    }
    if (floats * 4 <= kLdsBudget) {
      p->tp = (int)tp; p->hr = (int)hr; p->hc = (int)hc;
      *lds = (size_t)floats * 4;
      break;
    }
    if (tp == 1) return false;
  }
  p->prs = (int)CeilDiv(g.oh, p->tp);
  p->pcs = (int)CeilDiv(g.ow, tq);
  int64_t npatch = (int64_t)g.n * p->prs * p->pcs;
  if (npatch * p->slices > lim) return false;  // gridDim.x
  p->npatch = (int)npatch;
  return true;
}

bool UseVec4(const StfConvGeom& g, int mult, const void* a, const void* b,
             const void* c) {
  return mult == 1 && g.c % 4 == 0 && Aligned16(a) && Aligned16(b) &&
         Aligned16(c);
}

Shape FwdShape(const StfConvGeom& g, int mult) {
  return Shape{g.n, g.h, g.w, g.c, g.p, g.q, g.c * mult, g.r, g.s, g.sh,
               g.sw, g.ph, g.pw, mult, g.c * mult};
}

// DX as a gather over dy; with stride 1 and mult 1 it is a forward pass.
Shape DxShape(const StfConvGeom& g, int mult) {
  return Shape{g.n, g.p, g.q, g.c * mult, g.h, g.w, g.c, g.r, g.s, g.sh,
               g.sw, g.ph, g.pw, mult, g.c * mult};
}

bool DxIsForward(const StfConvGeom& g, int mult) {
  return mult == 1 && g.sh == 1 && g.sw == 1;
}

Shape DxForwardShape(const StfConvGeom& g) {
  return Shape{g.n, g.p, g.q, g.c, g.h, g.w, g.c, g.r, g.s, 1, 1,
               g.r - 1 - g.ph, g.s - 1 - g.pw, 1, g.c};
}

bool ChannelsFit(const StfConvGeom& g, int mult) {
  return mult >= 1 && g.c >= 0 && (int64_t)g.c * mult <= INT_MAX - 64;
}

template <int VEC>
void LaunchForward(const Params& p, int64_t blocks, size_t lds,
                   hipStream_t stream) {
  dim3 grid((uint32_t)blocks), block(kThreads);
  if (p.r == 3 && p.s == 3 && p.sw == 1)
    hipLaunchKernelGGL((DwF32<FWD, VEC, 1>), grid, block, lds, stream, p);
  else if (p.r == 3 && p.s == 3 && p.sw == 2)
    hipLaunchKernelGGL((DwF32<FWD, VEC, 2>), grid, block, lds, stream, p);
  else
    hipLaunchKernelGGL((DwF32<FWD, VEC, 0>), grid, block, lds, stream, p);
}

}  // namespace

extern "C" int stf_depthwise_f32_ok(const StfConvGeom* g, int mult) {
  if (!ChannelsFit(*g, mult)) return 0;
  Params p;
  size_t lds;
  bool dx = DxIsForward(*g, mult)
                ? PickTile(FWD, DxForwardShape(*g), &p, &lds)
                : PickTile(DX, DxShape(*g, mult), &p, &lds);
  return dx && PickTile(FWD, FwdShape(*g, mult), &p, &lds) &&
         PickTile(DW, FwdShape(*g, mult), &p, &lds);
}

extern "C" hipError_t stf_depthwise_f32_fwd(const void* x, const void* w,
                                            void* y, const StfConvGeom* g,
                                            int mult, hipStream_t stream) {
  Params p;
  size_t lds;
  if (!ChannelsFit(*g, mult) || !PickTile(FWD, FwdShape(*g, mult), &p, &lds))
    return hipErrorInvalidValue;
  int64_t blocks = (int64_t)p.npatch * p.slices;
  if (blocks == 0) return hipSuccess;
  p.a = (const float*)x;
  p.b = (const float*)w;
  p.out = (float*)y;
  if (UseVec4(*g, mult, x, w, y)) LaunchForward<4>(p, blocks, lds, stream);
  else LaunchForward<1>(p, blocks, lds, stream);
  return hipGetLastError();
}

extern "C" hipError_t stf_depthwise_f32_dx(const void* dy, const void* w,
                                           void* dx, const StfConvGeom* g,
                                           int mult, hipStream_t stream) {
  Params p;
  size_t lds;
  if (!ChannelsFit(*g, mult)) return hipErrorInvalidValue;
  bool fwd = DxIsForward(*g, mult);
  if (!(fwd ? PickTile(FWD, DxForwardShape(*g), &p, &lds)
            : PickTile(DX, DxShape(*g, mult), &p, &lds)))
    return hipErrorInvalidValue;
  int64_t blocks = (int64_t)p.npatch * p.slices;
  if (blocks == 0) return hipSuccess;
  p.a = (const float*)dy;
  p.b = (const float*)w;
  p.out = (float*)dx;
  p.flip = fwd;
  bool vec = UseVec4(*g, mult, dy, w, dx);
  dim3 grid((uint32_t)blocks), block(kThreads);
  if (fwd && vec) LaunchForward<4>(p, blocks, lds, stream);
  else if (fwd) LaunchForward<1>(p, blocks, lds, stream);
  else if (vec)
    hipLaunchKernelGGL((DwF32<DX, 4, 0>), grid, block, lds, stream, p);
  else
    hipLaunchKernelGGL((DwF32<DX, 1, 0>), grid, block, lds, stream, p);
  return hipGetLastError();
}

extern "C" hipError_t stf_depthwise_f32_dw(const void* x, const void* dy,
                                           void* dw, const StfConvGeom* g,
                                           int mult, int workers,
                                           hipStream_t stream) {
  Params p;
  size_t lds;
  if (!ChannelsFit(*g, mult) || !PickTile(DW, FwdShape(*g, mult), &p, &lds))
    return hipErrorInvalidValue;
  if ((int64_t)g->r * g->s * p.cm == 0) return hipSuccess;
  // a worker without a patch would only add zeros; no patch at all (an empty
  // batch) still stores dw = 0
  p.workers = std::max(1, std::min(workers, p.npatch));
  if ((int64_t)p.workers * p.slices > INT_MAX - 64) return hipErrorInvalidValue;
  p.a = (const float*)x;
  p.b = (const float*)dy;
  p.out = (float*)dw;
  bool vec = UseVec4(*g, mult, x, dy, dw);
  bool small = g->r * g->s <= 9;
  dim3 grid((uint32_t)(p.workers * p.slices)), block(kThreads);
  if (vec && small)
    hipLaunchKernelGGL((DwF32<DW, 4, 9>), grid, block, lds, stream, p);
  else if (vec)
    hipLaunchKernelGGL((DwF32<DW, 4, kMaxTapsInRegs>), grid, block, lds,
                       stream, p);
  else if (small)
    hipLaunchKernelGGL((DwF32<DW, 1, 9>), grid, block, lds, stream, p);
  else
    hipLaunchKernelGGL((DwF32<DW, 1, kMaxTapsInRegs>), grid, block, lds,
                       stream, p);
  return hipGetLastError();
}
