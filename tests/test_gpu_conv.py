"""Bit-exact pinning tests for the bf16 Conv2D forward, backprop-filter (dW)
and backprop-input (dx, with and without the fused residual `side`) GPU ops:
csrc/kernels/gpu_conv.cc over hip/gemm_bf16.hip, hip/gemm_bf16_8ph.hip,
hip/conv_im2col.hip and the ConvAG address generator in hip/hip_common.h.

The inputs are those of test_gpu_gemm.py (see its docstring for why f32
accumulation is then exact in any order): family 'int' has integers in
[-2, 2] against a sparse {-1, 0, 1} operand, with max|exact| <= 256 asserted
on the reference; 'mantA' / 'mantB' have n/16, |n| <= 255, in the first /
second operand against the sparse one. The non-zero share of the sparse
operand is min(2/3, 1000/Kc), Kc the contraction length: r*s*c forward,
n*p*q for dW, r*s*cout for dx. The operand pairs are (x, w) forward, (x, dy)
for dW and (dy, w) for dx.

The reference is numpy float64, one function each for forward, dW and dx,
looping over the (r, s) taps with strided slices, with independent sh and sw
and TF's SAME rule (pad_before = total // 2). It shares nothing with the
project's CPU conv kernels or window_geom.h.

Expected outputs
  forward, dW           _bf16(exact): one rounding, in the GEMM epilogue or
                        in the split-K cast
  dx, 1x1 and implicit  _bf16(exact)
  dx, GEMM + col2im     the GEMM writes dcol[m, (r, s, c)] in bf16 and col2im
                        sums the taps of one dx element in f32, then rounds:
                        _bf16(sum over taps of _bf16(tap)). In the 'int'
                        family every tap is an integer of at most 256 in
                        magnitude (asserted), so this is _bf16(exact) again;
                        in the 'mant' families the per-tap rounding is part
                        of what the path computes and the reference applies
                        it. The rounded taps are multiples of 1/16 below
                        2^14, so their f32 sum is exact in any order.
  with `side`           a second rounding, on every path (8-phase epilogue,
                        col2im's store, stf_binary after the 1x1):
                        _bf16(<the above> + side), side integers in [-3, 3]

Paths, as derived from the dispatch in gpu_conv.cc (mirrored by _fwd_path,
_dw_path and _dx_path below; M = n*p*q, 1x1s1 = 1x1 filter, stride 1):

  forward   C % 8 != 0 and not 1x1s1    'stem': x and w zero-padded to 8
                                         channels, then as below
            rscp = r*s*c, rounded up to 64 unless 1x1s1
            not 1x1s1, 8ph_ok(M, cout, rscp)   implicit_8ph  (NR by cout)
            not 1x1s1, cout % 8 == 0           implicit_nt   (A = ConvAG,
                                                B K-major, no skinny tile)
            1x1s1, not 8ph_ok, cout % 8 == 0   gemm_bkm      (x is A)
            1x1s1, 8ph_ok(M, cout, c)          gemm_8ph      (w^T, 8-phase)
            otherwise (cout % 8 != 0)          im2col_wT     (im2col unless
                                                1x1s1, w^T, NT GEMM)
  dW        not 1x1s1, cout % 8 == 0, M % 64 == 0   implicit, split =
                                         PickSplitK(r*s*c8, cout, M); 'stem'
                                         pads x to c8 channels and unpads dW
            cout % 8 == 0 and (not 1x1s1 or c % 8 == 0)   kmajor_gemm
                                         (im2col unless 1x1s1; A and B
                                         K-major, through GemmBf16AutoEx)
            otherwise                               transpose_gemm
  dx        1x1s1, side, 8ph_ok(M, c, cout)         1x1_8ph_side
            stride 1, not 1x1s1, cout % 8 == 0,
              8ph_ok(n*h*w, c, roundup64(r*s*cout)) implicit_8ph
            1x1s1                                   1x1_nt (+ stf_binary add
                                                    when side is given)
            otherwise                               gemm_col2im (V8 kernel
                                                    when c % 8 == 0)

Geometries. Every image has h != w: (8, 32) at stride (1, 1), (16, 64) at
(2, 2), (16, 32) at (2, 1) and (8, 64) at (1, 2), so that SAME gives p, q =
8, 32 and M = 256 at batch 1; filters 3x3, 1x7, 7x1, 2x2 (even: asymmetric
SAME), 5x3 and 1x1; SAME and VALID. That is GEOMS, 48 entries; VALID and
batch 2 at (7, 9) (GEOMS_EDGE) give M that is no multiple of 256 or of 64.
Every variant the dispatch names runs all of GEOMS, and the gate decides
which path a geometry takes (the self-check counts them): forward at cout
64, 128, 256 (8-phase, NT under VALID), 24, 48 (NT) and 12 (im2col + w^T);
dW at batch 1 and 4 and at cout 12; dx at c = 8 and 12 with and without
`side`; implicit dx runs every stride-1 entry. Only the two extra 128-wide
NT shapes (c 16, cout 136) run GEOMS_SHORT: SAME,
every stride, 3x3 / 1x7 / 7x1 / 2x2."""
import collections
import functools
import itertools
import zlib

import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.framework import dtypes
from simple_tensorflow_amd.python.framework.ops import (apply_op,
                                                        convert_to_tensor)

from test_gpu_kernels import _bf16, _sess
from test_gpu_gemm import (_8ph_ok, _pick_splitk, _assert_equal, _feed,
                           _rich, _round_exact as _round_f64, _sparse,
                           _sessions, sess)  # noqa: F401  (the fixtures)

FAMILIES = ('int', 'mantA', 'mantB')

# ---------------------------------------------------------------------------
# geometry, written out here from the TF rule (not from window_geom.h)
# ---------------------------------------------------------------------------
IMAGES = (((8, 32), (1, 1)), ((16, 64), (2, 2)), ((16, 32), (2, 1)),
          ((8, 64), (1, 2)))
FILTERS = ((3, 3), (1, 7), (7, 1), (2, 2), (5, 3), (1, 1))
GEOMS = [(hw, f, st, pad) for (hw, st) in IMAGES for f in FILTERS
         for pad in ('SAME', 'VALID')]
GEOMS_SHORT = [(hw, f, st, 'SAME') for (hw, st) in IMAGES
               for f in FILTERS[:4]]
# batch 2 at 7x9: M = 126 under SAME, an edge block in every tile
GEOMS_EDGE = [((7, 9), f, (1, 1), pad) for f in FILTERS
              for pad in ('SAME', 'VALID')]


def _axis(size, k, stride, padding):
    """(output extent, pad_before) of one spatial axis."""
    if padding == 'SAME':
        out = -(-size // stride)
        return out, max(0, (out - 1) * stride + k - size) // 2
    return (size - k) // stride + 1, 0


class Case(collections.namedtuple(
        'Case', 'op n h w c r s cout sh sw padding side')):
    __slots__ = ()

    @property
    def pq(self):
        p, ph = _axis(self.h, self.r, self.sh, self.padding)
        q, pw = _axis(self.w, self.s, self.sw, self.padding)
        return p, q, ph, pw

    @property
    def id(self):
        return '%s%s-%dx%dx%dx%d-%dx%d-k%d-s%d%d-%s' % (
            self.op, '+side' if self.side else '', self.n, self.h, self.w,
            self.c, self.r, self.s, self.cout, self.sh, self.sw,
            self.padding)


def _cases(op, n, c, cout, geoms, side=False):
    return [Case(op, n, hw[0], hw[1], c, f[0], f[1], cout, st[0], st[1],
                 pad, side) for (hw, f, st, pad) in geoms]


def _up(v, to):
    return -(-v // to) * to


# ---------------------------------------------------------------------------
# Python mirrors of the dispatch in csrc/kernels/gpu_conv.cc
# ---------------------------------------------------------------------------
def _is_1x1_s1(cs):
    p, q, ph, pw = cs.pq
    return (cs.r == 1 and cs.s == 1 and cs.sh == 1 and cs.sw == 1 and
            ph == 0 and pw == 0)


def _fwd_path(cs):
    # GpuConv2DOp::Compute
    p, q, _, _ = cs.pq
    M, one, c, stem = cs.n * p * q, _is_1x1_s1(cs), cs.c, ''
    if not one and c % 8:
        c, stem = _up(c, 8), 'stem+'
    rsc = cs.r * cs.s * c
    rscp = rsc if one else _up(rsc, 64)
    fits = _8ph_ok(M, cs.cout, rscp)
    if not one and c % 8 == 0:
        if fits:
            return stem + 'implicit_8ph'
        if cs.cout % 8 == 0:
            return stem + 'implicit_nt'
    if not fits and cs.cout % 8 == 0:
        return stem + 'gemm_bkm'
    return stem + ('gemm_8ph' if fits else 'im2col_wT')


def _dw_path(cs):
    # GpuConv2DBackpropFilterOp::Compute
    p, q, _, _ = cs.pq
    M, one = cs.n * p * q, _is_1x1_s1(cs)
    if not one and cs.cout % 8 == 0 and M % 64 == 0:
        sk = _pick_splitk(cs.r * cs.s * _up(cs.c, 8), cs.cout, M)
        return '%simplicit_sk%s' % ('stem+' if cs.c % 8 else '',
                                    '1' if sk == 1 else 'N')
    if cs.cout % 8 == 0 and (not one or cs.c % 8 == 0):
        return 'kmajor_gemm'
    return 'transpose_gemm'


def _dx_path(cs):
    # GpuConv2DBackpropInputOp::Compute
    p, q, _, _ = cs.pq
    M, one = cs.n * p * q, _is_1x1_s1(cs)
    if one and cs.side and _8ph_ok(M, cs.c, cs.cout):
        return '1x1_8ph_side'
    if (cs.sh == 1 and cs.sw == 1 and not one and cs.cout % 8 == 0 and
            _8ph_ok(cs.n * cs.h * cs.w, cs.c,
                    _up(cs.r * cs.s * cs.cout, 64))):
        return 'implicit_8ph'
    if one:
        return '1x1_nt'
    return 'gemm_col2im'


def _path(cs):
    return {'fwd': _fwd_path, 'dw': _dw_path, 'dx': _dx_path}[cs.op](cs)


# ---------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------
STEM = [((16, 64), (7, 7), (2, 2), 'SAME')]
STEM_EDGE = [((14, 18), (7, 7), (2, 2), 'SAME'),
             ((14, 18), (7, 7), (2, 2), 'VALID')]
ONE_BY_ONE = [((8, 32), (1, 1), (1, 1), 'SAME')]

FWD_CASES = (
    _cases('fwd', 1, 8, 64, GEOMS) +            # implicit 8-phase NR 1; VALID: NT
    _cases('fwd', 1, 8, 128, GEOMS) +           # NR 2
    _cases('fwd', 1, 8, 256, GEOMS) +           # NR 4
    _cases('fwd', 1, 8, 24, GEOMS) +            # implicit NT, 64x64 tile; 1x1: bkm
    _cases('fwd', 1, 8, 48, GEOMS) +
    _cases('fwd', 1, 16, 136, GEOMS_SHORT) +    # implicit NT, 128x128 tile
    _cases('fwd', 2, 8, 64, GEOMS_EDGE) +       # M = 2*7*9: edge rows
    _cases('fwd', 1, 64, 64, ONE_BY_ONE) +      # 1x1 inside the 8-phase gate
    _cases('fwd', 1, 64, 128, ONE_BY_ONE) +
    _cases('fwd', 1, 8, 12, GEOMS) +            # im2col (1x1: x itself) + w^T
    _cases('fwd', 2, 8, 12, GEOMS_EDGE) +
    _cases('fwd', 1, 3, 64, STEM) +             # channel pad, RSC 147 -> 448
    _cases('fwd', 1, 3, 24, STEM) +
    _cases('fwd', 2, 3, 64, STEM_EDGE))

DW_CASES = (
    _cases('dw', 1, 8, 16, GEOMS) +             # implicit split 1; VALID and
                                                # 1x1: K-major GEMM
    _cases('dw', 4, 8, 16, GEOMS) +             # n*p*q = 1024: split 2
    _cases('dw', 1, 16, 136, GEOMS_SHORT) +     # 128-wide tiles with edges
    _cases('dw', 2, 8, 16, GEOMS_EDGE) +        # M % 64 != 0
    _cases('dw', 1, 3, 16, STEM) +              # stem pad and unpad
    _cases('dw', 4, 3, 16, STEM) +
    _cases('dw', 2, 3, 16, STEM_EDGE) +         # C = 3 through im2col
    _cases('dw', 1, 8, 12, GEOMS) +             # transpose path
    _cases('dw', 2, 8, 12, GEOMS_EDGE) +
    _cases('dw', 1, 12, 16, ONE_BY_ONE))        # 1x1 with c % 8 != 0

_S1 = [g for g in GEOMS if g[2] == (1, 1)]
DX_CASES = (
    _cases('dx', 1, 8, 16, GEOMS) +             # col2im V8; 1x1: NT GEMM
    _cases('dx', 1, 64, 8, _S1) +               # implicit 8-phase NR 1
    _cases('dx', 1, 128, 16, _S1[:8:2]) +       # NR 2
    _cases('dx', 2, 64, 16, GEOMS_EDGE) +       # n*h*w = 126: outside the gate
    _cases('dx', 1, 12, 16, GEOMS) +            # col2im, scalar kernel
    _cases('dx', 1, 64, 64, ONE_BY_ONE) +       # 1x1 NT diverted to 8-phase
    _cases('dx', 1, 64, 64, ONE_BY_ONE, side=True) +      # 8-phase epilogue
    _cases('dx', 1, 64, 8, _S1, side=True) +    # implicit dx; 1x1: NT + add
    _cases('dx', 1, 8, 16, GEOMS, side=True) +  # col2im V8; 1x1 outside the gate
    _cases('dx', 2, 8, 16, GEOMS_EDGE, side=True) +
    _cases('dx', 1, 12, 16, GEOMS, side=True))  # col2im scalar

ALL_CASES = FWD_CASES + DW_CASES + DX_CASES


# ---------------------------------------------------------------------------
# reference: numpy float64, a loop over the filter taps
# ---------------------------------------------------------------------------
def _padded(cs):
    """Shape of x zero-padded so that every tap's strided window is inside,
    and the offsets of x within it."""
    p, q, ph, pw = cs.pq
    return ((cs.n, max(ph + cs.h, (p - 1) * cs.sh + cs.r),
             max(pw + cs.w, (q - 1) * cs.sw + cs.s), cs.c), ph, pw)


def _window(cs, i, j):
    p, q, _, _ = cs.pq
    return (slice(None), slice(i, i + (p - 1) * cs.sh + 1, cs.sh),
            slice(j, j + (q - 1) * cs.sw + 1, cs.sw), slice(None))


def _ref_fwd(cs, x, w):
    shape, ph, pw = _padded(cs)
    xp = np.zeros(shape, np.float64)
    xp[:, ph:ph + cs.h, pw:pw + cs.w, :] = x
    p, q, _, _ = cs.pq
    y = np.zeros((cs.n, p, q, cs.cout), np.float64)
    for i, j in itertools.product(range(cs.r), range(cs.s)):
        y += xp[_window(cs, i, j)] @ w[i, j].astype(np.float64)
    return y


def _ref_dw(cs, x, dy):
    shape, ph, pw = _padded(cs)
    xp = np.zeros(shape, np.float64)
    xp[:, ph:ph + cs.h, pw:pw + cs.w, :] = x
    dy2 = dy.astype(np.float64).reshape(-1, cs.cout)
    dw = np.zeros((cs.r, cs.s, cs.c, cs.cout), np.float64)
    for i, j in itertools.product(range(cs.r), range(cs.s)):
        dw[i, j] = xp[_window(cs, i, j)].reshape(-1, cs.c).T @ dy2
    return dw


def _ref_dx(cs, dy, w, tap=lambda t: t):
    """`tap` is applied to each filter tap's contribution before the sum."""
    shape, ph, pw = _padded(cs)
    dxp = np.zeros(shape, np.float64)
    dy = dy.astype(np.float64)
    for i, j in itertools.product(range(cs.r), range(cs.s)):
        dxp[_window(cs, i, j)] += tap(dy @ w[i, j].astype(np.float64).T)
    return dxp[:, ph:ph + cs.h, pw:pw + cs.w, :]


# ---------------------------------------------------------------------------
# inputs and expected outputs
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _build(cs):
    """[(family, operand 1, operand 2, side or None, expected)] of a case;
    computed once and shared by the CPU and the GPU tests."""
    p, q, _, _ = cs.pq
    x_shape = (cs.n, cs.h, cs.w, cs.c)
    w_shape = (cs.r, cs.s, cs.c, cs.cout)
    dy_shape = (cs.n, p, q, cs.cout)
    shapes, kc = {
        'fwd': ((x_shape, w_shape), cs.r * cs.s * cs.c),
        'dw': ((x_shape, dy_shape), cs.n * p * q),
        'dx': ((dy_shape, w_shape), cs.r * cs.s * cs.cout)}[cs.op]
    col2im = cs.op == 'dx' and _dx_path(cs) == 'gemm_col2im'
    out = []
    for fam in FAMILIES:
        seed = zlib.crc32(('%s/%s' % (cs.id, fam)).encode())
        rng = np.random.RandomState(seed % 2**31)
        if fam == 'mantB':
            a, b = _sparse(rng, shapes[0], kc), _rich(rng, shapes[1], fam)
        else:
            a, b = _rich(rng, shapes[0], fam), _sparse(rng, shapes[1], kc)
        side = None
        if cs.side:
            side = rng.randint(-3, 4, x_shape).astype(np.float32)
        if cs.op == 'fwd':
            exact = _ref_fwd(cs, a, b)
        elif cs.op == 'dw':
            exact = _ref_dw(cs, a, b)
        else:
            exact = _ref_dx(cs, a, b)
        if fam == 'int':
            # conditions on the inputs, not checks of the kernel
            assert np.abs(exact).max() <= 256, (cs.id, np.abs(exact).max())
            if col2im:
                def small(t):
                    assert np.abs(t).max() <= 256, cs.id
                    return t
                _ref_dx(cs, a, b, tap=small)
        else:
            assert np.abs(exact).max() < 2.0 ** 20, cs.id
            if col2im:
                exact = _ref_dx(cs, a, b,
                                tap=lambda t: _round_f64(t).astype(np.float64))
        want = _round_f64(exact)
        if cs.side:
            want = _round_f64(want.astype(np.float64) + side)
        out.append((fam, a, b, side, want))
    return out


# ---------------------------------------------------------------------------
# CPU: the table reaches every path, and the inputs meet their conditions
# ---------------------------------------------------------------------------
def _count(cases, path, **fields):
    return sum(1 for cs in cases if _path(cs) == path and
               all(getattr(cs, k) == v for k, v in fields.items()))


def test_case_table_reaches_every_path():
    assert len(set(ALL_CASES)) == len(ALL_CASES)
    for cs in ALL_CASES:
        assert cs.h != cs.w, cs.id
    n_all, n_one = len(GEOMS), 2    # 1x1 at stride 1, SAME and VALID
    # SAME gives M = 256 at batch 1; so do 1x1 and 2x2 VALID at stride 2
    m256 = sum(1 for cs in _cases('fwd', 1, 8, 64, GEOMS)
               if cs.pq[0] * cs.pq[1] == 256 and not _is_1x1_s1(cs))
    assert m256 == n_all // 2 - 1 + 4
    # forward: every named cout on all of GEOMS
    for cout in (64, 128, 256):
        assert _count(FWD_CASES, 'implicit_8ph', cout=cout, n=1) == m256
        assert _count(FWD_CASES, 'implicit_nt', cout=cout, n=1) == \
            n_all - n_one - m256
    for cout in (24, 48):
        assert _count(FWD_CASES, 'implicit_nt', cout=cout) == n_all - n_one
        assert _count(FWD_CASES, 'gemm_bkm', cout=cout) == n_one
    assert _count(FWD_CASES, 'implicit_nt', cout=136) == len(GEOMS_SHORT)
    assert _count(FWD_CASES, 'implicit_nt', cout=64, n=2) == \
        len(GEOMS_EDGE) - n_one       # M = 126 under SAME
    assert _count(FWD_CASES, 'gemm_8ph') == 2
    assert _count(FWD_CASES, 'im2col_wT', cout=12, n=1) == n_all
    assert _count(FWD_CASES, 'im2col_wT', cout=12, n=2) == len(GEOMS_EDGE)
    assert _count(FWD_CASES, 'stem+implicit_8ph') == 1
    assert _count(FWD_CASES, 'stem+implicit_nt') == 3
    # dW
    m64 = sum(1 for cs in _cases('dw', 1, 8, 16, GEOMS)
              if cs.pq[0] * cs.pq[1] % 64 == 0 and not _is_1x1_s1(cs))
    big = sum(1 for cs in _cases('dw', 4, 8, 16, GEOMS)
              if 4 * cs.pq[0] * cs.pq[1] >= 1024 and not _is_1x1_s1(cs))
    assert m64 >= n_all // 2 - 1 and big >= n_all // 2 - 1
    assert _count(DW_CASES, 'implicit_sk1', n=1, cout=16) == m64
    assert _count(DW_CASES, 'kmajor_gemm', n=1, cout=16) == n_all - m64
    assert _count(DW_CASES, 'implicit_skN', n=4, c=8) == big
    assert _count(DW_CASES, 'implicit_sk1', n=4, c=8) + \
        _count(DW_CASES, 'kmajor_gemm', n=4, c=8) == n_all - big
    assert _count(DW_CASES, 'implicit_sk1', cout=136) == len(GEOMS_SHORT)
    assert _count(DW_CASES, 'stem+implicit_sk1') == 1
    assert _count(DW_CASES, 'stem+implicit_skN') == 1
    assert _count(DW_CASES, 'kmajor_gemm', c=3) == 2
    assert _count(DW_CASES, 'kmajor_gemm', n=2, c=8) == len(GEOMS_EDGE)
    assert _count(DW_CASES, 'kmajor_gemm', r=1, s=1, sh=1, sw=1) >= 2
    assert _count(DW_CASES, 'transpose_gemm', cout=12, n=1) == n_all
    assert _count(DW_CASES, 'transpose_gemm', cout=12, n=2) == len(GEOMS_EDGE)
    assert _count(DW_CASES, 'transpose_gemm', c=12) == 1
    # dx and dx with side: every path on every geometry its gate admits
    for side in (False, True):
        assert _count(DX_CASES, 'implicit_8ph', c=64, side=side) == \
            len(_S1) - n_one
        for c in (8, 12):       # V8 and scalar col2im; 1x1 outside the gate
            assert _count(DX_CASES, 'gemm_col2im', n=1, c=c, side=side) == \
                n_all - n_one
            assert _count(DX_CASES, '1x1_nt', n=1, c=c, side=side) == n_one
    assert _count(DX_CASES, 'implicit_8ph', c=128) == 4
    assert _count(DX_CASES, 'gemm_col2im', n=2, c=64) == \
        len(GEOMS_EDGE) - n_one
    assert _count(DX_CASES, 'gemm_col2im', n=2, c=8, side=True) == \
        len(GEOMS_EDGE) - n_one
    assert _count(DX_CASES, '1x1_nt', n=2, side=True) == n_one
    assert _count(DX_CASES, '1x1_8ph_side') == 1


@pytest.mark.parametrize('op,cases', [('fwd', FWD_CASES), ('dw', DW_CASES),
                                      ('dx', DX_CASES)],
                         ids=['fwd', 'dw', 'dx'])
def test_reference_conditions(op, cases):
    """max|exact| <= 256 for every small-integer case, and the other
    exactness conditions: the reference side alone, no GPU."""
    for cs in cases:
        assert cs.op == op
        for fam, a, b, side, want in _build(cs):
            assert np.array_equal(_bf16(a), a) and np.array_equal(_bf16(b), b)


def test_reference_same_padding_is_asymmetric():
    """The reference itself, on a case small enough to do by hand: a 2x2
    filter of ones under SAME pads after, not before."""
    cs = Case('fwd', 1, 2, 3, 1, 2, 2, 1, 1, 1, 'SAME', False)
    x = np.arange(1.0, 7.0).reshape(1, 2, 3, 1)
    y = _ref_fwd(cs, x, np.ones((2, 2, 1, 1)))
    assert np.array_equal(y[0, :, :, 0], [[12, 16, 9], [9, 11, 6]])
    dx = _ref_dx(cs, np.ones((1, 2, 3, 1)), np.ones((2, 2, 1, 1)))
    assert np.array_equal(dx[0, :, :, 0], [[1, 2, 2], [2, 4, 4]])
    dw = _ref_dw(cs, x, np.ones((1, 2, 3, 1)))
    assert np.array_equal(dw[:, :, 0, 0], [[21, 16], [15, 11]])


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _op(cs, feeds, a, b, side):
    strides = [1, cs.sh, cs.sw, 1]
    a, b = _feed(feeds, a, tf.bfloat16), _feed(feeds, b, tf.bfloat16)
    if cs.op == 'fwd':
        return tf.nn.conv2d(a, b, strides, cs.padding)
    if cs.op == 'dw':
        return tf.nn.conv2d_backprop_filter(
            a, [cs.r, cs.s, cs.c, cs.cout], b, strides, cs.padding)
    sizes = [cs.n, cs.h, cs.w, cs.c]
    if side is None:
        return tf.nn.conv2d_backprop_input(sizes, b, a, strides, cs.padding)
    return apply_op('Conv2DBackpropInputAdd',
                    convert_to_tensor(sizes, dtype=dtypes.int32), b, a,
                    _feed(feeds, side, tf.bfloat16), strides=strides, padding=cs.padding)


def _run(sess, cs):
    feeds, ops = {}, []
    fams = _build(cs)
    for fam, a, b, side, _ in fams:
        ops.append(_op(cs, feeds, a, b, side))
    outs = sess.run(ops, feeds)
    for (fam, _, _, _, want), out in zip(fams, outs):
        _assert_equal('%s [%s] %s' % (cs.id, _path(cs), fam), out, want)


@pytest.mark.gpu
@pytest.mark.parametrize('cs', FWD_CASES, ids=lambda cs: cs.id)
def test_conv2d_forward(sess, cs):
    _run(sess, cs)


@pytest.mark.gpu
@pytest.mark.parametrize('cs', DW_CASES, ids=lambda cs: cs.id)
def test_conv2d_backprop_filter(sess, cs):
    _run(sess, cs)


@pytest.mark.gpu
@pytest.mark.parametrize('cs', DX_CASES, ids=lambda cs: cs.id)
def test_conv2d_backprop_input(sess, cs):
    _run(sess, cs)
