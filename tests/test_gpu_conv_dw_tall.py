"""Bit-exact tests of the tall-skinny Conv2D backprop-filter kernel for
cout = 64 (csrc/kernels/hip/conv_dw_tall.hip, dispatched from
GpuConv2DBackpropFilterOp::Compute in csrc/kernels/gpu_conv.cc).

Inputs, reference and comparison are those of test_gpu_conv.py: the operand
families make the f32 sum exact in any order, so the result must equal the
numpy float64 reference rounded once to bf16, whatever the kernel's summation
order and however the atomics of its blocks interleave.

The kernel walks the output pixels in steps of 32 along one output row and
deals 16-row tiles of the [r*s*c8, 64] output to 4 waves. The cases:

  TALL_CASES
    base            3x3 s1 SAME at 8x32: q is exactly one step
    q tail          4x56 (ResNet's q = 56: steps of 32 + 24) and 8x24
    VALID           8x34, p, q = 6, 32: no halo zeros
    stem            c 3 padded to 8, 7x7 stride 2, 25 row tiles, at 16x64 and
                    at 14x48 (q = 24; batch 8 there, since 7 * 24 pixels per
                    image need it for M % 64 == 0)
    small c         c 8 (r*s*c = 72, 4.5 row tiles), 16, 32
    filters         2x2, 1x7, 7x1 and 5x3 at c 32, strides (1,1), (2,1), (1,2)
    many steps      batch 32 at 16x64: 1024 steps, more than one per block
                    for any grid of about one block per CU, all blocks adding
                    into one accumulator
  EDGE_CASES        just outside the gate, on the split-K path as before:
                    M = 704, r*s*c8 = 584 (1x73 at c 8) and cout 128
"""
import numpy as np
import pytest

import simple_tensorflow_amd as tf

from test_gpu_conv import (Case, DW_CASES, IMAGES, _build, _is_1x1_s1, _run,
                           _up)
from test_gpu_gemm import _sessions, sess  # noqa: F401  (the fixtures)
from test_gpu_kernels import _bf16


# ---------------------------------------------------------------------------
# Python mirror of stf_conv2d_dw_tall_ok (hip/conv_dw_tall.hip) behind the
# kImplicit branch of GpuConv2DBackpropFilterOp::Compute (STF_NO_TALL_DW unset)
# ---------------------------------------------------------------------------
def _tall_ok(cs):
    p, q, _, _ = cs.pq
    M, c8 = cs.n * p * q, _up(cs.c, 8)
    if _is_1x1_s1(cs) or cs.cout != 64 or M % 64 or M < 768:
        return False
    if cs.r * cs.s * c8 > 576:
        return False
    # three LDS buffers: the x halo in 16-byte slots, rounded up to 256, plus
    # the 256 slots of the dy tile, within 160 KiB
    slots = cs.r * (31 * cs.sw + cs.s) * (c8 // 8)
    return 3 * 16 * (_up(slots, 256) + 256) <= 160 * 1024


def _dw(n, hw, c, f, cout=64, st=(1, 1), pad='SAME'):
    return Case('dw', n, hw[0], hw[1], c, f[0], f[1], cout, st[0], st[1], pad,
                False)


_STRIDED = [(hw, st) for (hw, st) in IMAGES if st != (2, 2)]

TALL_CASES = (
    [_dw(4, (8, 32), 64, (3, 3))] +
    [_dw(4, (4, 56), 64, (3, 3)), _dw(4, (8, 24), 64, (3, 3))] +
    [_dw(4, (8, 34), 64, (3, 3), pad='VALID')] +
    [_dw(4, (16, 64), 3, (7, 7), st=(2, 2)),
     _dw(8, (14, 48), 3, (7, 7), st=(2, 2))] +
    [_dw(4, (8, 32), c, (3, 3)) for c in (8, 16, 32)] +
    [_dw(4, hw, 32, f, st=st) for f in ((2, 2), (1, 7), (7, 1), (5, 3))
     for (hw, st) in _STRIDED] +
    [_dw(32, (16, 64), 64, (3, 3))])

EDGE_CASES = [
    _dw(11, (4, 16), 64, (3, 3)),           # M = 704 < 768
    _dw(4, (8, 32), 8, (1, 73)),            # r*s*c8 = 584 > 576
    _dw(4, (8, 32), 64, (3, 3), cout=128)]


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_gate_mirror():
    for cs in TALL_CASES:
        assert cs.h != cs.w and _tall_ok(cs), cs.id
    for cs in EDGE_CASES:
        assert cs.h != cs.w and not _tall_ok(cs), cs.id
    p, q, _, _ = EDGE_CASES[0].pq
    assert EDGE_CASES[0].n * p * q == 704
    assert EDGE_CASES[1].r * EDGE_CASES[1].s * EDGE_CASES[1].c == 584
    for cs in DW_CASES:
        assert not _tall_ok(cs), cs.id
    # what the table is there for
    assert [cs.pq[1] for cs in TALL_CASES[:4]] == [32, 56, 24, 32]
    assert [cs.pq[:2] for cs in TALL_CASES[4:6]] == [(8, 32), (7, 24)]
    assert sorted({(cs.sh, cs.sw) for cs in TALL_CASES[9:21]}) == \
        [(1, 1), (1, 2), (2, 1)]
    big = TALL_CASES[-1]
    assert big.n * big.pq[0] * big.pq[1] == 32768


@pytest.mark.parametrize('cs', TALL_CASES + EDGE_CASES, ids=lambda cs: cs.id)
def test_reference_conditions(cs):
    """max|exact| <= 256 in the 'int' family and the other exactness
    conditions (asserted inside _build): the reference side alone, no GPU."""
    for fam, a, b, side, want in _build(cs):
        assert np.array_equal(_bf16(a), a) and np.array_equal(_bf16(b), b)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_fragment_read():
    """The transposing LDS read that feeds both MFMA operands: lane l must
    hold row l % 16 at k = 8 * (l // 16) + 0..7 of a [32 k][16 rows] tile."""
    tile = np.random.RandomState(7).permutation(1 << 16)[:512] \
        .astype(np.uint16).reshape(32, 16)
    got = np.asarray(tf._core.conv_dw_tall_frag_probe(tile))
    want = np.empty((64, 8), np.uint16)
    for lane in range(64):
        for e in range(8):
            want[lane, e] = tile[8 * (lane // 16) + e, lane % 16]
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize('cs', TALL_CASES, ids=lambda cs: cs.id)
def test_conv2d_backprop_filter_tall(sess, cs):
    _run(sess, cs)


@pytest.mark.gpu
@pytest.mark.parametrize('cs', EDGE_CASES, ids=lambda cs: cs.id)
def test_conv2d_backprop_filter_gate_edge(sess, cs):
    _run(sess, cs)
