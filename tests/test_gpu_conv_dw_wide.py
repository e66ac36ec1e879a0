"""Bit-exact tests of the wide Conv2D backprop-filter kernel for cout = 64*k
(csrc/kernels/hip/conv_dw_wide.hip, dispatched from
GpuConv2DBackpropFilterOp::Compute after the tall gate fails).

Inputs and reference are those of test_gpu_conv.py: the operand families make
the f32 sum exact in any order, so the kernel's accumulator must equal the
float64 reference as f32, and the op's output that reference rounded once to
bf16, however the blocks' atomics interleave.

The kernel tiles dW into channel slices of CS by cout slices of 128 and sums
over patches of PW x PH = 32 output pixels. WIDE_CASES (3x3, stride 1, SAME at
n 4, 8x32 unless said otherwise) walks each of those: one slice; two channel
slices; two cout slices and a half-empty one; the 16x2 and 8x4 patches with p
and q tails, 4x56 (seven 8x4 patches) and 4x28 (q tail of 32x1); VALID; strided 1x1 (compact halo) with one slice of
256 and two of 512; 5x5 (CS 16), 1x7 and 7x1 (CS 80, swizzle mask 1), the 7x7
stem shape with its channel pad (op level only); many steps per block.
EDGE_CASES stay on split-K: cout 136, M = 704, 1x73 (no CS)."""
import numpy as np
import pytest

import simple_tensorflow_amd as tf

from test_gpu_conv import Case, DW_CASES, IMAGES, _build, _ref_dw, _run, _up
from test_gpu_gemm import _sessions, sess  # noqa: F401  (the fixtures)
from test_gpu_kernels import _bf16


def _dw(n, hw, c, f, cout=128, st=(1, 1), pad='SAME'):
    return Case('dw', n, hw[0], hw[1], c, f[0], f[1], cout, st[0], st[1], pad,
                False)


WIDE_CASES = (
    [_dw(4, (8, 32), 64, (3, 3)), _dw(4, (8, 32), 128, (3, 3))] +
    [_dw(4, (8, 32), 64, (3, 3), cout=co) for co in (256, 192)] +
    [_dw(32, (7, 14), 64, (3, 3)), _dw(32, (14, 7), 64, (3, 3)),
     _dw(4, (4, 56), 64, (3, 3))] +
    [_dw(4, (8, 34), 64, (3, 3), pad='VALID')] +
    [_dw(4, hw, 256, (1, 1), st=st) for (hw, st) in IMAGES if st != (1, 1)] +
    [_dw(4, (16, 64), 1024, (1, 1), st=(2, 2))] +
    [_dw(4, (8, 32), 48, (5, 5), cout=64)] +
    [_dw(4, (8, 32), 160, f, cout=192) for f in ((1, 7), (7, 1))] +
    [_dw(4, (16, 64), 3, (7, 7), st=(2, 2))] +
    [_dw(32, (16, 64), 64, (3, 3))] +
    # 4x56 minimises to 8x4 patches: the q tail of a 32x1 patch, at
    # ResNet's stage-3 width (28 of 32)
    [_dw(8, (4, 28), 64, (3, 3))])

EDGE_CASES = [
    _dw(4, (8, 32), 64, (3, 3), cout=136),
    _dw(11, (4, 16), 64, (3, 3)),           # M = 704 < 768
    _dw(4, (8, 32), 8, (1, 73))]            # r*s*8 = 584 > 576: no CS

KERNEL_CASES = [cs for cs in WIDE_CASES if cs.c % 8 == 0]


def _plan(cs):
    p, q, ph, pw = cs.pq
    return tf._core.conv_dw_wide_plan(cs.n, cs.h, cs.w, _up(cs.c, 8), cs.r,
                                      cs.s, cs.cout, cs.sh, cs.sw, ph, pw, p,
                                      q)


def test_plan():
    for cs in WIDE_CASES:
        p, q, _, _ = cs.pq
        assert cs.h != cs.w and cs.n * p * q % 64 == 0, cs.id
        assert cs.n * p * q >= 768, cs.id
        assert _plan(cs) is not None, cs.id
        assert _plan(cs)[5] <= 160 * 1024, cs.id
    for cs in EDGE_CASES + list(DW_CASES):
        assert _plan(cs) is None, cs.id
    resnet = {
        _dw(256, (28, 28), 128, (3, 3), cout=128): (64, 32, 1, 2, 1),
        _dw(256, (14, 14), 256, (3, 3), cout=256): (64, 16, 2, 4, 2),
        _dw(256, (7, 7), 512, (3, 3), cout=512): (64, 8, 4, 8, 4),
        _dw(256, (14, 14), 1024, (1, 1), cout=2048, st=(2, 2)):
            (512, 8, 4, 2, 16)}
    for cs, want in resnet.items():
        assert _plan(cs)[:5] == want, cs.id
        assert _plan(cs)[5] <= 160 * 1024, cs.id
    # what the table is there for: (CS, PW, PH, channel slices, cout slices)
    got = {cs.id: _plan(cs)[:5] for cs in WIDE_CASES}
    assert got[WIDE_CASES[1].id] == (64, 32, 1, 2, 1)
    assert got[WIDE_CASES[3].id] == (64, 32, 1, 1, 2)       # cout 192
    assert got[WIDE_CASES[4].id][1:3] == (16, 2)
    assert got[WIDE_CASES[5].id][1:3] == (8, 4)
    assert got[WIDE_CASES[6].id][1:3] == (8, 4)             # 4x56: 7 x 1
    assert got[WIDE_CASES[17].id][1:3] == (32, 1)           # 4x28
    assert got[WIDE_CASES[11].id] == (512, 32, 1, 2, 1)
    assert got[WIDE_CASES[12].id] == (16, 32, 1, 3, 1)      # 5x5
    assert got[WIDE_CASES[13].id] == (80, 32, 1, 2, 2)      # 1x7
    assert got[WIDE_CASES[15].id] == (8, 32, 1, 1, 1)       # padded stem


@pytest.mark.parametrize('cs', WIDE_CASES + EDGE_CASES, ids=lambda cs: cs.id)
def test_reference_conditions(cs):
    """The exactness conditions on the inputs (asserted inside _build): the
    reference side alone, no GPU."""
    for fam, a, b, side, want in _build(cs):
        assert np.array_equal(_bf16(a), a) and np.array_equal(_bf16(b), b)


def _bits(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) >> 16) \
        .astype(np.uint16)


@pytest.mark.gpu
@pytest.mark.parametrize('cs', KERNEL_CASES, ids=lambda cs: cs.id)
def test_kernel(cs):
    """One launch into a zeroed f32 accumulator: sums are multiples of 1/16
    below 2^20, so the float64 reference is representable and must match."""
    _, _, ph, pw = cs.pq
    for fam, x, dy, _, _ in _build(cs):
        got = tf._core.conv2d_dw_wide(_bits(x), _bits(dy), cs.r, cs.s, cs.sh,
                                      cs.sw, ph, pw)
        want = _ref_dw(cs, x, dy).reshape(-1, cs.cout)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.astype(np.float64), want), (cs.id, fam)


@pytest.mark.gpu
@pytest.mark.parametrize('cs', WIDE_CASES, ids=lambda cs: cs.id)
def test_conv2d_backprop_filter_wide(sess, cs):
    _run(sess, cs)


@pytest.mark.gpu
@pytest.mark.parametrize('cs', EDGE_CASES, ids=lambda cs: cs.id)
def test_conv2d_backprop_filter_gate_edge(sess, cs):
    _run(sess, cs)
