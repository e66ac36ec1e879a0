"""MaxPoolGradTiled (csrc/kernels/hip/pool.hip): the tiled gradient kernel
that bf16, C % 8 == 0 max pools with 3x3 windows of stride 2 run.

The tile is a core of 16 x 16 input pixels by 32 channels, the shape the
kernel was first written for, so the sizes below are the ones its design
names:

  9x9 SAME     N 2 C 8    one partial tile, ph = pw = 1
  16x16 SAME   N 3 C 40   ph = 0, exactly one core, a slice past C
  17x33 SAME   N 2 C 64   tile tails in both directions, windows that
                          straddle cores
  37x20 SAME   N 2 C 72   three tile rows, two slices plus a tail
  10x10 VALID  N 2 C 8    last row and column uncovered: written as zero
  35x35 VALID  N 1 C 96   Inception's reduction geometry, small

What is asserted:
  1. against numpy's first-argmax reference, bit-equal, on `ties` data (what
     a ReLU leaves) and on `unique` data (every (n, c) plane a permutation of
     H*W distinct bf16 values; the integers 0..H*W-1 of test_gpu_nn.py stop
     being exact in bf16 at 256, so the values here are the H*W bf16 numbers
     that follow 1.0), with integer dy in [-3, 3];
  2. against MaxPoolGradKernelV8, which STF_NO_TILED_MAXPOOL_GRAD=1 selects
     for a fresh graph in the same process: equal bit patterns on random
     normal dy, where the order of the f32 adds shows, and on x with NaN,
     +inf and -inf scattered in and one window of each all -inf and all NaN;
  3. that every element of dx is written, after a step that leaves NaN in
     the buffers the allocator hands out next.

The project has no per-kernel launch counter, so that the gated cases run
the tiled kernel (and 2x2/2 does not) is covered only by assertion 2, where
the two settings would otherwise run the same code, and by the kernel trace
in profiles/resnet50_max_pool_grad.md."""
import collections
import os

import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.framework.ops import apply_op

pytestmark = pytest.mark.gpu

ENV = 'STF_NO_TILED_MAXPOOL_GRAD'

# (H, W, padding, N, C), all 3x3 windows of stride 2
CASES = [
    (9, 9, 'SAME', 2, 8),
    (16, 16, 'SAME', 3, 40),
    (17, 33, 'SAME', 2, 64),
    (37, 20, 'SAME', 2, 72),
    (10, 10, 'VALID', 2, 8),
    (35, 35, 'VALID', 1, 96),
]
CASE_IDS = ['%dx%d-%s-n%d-c%d' % c for c in CASES]


def _bf16(x):
    """round-trip f32 -> bf16 -> f32 (numpy)"""
    bits = np.asarray(x, np.float32).view(np.uint32)
    lsb = (bits >> 16) & 1
    out = ((bits + 0x7FFF + lsb) >> 16).astype(np.uint32) << 16
    return out.view(np.float32)


def _bits(a):
    a = np.ascontiguousarray(np.asarray(a, np.float32))
    return a.view(np.uint32)


Geom = collections.namedtuple('Geom', 'H W kh kw sh sw ph pw P Q')


def _geom(H, W, padding):
    kh = kw = 3
    sh = sw = 2
    if padding == 'SAME':
        P, Q = -(-H // sh), -(-W // sw)
        ph = max(0, (P - 1) * sh + kh - H) // 2
        pw = max(0, (Q - 1) * sw + kw - W) // 2
    else:
        P, Q = (H - kh) // sh + 1, (W - kw) // sw + 1
        ph = pw = 0
    return Geom(H, W, kh, kw, sh, sw, ph, pw, P, Q)


def _padded(a, g, fill):
    """a (N, H, W, C) inside a frame of `fill` wide enough for every tap."""
    n, _, _, c = a.shape
    ap = np.full((n, g.ph + g.H + g.kh + g.sh, g.pw + g.W + g.kw + g.sw, c),
                 fill, a.dtype)
    ap[:, g.ph:g.ph + g.H, g.pw:g.pw + g.W] = a
    return ap


def _tap(ap, g, a, b):
    """View (N, P, Q, C) of the padded array: element (a, b) of every
    window."""
    return ap[:, a:a + (g.P - 1) * g.sh + 1:g.sh,
              b:b + (g.Q - 1) * g.sw + 1:g.sw]


def _taps(g):
    """Window offsets in row-major scan order."""
    return [(a, b) for a in range(g.kh) for b in range(g.kw)]


def _max_pool_grad_ref(x, dy, g):
    """dx with every dy routed to np.argmax of its window in row-major scan
    order, that is to the first maximum."""
    xp = _padded(x, g, -np.inf)
    wins = np.stack([_tap(xp, g, a, b) for a, b in _taps(g)], -1)
    arg = wins.argmax(-1)
    dxp = np.zeros(xp.shape, np.float64)
    for k, (a, b) in enumerate(_taps(g)):
        view = _tap(dxp, g, a, b)
        view += np.where(arg == k, dy, 0.0)
    return dxp[:, g.ph:g.ph + g.H, g.pw:g.pw + g.W]


def _x(rng, data, N, H, W, C):
    if data == 'ties':
        # what a ReLU leaves: many ties and all-zero windows
        return np.maximum(rng.randint(-3, 3, (N, H, W, C)), 0).astype(
            np.float32)
    # every (n, c) plane a permutation of the H*W bf16 values after 1.0
    vals = ((0x3F80 + np.arange(H * W, dtype=np.uint32)) << 16).view(
        np.float32)
    assert np.isfinite(vals).all() and np.unique(vals).size == H * W
    return np.stack([np.stack([vals[rng.permutation(H * W)].reshape(H, W)
                               for _ in range(C)], axis=-1)
                     for _ in range(N)])


def _specials(rng, N, H, W, C, g):
    """bf16 normal x with NaN, +inf and -inf scattered in, the window
    (p, q) = (1, 1) of image 0 all -inf and the window (3, 2) all NaN."""
    x = _bf16(rng.randn(N, H, W, C))
    kind = rng.randint(0, 40, x.shape)
    x[kind == 0] = np.nan
    x[kind == 1] = np.inf
    x[kind == 2] = -np.inf
    for (p, q), v in (((1, 1), -np.inf), ((3, 2), np.nan)):
        assert p < g.P and q < g.Q
        h, w = p * 2 - g.ph, q * 2 - g.pw
        assert h >= 0 and w >= 0 and h + 3 <= H and w + 3 <= W
        x[0, h:h + 3, w:w + 3] = v
    return x


def _feed(feeds, x):
    """bf16 tensor fed with x: it goes in as f32 and is cast on the device
    (exact: x is already bf16-rounded)."""
    p = tf.placeholder(tf.float32, list(x.shape))
    feeds[p] = x
    return tf.cast(p, tf.bfloat16)


def _grad(feeds, x, dy, ksize=3, stride=2, padding='SAME'):
    attrs = dict(ksize=[1, ksize, ksize, 1], strides=[1, stride, stride, 1],
                 padding=padding)
    xt = _feed(feeds, x)
    y = apply_op('MaxPool', xt, **attrs)
    return apply_op('MaxPoolGrad', xt, y, _feed(feeds, dy), **attrs)


def _run(inputs, tiled, poison=False):
    """dx of every (x, dy, padding) in a fresh graph and session, which is
    what makes MaxPoolGrad read the setting again."""
    saved = os.environ.pop(ENV, None)
    if not tiled:
        os.environ[ENV] = '1'
    try:
        tf.reset_default_graph()
        with tf.Session() as s:
            assert s.num_gpus() > 0
            if poison:
                # the same op at the largest shape, with NaN for every dy,
                # and NaN tensors of each dx's own size: the next buffers
                # of these sizes come back dirty
                pf, pfetch = {}, []
                nan_big = np.full((4, 37, 37, 96), np.nan, np.float32)
                pfetch.append(_grad(pf, np.zeros((4, 74, 74, 96), np.float32),
                                    nan_big))
                for x, _, _ in inputs:
                    pfetch.append(_feed(pf, np.full(x.shape, np.nan,
                                                    np.float32)))
                for out in s.run(pfetch, pf):
                    assert np.isnan(np.asarray(out, np.float32)).any()
            feeds = {}
            fetches = [_grad(feeds, x, dy, padding=padding)
                       for x, dy, padding in inputs]
            return [np.asarray(o, np.float32) for o in s.run(fetches, feeds)]
    finally:
        os.environ.pop(ENV, None)
        if saved is not None:
            os.environ[ENV] = saved


@pytest.mark.parametrize('data', ['unique', 'ties'])
def test_against_numpy(data):
    """Bit-equal to the first-argmax reference. dy is integers in [-3, 3],
    so the sums over overlapping windows are exact in bf16 too."""
    rng = np.random.RandomState(301)
    inputs, geoms = [], []
    for H, W, padding, N, C in CASES:
        g = _geom(H, W, padding)
        inputs.append((_x(rng, data, N, H, W, C),
                       rng.randint(-3, 4, (N, g.P, g.Q, C)).astype(
                           np.float32), padding))
        geoms.append(g)
    outs = _run(inputs, tiled=True)
    for label, g, (x, dy, _), got in zip(CASE_IDS, geoms, inputs, outs):
        ref = _max_pool_grad_ref(x, dy, g).astype(np.float32)
        assert got.shape == ref.shape, label
        bad = np.flatnonzero(_bits(got).ravel() != _bits(ref + 0.0).ravel())
        print('%s %s: %d of %d differ' % (label, data, bad.size, got.size))
        np.testing.assert_array_equal(got, ref, err_msg=label)
        assert bad.size == 0, (label, bad[:8])
        if _last_uncovered(g):
            # no window covers the last row or column: written as zero
            assert (got[:, g.H - 1] == 0).all(), label
            assert (got[:, :, g.W - 1] == 0).all(), label
        if data == 'ties':
            # every dy lands exactly once, whichever maximum takes it
            np.testing.assert_array_equal(got.sum((1, 2)), dy.sum((1, 2)),
                                          err_msg=label + ' plane sums')


def _last_uncovered(g):
    return (g.P - 1) * 2 - g.ph + 3 < g.H and (g.Q - 1) * 2 - g.pw + 3 < g.W


def _same_bits(label, new, old):
    for name, a, b in zip(CASE_IDS, new, old):
        bad = np.flatnonzero(_bits(a).ravel() != _bits(b).ravel())
        print('%s %s: %d of %d bit patterns differ'
              % (label, name, bad.size, a.size))
        assert bad.size == 0, (label, name, bad[:8])


def test_against_per_input_kernel_random_dy():
    """Random normal dy on ties data: several windows give to one pixel and
    the f32 adds are inexact, so their order shows in the bits."""
    rng = np.random.RandomState(302)
    inputs = []
    for H, W, padding, N, C in CASES:
        g = _geom(H, W, padding)
        inputs.append((_x(rng, 'ties', N, H, W, C),
                       _bf16(rng.randn(N, g.P, g.Q, C)), padding))
    new, old = _run(inputs, tiled=True), _run(inputs, tiled=False)
    _same_bits('random dy', new, old)
    # the comparison is not of two empty results
    assert all(np.count_nonzero(a) > a.size // 16 for a in new)


def test_against_per_input_kernel_nan_inf():
    """NaN and -inf never win, +inf does, a window without a winner drops
    its dy: whatever the per-input kernel does, bit for bit."""
    rng = np.random.RandomState(303)
    inputs = []
    for H, W, padding, N, C in CASES:
        g = _geom(H, W, padding)
        inputs.append((_specials(rng, N, H, W, C, g),
                       _bf16(rng.randn(N, g.P, g.Q, C)), padding))
    new, old = _run(inputs, tiled=True), _run(inputs, tiled=False)
    _same_bits('nan/inf x', new, old)


def test_every_element_written():
    """The op's output buffer is not cleared: after a step that left NaN in
    buffers of these sizes, dx still equals the reference everywhere, the
    zeros of pixels that no window covers or that win nothing included."""
    rng = np.random.RandomState(304)
    inputs, geoms = [], []
    for H, W, padding, N, C in CASES:
        g = _geom(H, W, padding)
        inputs.append((_x(rng, 'ties', N, H, W, C),
                       rng.randint(-3, 4, (N, g.P, g.Q, C)).astype(
                           np.float32), padding))
        geoms.append(g)
    outs = _run(inputs, tiled=True, poison=True)
    for label, g, (x, dy, _), got in zip(CASE_IDS, geoms, inputs, outs):
        assert not np.isnan(got).any(), label
        np.testing.assert_array_equal(
            got, _max_pool_grad_ref(x, dy, g).astype(np.float32),
            err_msg=label)


def test_other_geometry_unchanged():
    """2x2 windows of stride 2 are outside the gate: both settings give the
    reference."""
    rng = np.random.RandomState(305)
    x = np.maximum(rng.randint(-3, 3, (2, 8, 8, 8)), 0).astype(np.float32)
    dy = rng.randint(-3, 4, (2, 4, 4, 8)).astype(np.float32)
    ref = np.zeros(x.shape, np.float32)
    for p in range(4):
        for q in range(4):
            win = x[:, 2 * p:2 * p + 2, 2 * q:2 * q + 2].reshape(2, 4, 8)
            k = win.argmax(1)
            for n in range(2):
                for c in range(8):
                    ref[n, 2 * p + k[n, c] // 2, 2 * q + k[n, c] % 2, c] += \
                        dy[n, p, q, c]
    for tiled in (True, False):
        tf.reset_default_graph()
        saved = os.environ.pop(ENV, None)
        if not tiled:
            os.environ[ENV] = '1'
        try:
            with tf.Session() as s:
                feeds = {}
                dx = _grad(feeds, x, dy, ksize=2, stride=2, padding='VALID')
                got = np.asarray(s.run(dx, feeds), np.float32)
        finally:
            os.environ.pop(ENV, None)
            if saved is not None:
                os.environ[ENV] = saved
        np.testing.assert_array_equal(got, ref)
