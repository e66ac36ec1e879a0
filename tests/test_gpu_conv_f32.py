"""Bit-exact tests of the float32 Conv2D, Conv2DBackpropInput(Add) and
Conv2DBackpropFilter GPU ops (csrc/kernels/gpu_conv.cc over
hip/conv_f32.hip), each fetched with a trace that shows its node ran on the
GPU.

Reference and operands are those of test_gpu_conv.py: float64 tap loops, and
the families 'int', 'mantA', 'mantB' whose products and partial sums are
multiples of 1/16 below 2^20. Those are bf16-representable, so a kernel that
rounded its operands to bf16 would pass them; family 'wide' has a rich operand
of random-signed integers 4096 + j, 0 <= j < 4096 (13 significant bits)
against the sparse {-1, 0, 1} one. With sum |a||b| below 2^24 (2^20 for the
1/16 families) every partial sum is an f32 value in any order, dW's atomics
included: the tolerance is zero, want = f32(exact) (+ side, integers in
[-3, 3]).

GEOMS holds the smallest shapes that reach each thing the kernel can get
wrong; each runs as fwd, dx, dx + side and dw."""
import zlib

import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.framework import dtypes
from simple_tensorflow_amd.python.framework.ops import (apply_op,
                                                        convert_to_tensor)

from test_gpu_conv import Case, _ref_dw, _ref_dx, _ref_fwd
from test_gpu_gemm import (_assert_equal, _feed, _rich, _sparse, _sessions,
                           sess)  # noqa: F401  (the fixtures)
from test_gpu_kernels import _bf16
from test_gpu_nn import _trace_run

FAMILIES = ('int', 'mantA', 'mantB', 'wide')
REFS = {'fwd': _ref_fwd, 'dw': _ref_dw, 'dx': _ref_dx}

# (n, h, w, c, r, s, cout, sh, sw, padding)
GEOMS = [
    # scalar gather; K = 25, no multiple of 4 or 16; M = 192: 1.5 row tiles
    (2, 8, 12, 1, 5, 5, 32, 1, 1, 'SAME'),
    # odd asymmetric SAME padding, strided dx, cout and M tails
    (2, 9, 13, 3, 3, 3, 20, 2, 2, 'SAME'),
    (1, 8, 32, 8, 3, 3, 64, 1, 1, 'SAME'),      # 16-byte path, exact tiles
    (1, 16, 32, 12, 1, 7, 24, 2, 1, 'SAME'),    # independent sh and sw,
    (1, 8, 64, 12, 7, 1, 24, 1, 2, 'SAME'),     # long thin filters
    (2, 8, 32, 16, 1, 1, 72, 1, 1, 'SAME'),     # no gather; column tile of 8
    (1, 8, 32, 8, 2, 2, 16, 1, 1, 'SAME'),      # pad_before < pad_after
    (2, 7, 9, 8, 5, 3, 16, 1, 1, 'VALID'),      # M = 2*3*7 = 42 < one tile
]
CASES = [Case(op, *g, side) for g in GEOMS
         for op, side in (('fwd', False), ('dx', False), ('dx', True),
                          ('dw', False))]
# M = 1024 pixels into a 72 x 16 dW: several slices, added with atomics
CASES.append(Case('dw', 4, 8, 32, 8, 3, 3, 16, 1, 1, 'SAME', False))


def _operands(cs, fam):
    """(operand 1, operand 2, side or None, expected) of one family, with the
    conditions that make f32 accumulation exact asserted on the inputs."""
    p, q, _, _ = cs.pq
    x_shape = (cs.n, cs.h, cs.w, cs.c)
    w_shape = (cs.r, cs.s, cs.c, cs.cout)
    dy_shape = (cs.n, p, q, cs.cout)
    (sa, sb), kc = {'fwd': ((x_shape, w_shape), cs.r * cs.s * cs.c),
                    'dw': ((x_shape, dy_shape), cs.n * p * q),
                    'dx': ((dy_shape, w_shape), cs.r * cs.s * cs.cout)}[cs.op]
    rng = np.random.RandomState(
        zlib.crc32(('%s/%s' % (cs.id, fam)).encode()) % 2**31)
    if fam == 'wide':
        a = (rng.choice([-1.0, 1.0], sa) *
             (4096 + rng.randint(0, 4096, sa))).astype(np.float32)
        b = _sparse(rng, sb, kc)
        assert not np.array_equal(_bf16(a), a)
    elif fam == 'mantB':
        a, b = _sparse(rng, sa, kc), _rich(rng, sb, fam)
    else:
        a, b = _rich(rng, sa, fam), _sparse(rng, sb, kc)
    bound = 2.0 ** 24 if fam == 'wide' else 2.0 ** 20
    assert REFS[cs.op](cs, np.abs(a), np.abs(b)).max() < bound, (cs.id, fam)
    exact = REFS[cs.op](cs, a, b)
    side = None
    if cs.side:
        side = rng.randint(-3, 4, x_shape).astype(np.float32)
        exact = exact + side
    return a, b, side, (exact + 0.0).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize('cs', CASES, ids=lambda cs: cs.id)
def test_conv2d_f32(sess, cs):
    strides, feeds, ops, wants = [1, cs.sh, cs.sw, 1], {}, [], []
    for fam in FAMILIES:
        a, b, side, want = _operands(cs, fam)
        a, b = _feed(feeds, a, tf.float32), _feed(feeds, b, tf.float32)
        sizes = [cs.n, cs.h, cs.w, cs.c]
        if cs.op == 'fwd':
            op = tf.nn.conv2d(a, b, strides, cs.padding)
        elif cs.op == 'dw':
            op = tf.nn.conv2d_backprop_filter(
                a, [cs.r, cs.s, cs.c, cs.cout], b, strides, cs.padding)
        elif side is None:
            op = tf.nn.conv2d_backprop_input(sizes, b, a, strides, cs.padding)
        else:
            op = apply_op('Conv2DBackpropInputAdd',
                          convert_to_tensor(sizes, dtype=dtypes.int32), b, a,
                          _feed(feeds, side, tf.float32), strides=strides,
                          padding=cs.padding)
        ops.append(op)
        wants.append(want)
    outs, on_gpu = _trace_run(sess, ops, feeds)
    for fam, op, out, want in zip(FAMILIES, ops, outs, wants):
        assert op.op.name in on_gpu, (cs.id, op.op.type, sorted(on_gpu))
        _assert_equal('%s %s' % (cs.id, fam), out, want)


@pytest.mark.gpu
def test_two_layer_net_gradients_run_on_gpu(sess):
    """tf.layers.conv2d twice, a residual add and tf.gradients: all four conv
    ops are placed on the GPU, and on 'int' operands (every sum an integer
    far below 2^24) the gradients equal those of the same graph on the CPU."""
    rng = np.random.RandomState(5)
    feeds = {}
    x = _feed(feeds, _rich(rng, (2, 8, 12, 4), 'int'), tf.float32)
    gy = _feed(feeds, _sparse(rng, (2, 8, 12, 8), 72), tf.float32)
    k1, k2 = _sparse(rng, (3, 3, 4, 8), 36), _sparse(rng, (3, 3, 8, 8), 72)
    grads = {}
    for dev in ('cpu', 'gpu'):
        with tf.device('/cpu:0' if dev == 'cpu' else None):
            h = tf.layers.conv2d(
                x, 8, 3, padding='same', use_bias=False, name=dev + '1',
                kernel_initializer=tf.constant_initializer(k1))
            y = tf.layers.conv2d(
                h, 8, 3, padding='same', use_bias=False, name=dev + '2',
                kernel_initializer=tf.constant_initializer(k2))
            loss = tf.reduce_sum((y + h) * gy)
            kernels = [v for v in tf.trainable_variables()
                       if v.name.startswith(dev)]
            assert len(kernels) == 2
            grads[dev] = tf.gradients(loss, [x] + kernels)
    sess.run(tf.variables_initializer(tf.trainable_variables()))
    outs, on_gpu = _trace_run(sess, grads['cpu'] + grads['gpu'], feeds)
    ran = {op.type for op in tf.get_default_graph().get_operations()
           if op.name in on_gpu}
    for kind in ('Conv2D', 'Conv2DBackpropFilter', 'Conv2DBackpropInput',
                 'Conv2DBackpropInputAdd'):
        assert kind in ran, (kind, sorted(ran))
    for name, cpu, gpu in zip(('dx', 'dk1', 'dk2'), outs[:3], outs[3:]):
        assert np.abs(cpu).max() > 0, name
        _assert_equal('net ' + name, gpu, cpu)


@pytest.mark.gpu
def test_split_dw_replayed_from_a_captured_step(sess):
    """A step without feeds or fetches is captured into a hipGraph on its
    third run and replayed from then on. The split dW (zero fill, then 8
    slices of atomics) still gives the exact result on the fifth run."""
    cs = CASES[-1]
    a, b, _, want = _operands(cs, 'wide')
    x, dy = tf.Variable(a), tf.Variable(b)
    out = tf.Variable(np.full(want.shape, 7.0, np.float32))
    dw = tf.nn.conv2d_backprop_filter(x.ref(), list(want.shape), dy.ref(),
                                      [1, cs.sh, cs.sw, 1], cs.padding)
    step = tf.assign(out, dw).op
    sess.run(tf.variables_initializer([x, dy, out]))
    for _ in range(5):
        sess.run(step)
    _assert_equal(cs.id, sess.run(tf.identity(out.ref())), want)
