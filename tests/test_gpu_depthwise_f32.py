"""Bit-exact tests of the float32 DepthwiseConv2dNative, ...BackpropInput and
...BackpropFilter GPU ops (csrc/kernels/gpu_conv.cc over
hip/depthwise_f32.hip), fetched with a trace that shows each node ran on the
GPU.

Reference and operands are those of test_gpu_conv_f32.py: the float64 tap
loops of test_gpu_nn._depthwise_ref, the families 'int', 'mantA', 'mantB'
(multiples of 1/16, sum |a||b| < 2^20) and 'wide' (13 significant bits
against {-1, 0, 1}, sum |a||b| < 2^24; a kernel that rounded to bf16 fails
it). Every partial sum is then an f32 value in any order, dW's cross-block
atomics included: the tolerance is zero, want = f32(exact).

GEOMS holds the smallest shapes that reach each thing the kernel can get
wrong. Its tiles: 32 channels, patches of 8 x 16 output pixels (16 x 8 when
the output is at most 8 wide)."""
import zlib

import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.framework.ops import apply_op

from test_gpu_gemm import (_assert_equal, _feed, _rich, _sparse, _sessions,
                           sess)  # noqa: F401  (the fixtures)
from test_gpu_kernels import _bf16
from test_gpu_nn import _depthwise_ref, _geom, _trace_run

FAMILIES = ('int', 'mantA', 'mantB', 'wide')
OPS = ('fwd', 'dx', 'dw')

# (x shape, (R, S, mult), (sh, sw), padding, ops)
GEOMS = [
    # VEC 4 baseline, two images, partial patches both ways
    ((2, 9, 13, 8), (3, 3, 1), (1, 1), 'SAME', OPS),
    # one full channel slice + a 4-wide tail; odd sizes, asymmetric SAME
    # padding; strided dx phases
    ((2, 9, 13, 36), (3, 3, 1), (2, 2), 'SAME', OPS),
    # several patches per image both ways: halos across patch borders;
    # 100-accumulator dW
    ((1, 20, 40, 4), (5, 5, 1), (1, 1), 'SAME', OPS),
    ((1, 16, 33, 8), (1, 7, 1), (2, 1), 'SAME', OPS),   # independent sh, sw
    ((1, 8, 64, 8), (7, 1, 1), (1, 2), 'SAME', OPS),    # long thin filters
    ((2, 7, 9, 8), (5, 3, 1), (1, 1), 'VALID', OPS),    # output 3 x 7 < patch
    # VEC 1: C not a multiple of 4, mult 2, pad_before < pad_after filter
    ((1, 8, 10, 5), (3, 2, 2), (1, 1), 'VALID', OPS),
    ((2, 9, 9, 4), (3, 3, 3), (2, 2), 'SAME', OPS),     # VEC 1 by mult alone;
                                                        # dx sums over m
    ((2, 7, 7, 3), (1, 1, 1), (2, 2), 'VALID', OPS),    # no halo, C = 3
    # 2048 pixels: 8 workers per slice, added with atomics after the zero fill
    ((4, 16, 32, 8), (3, 3, 1), (1, 1), 'SAME', ('dw',)),
]


def _geom_id(geom):
    (n, h, w, c), (r, s, mult), (sh, sw), padding, _ = geom
    return '%dx%dx%dx%d-%dx%dm%d-s%d%d-%s' % (n, h, w, c, r, s, mult, sh, sw,
                                              padding)


def _operands(geom, op, fam):
    """(x, w, dy, g, expected) of one op and family: its two operands and a
    zero third, with the conditions that make f32 accumulation exact asserted
    on the inputs."""
    (n, h, w, c), (r, s, mult), strides, padding, _ = geom
    g = _geom(h, w, (r, s), strides, padding)
    shapes = {'x': (n, h, w, c), 'w': (r, s, c, mult),
              'dy': (n, g.P, g.Q, c * mult)}
    (na, nb), kc = {'fwd': (('x', 'w'), r * s),
                    'dx': (('dy', 'w'), r * s * mult),
                    'dw': (('x', 'dy'), n * g.P * g.Q)}[op]
    sa, sb = shapes[na], shapes[nb]
    rng = np.random.RandomState(
        zlib.crc32(('%s/%s/%s' % (_geom_id(geom), op, fam)).encode()) % 2**31)
    if fam == 'wide':
        a = (rng.choice([-1.0, 1.0], sa) *
             (4096 + rng.randint(0, 4096, sa))).astype(np.float32)
        b = _sparse(rng, sb, kc)
        assert not np.array_equal(_bf16(a), a)
    elif fam == 'mantB':
        a, b = _sparse(rng, sa, kc), _rich(rng, sb, fam)
    else:
        a, b = _rich(rng, sa, fam), _sparse(rng, sb, kc)
    t = {k: np.zeros(v, np.float32) for k, v in shapes.items()}
    t[na], t[nb] = a, b
    exact, exact_abs = _depthwise_ref(t['x'], t['w'], t['dy'],
                                      g)[OPS.index(op)]
    assert exact_abs.max() < (2.0 ** 24 if fam == 'wide' else 2.0 ** 20)
    return t['x'], t['w'], t['dy'], g, (exact + 0.0).astype(np.float32)


def _build(geom, op, x, w, dy):
    (n, h, wd, c), (r, s, mult), (sh, sw), padding, _ = geom
    attrs = dict(strides=[1, sh, sw, 1], padding=padding)
    if op == 'fwd':
        return tf.nn.depthwise_conv2d(x, w, **attrs)
    if op == 'dx':
        return apply_op('DepthwiseConv2dNativeBackpropInput',
                        tf.constant([n, h, wd, c], dtype=tf.int32), w, dy,
                        **attrs)
    return apply_op('DepthwiseConv2dNativeBackpropFilter', x,
                    tf.constant([r, s, c, mult], dtype=tf.int32), dy, **attrs)


@pytest.mark.gpu
@pytest.mark.parametrize('geom', GEOMS, ids=_geom_id)
def test_depthwise_f32(sess, geom):
    feeds, labels, ops, wants = {}, [], [], []
    for op in geom[4]:
        for fam in FAMILIES:
            x, w, dy, _, want = _operands(geom, op, fam)
            x, w, dy = (_feed(feeds, a, tf.float32) for a in (x, w, dy))
            ops.append(_build(geom, op, x, w, dy))
            wants.append(want)
            labels.append('%s %s %s' % (_geom_id(geom), op, fam))
    outs, on_gpu = _trace_run(sess, ops, feeds)
    for label, op, out, want in zip(labels, ops, outs, wants):
        assert op.op.name in on_gpu, (label, op.op.type, sorted(on_gpu))
        _assert_equal(label, out, want)


@pytest.mark.gpu
def test_separable_block_gradients_run_on_gpu(sess):
    """tf.nn.separable_conv2d (3x3 depthwise, mult 1, then 1x1) twice, a
    residual add and tf.gradients: the three depthwise ops are placed on the
    GPU, and on 'int' operands (every sum an integer far below 2^24) the
    gradients equal those of the same graph on the CPU."""
    rng = np.random.RandomState(5)
    feeds = {}
    x = _feed(feeds, _rich(rng, (2, 8, 12, 8), 'int'), tf.float32)
    gy = _feed(feeds, _sparse(rng, (2, 8, 12, 8), 72), tf.float32)
    d1, d2 = (_sparse(rng, (3, 3, 8, 1), 9) for _ in range(2))
    p1, p2 = (_sparse(rng, (1, 1, 8, 8), 8) for _ in range(2))
    grads = {}
    for dev in ('cpu', 'gpu'):
        with tf.device('/cpu:0' if dev == 'cpu' else None):
            k = [tf.Variable(v, name='%s%d' % (dev, i))
                 for i, v in enumerate((d1, p1, d2, p2))]
            h = tf.nn.separable_conv2d(x, k[0], k[1], [1, 1, 1, 1], 'SAME')
            y = tf.nn.separable_conv2d(h, k[2], k[3], [1, 1, 1, 1], 'SAME')
            loss = tf.reduce_sum((y + h) * gy)
            grads[dev] = tf.gradients(loss, [x, k[0], k[2]])
            sess.run(tf.variables_initializer(k))
    outs, on_gpu = _trace_run(sess, grads['cpu'] + grads['gpu'], feeds)
    ran = {op.type for op in tf.get_default_graph().get_operations()
           if op.name in on_gpu}
    for kind in ('DepthwiseConv2dNative', 'DepthwiseConv2dNativeBackpropInput',
                 'DepthwiseConv2dNativeBackpropFilter'):
        assert kind in ran, (kind, sorted(ran))
    for name, cpu, gpu in zip(('dx', 'dd1', 'dd2'), outs[:3], outs[3:]):
        assert np.abs(cpu).max() > 0, name
        _assert_equal('block ' + name, gpu, cpu)


@pytest.mark.gpu
def test_depthwise_dw_replayed_from_a_captured_step(sess):
    """A step without feeds or fetches is captured into a hipGraph on its
    third run and replayed from then on. The dW of several workers (zero fill
    by a kernel, then atomics) still gives the exact result on the fifth
    run."""
    geom = GEOMS[-1]
    a, _, b, _, want = _operands(geom, 'dw', 'wide')
    x, dy = tf.Variable(a), tf.Variable(b)
    out = tf.Variable(np.full(want.shape, 7.0, np.float32))
    step = tf.assign(out, _build(geom, 'dw', x.ref(), None, dy.ref())).op
    sess.run(tf.variables_initializer([x, dy, out]))
    for _ in range(5):
        sess.run(step)
    _assert_equal(_geom_id(geom), sess.run(tf.identity(out.ref())), want)
