"""QuantizedAvgPool, QuantizedRelu6 and QuantizedConcat on the CPU
(csrc/kernels/cpu_quantized.cc), and quantize_nodes on an Inception-style
block: parallel branches, average pooling, channel concat and a
global-average-pool head, in quint8 from one QuantizeV2 to one Dequantize.

As in test_quantized_inference.py, whose helpers this file reuses, every op
is checked with np.array_equal against a numpy implementation of its formula
written here, and the transformed graph against a numpy emulation of the
whole pipeline. Everything is pinned to /cpu:0;
tests/test_gpu_quantized_inception.py holds the GPU side.
"""
import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.framework import pbreader
from simple_tensorflow_amd.python.framework.ops import apply_op
from simple_tensorflow_amd.python.ops import quantized_ops as q
from simple_tensorflow_amd.python.tools import (quantize_graph_lib,
                                                transform_graph)

from test_quantized_inference import (F32, POOL_CASES, POOL_CHANNELS, RANGES,
                                      _check, _run_cpu, _windows,
                                      np_bias_add, np_conv2d,
                                      np_dequantize_u8, np_matmul,
                                      np_max_pool, np_quantize_const,
                                      np_quantize_v2, np_relu, np_requantize,
                                      np_requantization_range, np_step,
                                      np_zero_point, op_census, pin, rel_l2,
                                      run_graph)


def setup_function(_):
    tf.reset_default_graph()


# ---------------------------------------------------------------------------
# numpy specification of the three ops
# ---------------------------------------------------------------------------
def np_avg_pool(xq, ksize, strides, padding):
    """Sum of the taps inside the image over their number, truncating."""
    args = (ksize[1], ksize[2], strides[1], strides[2], padding, 0)
    total = _windows(xq.astype(np.int64), *args).sum(axis=(3, 4))
    taps = _windows(np.ones(xq.shape[:3] + (1,), np.int64), *args) \
        .sum(axis=(3, 4))
    return (total // taps).astype(np.uint8)


def np_relu6_bounds(mn, mx):
    lo = min(max(np_zero_point(mn, mx), 0), 255)
    hi = int(np_quantize_v2(np.array([6.0], F32), mn, mx)[0][0])
    return lo, hi


def np_relu6(xq, mn, mx):
    lo, hi = np_relu6_bounds(mn, mx)
    # max, then min: where hi < lo the result is hi
    return np.minimum(np.maximum(xq.astype(np.int32), lo), hi) \
        .astype(np.uint8)


def np_concat(axis, xs, mins, maxes):
    lo = F32(min([F32(0)] + [F32(m) for m in mins]))
    hi = F32(max(F32(m) for m in maxes))
    parts = []
    for x, mn, mx in zip(xs, mins, maxes):
        if F32(mn) == lo and F32(mx) == hi:
            parts.append(x)
        else:
            parts.append(np_quantize_v2(np_dequantize_u8(x, mn, mx), lo,
                                        hi)[0])
    return np.concatenate(parts, axis), lo, hi


# ---------------------------------------------------------------------------
# QuantizedAvgPool
# ---------------------------------------------------------------------------
POOL_IDS = ['%dx%d_k%d_s%d_%s' % (p[0], p[0], p[1], p[2], p[3])
            for p in POOL_CASES]


def avg_pool_input(case, c):
    hw = case[0]
    return np.random.RandomState(c + hw).randint(0, 256, (2, hw, hw, c)) \
        .astype(np.uint8)


@pytest.mark.parametrize('c', POOL_CHANNELS)
@pytest.mark.parametrize('case', POOL_CASES, ids=POOL_IDS)
def test_quantized_avg_pool(case, c):
    hw, k, stride, padding = case
    x = avg_pool_input(case, c)
    px = tf.placeholder(tf.uint8, x.shape)
    mn, mx = RANGES[c % 4]
    got = _run_cpu(lambda: q.quantized_avg_pool(
        px, mn, mx, [1, k, k, 1], [1, stride, stride, 1], padding), {px: x})
    want = np_avg_pool(x, [1, k, k, 1], [1, stride, stride, 1], padding)
    _check(got, [want, F32(mn), F32(mx)], 'QuantizedAvgPool')
    if padding == 'SAME' and k == 3 and c > 1:
        # border windows hold 4 or 6 taps: a kh*kw divisor gives less
        naive = (_windows(x.astype(np.int64), k, k, stride, stride, padding,
                          0).sum(axis=(3, 4)) // (k * k)).astype(np.uint8)
        assert not np.array_equal(naive, want)


# (image H = W, ksize, stride, padding, channels): every byte is 255, and so
# is every mean. 17 * 17 * 255 = 73 695 does not fit 16 bits; the 3x3 SAME
# image has windows of 4, 6 and 9 taps.
SATURATED_CASES = [(17, 17, 1, 'VALID', 16), (3, 3, 1, 'SAME', 16),
                   (3, 3, 1, 'SAME', 20)]


@pytest.mark.parametrize('case', SATURATED_CASES,
                         ids=['%dx%d_k%d_%s_c%d' % (p[0], p[0], p[1], p[3],
                                                   p[4])
                              for p in SATURATED_CASES])
def test_quantized_avg_pool_of_255_is_255(case):
    hw, k, stride, padding, c = case
    x = np.full((2, hw, hw, c), 255, np.uint8)
    px = tf.placeholder(tf.uint8, x.shape)
    got = _run_cpu(lambda: q.quantized_avg_pool(
        px, 0.0, 6.0, [1, k, k, 1], [1, stride, stride, 1], padding), {px: x})
    side = 1 if padding == 'VALID' else hw
    _check(got, [np.full((2, side, side, c), 255, np.uint8), F32(0.0),
                 F32(6.0)], 'QuantizedAvgPool of 255')
    if padding == 'SAME':
        taps = _windows(np.ones((1, hw, hw, 1), np.int64), k, k, stride,
                        stride, padding, 0).sum(axis=(3, 4))
        assert sorted(set(taps.ravel())) == [4, 6, 9]


@pytest.mark.parametrize('shape,k,match', [
    ((2, 2, 2, 1), 4, 'window larger'),
    ((2, 4, 4), 2, 'rank-4'),
], ids=['window', 'rank'])
def test_quantized_avg_pool_rejects(shape, k, match):
    """The argument checks are QuantizedMaxPool's."""
    px = tf.placeholder(tf.uint8, shape)
    with tf.device('/cpu:0'):
        outs = [apply_op(op, px, tf.constant(0.0), tf.constant(1.0),
                         ksize=[1, k, k, 1], strides=[1, 1, 1, 1],
                         padding='VALID')[0]
                for op in ('QuantizedAvgPool', 'QuantizedMaxPool')]
    with tf.Session() as s:
        for out, op in zip(outs, ('QuantizedAvgPool', 'QuantizedMaxPool')):
            with pytest.raises(Exception, match=op + '.*' + match):
                s.run(out, {px: np.zeros(shape, np.uint8)})


def test_quantized_avg_pool_shape():
    px = tf.placeholder(tf.uint8, (2, 7, 7, 48))
    out = q.quantized_avg_pool(px, 0.0, 1.0, [1, 3, 3, 1], [1, 2, 2, 1],
                               'SAME')
    assert tuple(out[0].get_shape().as_list()) == (2, 4, 4, 48)
    assert tuple(out[1].get_shape().as_list()) == ()


# ---------------------------------------------------------------------------
# QuantizedRelu6
# ---------------------------------------------------------------------------
RELU6_RANGES = RANGES + [(-1.0, 10.0), (7.0, 10.0), (0.0, 0.0)]
RELU6_SIZES = (1, 7, 1027)


def relu6_input(n):
    return np.resize(np.arange(256, dtype=np.uint8), n)


@pytest.mark.parametrize('n', RELU6_SIZES)
def test_quantized_relu6(n):
    x = relu6_input(n)
    for mn, mx in RELU6_RANGES:
        tf.reset_default_graph()
        px = tf.placeholder(tf.uint8, (n,))
        got = _run_cpu(lambda: q.quantized_relu6(px, mn, mx), {px: x})
        _check(got, [np_relu6(x, mn, mx), F32(mn), F32(mx)],
               'QuantizedRelu6 %r' % ((mn, mx),))
        if (mn, mx) == (-1.0, 10.0):
            # both clamps bind, on every byte value that is in x
            lo, hi = np_relu6_bounds(mn, mx)
            assert (lo, hi) == (23, 162) and lo < hi < 255
            assert np.array_equal(got[0][x <= lo],
                                  np.full((x <= lo).sum(), lo, np.uint8))
            assert np.array_equal(got[0][x >= hi],
                                  np.full((x >= hi).sum(), hi, np.uint8))
            assert (got[0] == lo).any()
            if n >= 256:
                assert (got[0] == hi).any()
                mid = (x > lo) & (x < hi)
                assert mid.any() and np.array_equal(got[0][mid], x[mid])


def test_quantized_relu6_clamps_where_relu_wraps():
    """(-4, -0.5) puts the zero point at 291: QuantizedRelu wraps it into
    the byte, QuantizedRelu6 clamps it."""
    x = relu6_input(256)
    assert np_zero_point(-4.0, -0.5) == 291
    px = tf.placeholder(tf.uint8, x.shape)
    got = _run_cpu(lambda: [q.quantized_relu6(px, -4.0, -0.5)[0],
                            q.quantized_relu(px, -4.0, -0.5)[0]], {px: x})
    assert np.all(got[0] == 255)
    assert np.all(got[1] == 291 - 256)
    # (7, 10): 6.0 lies below the range, the ceiling is 0
    assert np_relu6_bounds(7.0, 10.0) == (0, 0)


# ---------------------------------------------------------------------------
# QuantizedConcat
# ---------------------------------------------------------------------------
def _rank4(widths):
    return [(2, 5, 5, c) for c in widths]


# name -> (axis, input shapes)
CONCAT_CASES = {
    'vec_axis3': (3, _rank4((16, 32, 48))),
    'vec_axis-1': (-1, _rank4((16, 32, 48))),
    'bytes_axis3': (3, _rank4((3, 16, 5))),
    'bytes_axis-1': (-1, _rank4((3, 16, 5))),
    'axis0': (0, [(2, 3, 4, 5), (1, 3, 4, 5), (3, 3, 4, 5)]),
    'axis1': (1, [(2, 3, 4, 5), (2, 1, 4, 5), (2, 2, 4, 5)]),
    'axis2': (2, [(2, 3, 4, 5), (2, 3, 1, 5), (2, 3, 6, 5)]),
    'rank1': (0, [(1027,), (5,)]),
    'n2': (1, [(3, 16), (3, 7)]),
    'n4': (3, _rank4((16, 16, 32, 16))),
    'n17': (1, [(3, 1 + k % 5) for k in range(17)]),
    'zero_width': (3, _rank4((16, 0, 32, 8))),
}


def concat_range_sets(n):
    """name -> n (min, max) pairs."""
    different = [(-0.25 * (k + 1), 1.0 + 0.5 * k) for k in range(n)]
    different[:4] = RANGES[:min(4, n)]
    # the first and the last input have the range that becomes the output
    # range and are copied; the others lie inside it and are requantized
    shared = [(-2.0, 8.0)] + [(-1.0 + 0.01 * k, 1.0) for k in range(n - 2)] \
        + [(-2.0, 8.0)]
    if n == 2:
        shared = [(-2.0, 8.0), (-1.0, 1.0)]
    # output_min becomes 0, which is no input's minimum: nothing is copied
    positive = [(0.5 + 0.125 * k, 4.0 + k) for k in range(n)]
    return {'different': different, 'shared': shared, 'positive': positive,
            'degenerate': [(0.0, 0.0)] * n}


def concat_inputs(name):
    axis, shapes = CONCAT_CASES[name]
    rng = np.random.RandomState(len(name) + len(shapes))
    xs = [rng.randint(0, 256, s).astype(np.uint8) for s in shapes]
    for x in xs:
        x.reshape(-1)[:2] = [0, 255][:x.size]
    return axis, xs


@pytest.mark.parametrize('name', sorted(CONCAT_CASES))
def test_quantized_concat(name):
    axis, xs = concat_inputs(name)
    for set_name, ranges in concat_range_sets(len(xs)).items():
        tf.reset_default_graph()
        ps = [tf.placeholder(tf.uint8, x.shape) for x in xs]
        mins = [r[0] for r in ranges]
        maxes = [r[1] for r in ranges]
        got = _run_cpu(lambda: q.quantized_concat(axis, ps, mins, maxes),
                       dict(zip(ps, xs)))
        want = np_concat(axis, xs, mins, maxes)
        _check(got, want, 'QuantizedConcat %s %s' % (name, set_name))
        plain = np.concatenate(xs, axis)
        if set_name == 'degenerate':
            # the copy rule: requantizing under (0, 0) would give zeros
            assert want[1:] == (F32(0), F32(0))
            assert np.array_equal(got[0], plain) and plain.any()
            continue
        if set_name == 'positive':
            assert want[1] == 0 and all(m > 0 for m in mins)
        if set_name == 'shared':
            assert want[1:] == (F32(-2.0), F32(8.0))
            first = [slice(None)] * plain.ndim
            first[axis] = slice(0, xs[0].shape[axis])
            assert np.array_equal(got[0][tuple(first)], xs[0])
            assert not np.array_equal(got[0], plain)
        # independent of the formula: the output represents, within one
        # output step, the values the inputs represent
        before = np.concatenate(
            [np_dequantize_u8(x, mn, mx).astype(np.float64)
             for x, mn, mx in zip(xs, mins, maxes)], axis)
        after = np_dequantize_u8(got[0], got[1], got[2]).astype(np.float64)
        assert np.all(np.abs(after - before) <=
                      np.float64(np_step(got[1], got[2])))


def test_quantized_concat_shape():
    ps = [tf.placeholder(tf.uint8, (2, 5, 5, c)) for c in (16, 32, 48)]
    out = q.quantized_concat(-1, ps, [0.0] * 3, [1.0] * 3)
    assert tuple(out[0].get_shape().as_list()) == (2, 5, 5, 96)
    assert tuple(out[1].get_shape().as_list()) == ()
    assert tuple(out[2].get_shape().as_list()) == ()


@pytest.mark.parametrize('axis,shapes', [
    (0, [(2, 3), (2, 3, 1)]),          # a rank mismatch
    (1, [(2, 3), (3, 3)]),             # sizes differ off the concat axis
    (2, [(2, 3), (2, 3)]),             # concat_dim == rank
    (-3, [(2, 3), (2, 3)]),            # concat_dim < -rank
], ids=['rank', 'off_axis', 'dim_eq_rank', 'dim_below_-rank'])
def test_quantized_concat_rejects(axis, shapes):
    ps = [tf.placeholder(tf.uint8, s) for s in shapes]
    with tf.device('/cpu:0'):
        out = q.quantized_concat(axis, ps, [0.0, 0.0], [1.0, 1.0])[0]
    with tf.Session() as s:
        with pytest.raises(Exception, match='QuantizedConcat'):
            s.run(out, {p: np.zeros(sh, np.uint8)
                        for p, sh in zip(ps, shapes)})


# ---------------------------------------------------------------------------
# the Inception-style fixture
# ---------------------------------------------------------------------------
SAME1 = dict(strides=[1, 1, 1, 1], padding='SAME')
POOL3 = dict(ksize=[1, 3, 3, 1], strides=[1, 1, 1, 1], padding='SAME')
HEAD = dict(ksize=[1, 16, 16, 1], strides=[1, 1, 1, 1], padding='VALID')
X_SHAPE = (2, 16, 16, 8)
# x is scaled so that the stem's pre-activations pass 6
X_SCALE = 6.0
STATIC = 'quantize_nodes(fallback_min=-16, fallback_max=16)'
FALLBACK = (-16.0, 16.0)


def fixture_values(seed):
    rng = np.random.RandomState(seed)
    v = {}
    v['x'] = X_SCALE * rng.uniform(-1, 1, X_SHAPE)
    v['w1'] = rng.randn(3, 3, 8, 16) / np.sqrt(72)
    v['b1'] = 0.1 * rng.randn(16)
    v['wa'] = rng.randn(1, 1, 16, 16) / 4
    v['ba'] = 0.1 * rng.randn(16)
    v['wb'] = rng.randn(1, 1, 16, 32) / 4
    v['bb'] = 0.1 * rng.randn(32)
    v['w3'] = rng.randn(64, 10) / 8
    v['b3'] = 0.1 * rng.randn(10)
    return v


def fresh_input(seed):
    return X_SCALE * np.random.RandomState(seed).uniform(-1.2, 1.2, X_SHAPE)


def fixture_graph_def(v):
    """The frozen float graph: placeholder 'x' to BiasAdd 'logits'."""
    def const(name):
        return tf.constant(v[name].astype(F32), name=name)

    def conv(h, w, b, name):
        h = tf.nn.conv2d(h, const(w), name='conv_' + name, **SAME1)
        return tf.nn.bias_add(h, const(b), name='bias_' + name)

    with tf.Graph().as_default() as g:
        x = tf.placeholder(tf.float32, X_SHAPE, name='x')
        stem = tf.nn.relu6(conv(x, 'w1', 'b1', 'stem'), name='stem')
        a = tf.nn.relu(conv(stem, 'wa', 'ba', 'a'), name='a')
        b = tf.nn.avg_pool(stem, name='pool_b', **POOL3)
        b = tf.nn.relu(conv(b, 'wb', 'bb', 'b'), name='b')
        c = tf.nn.max_pool(stem, name='c', **POOL3)
        h = tf.concat([a, b, c], 3, name='mixed')
        h = tf.nn.avg_pool(h, name='head', **HEAD)
        h = tf.reshape(h, [2, 64], name='flat')
        h = tf.matmul(h, const('w3'), name='fc')
        tf.nn.bias_add(h, const('b3'), name='logits')
        return g.as_graph_def()


def float64_forward(v, x=None, parts=False):
    x = v['x'] if x is None else x

    def conv(t, w, b):
        r = w.shape[0]
        return np.einsum('npqrsc,rsck->npqk',
                         _windows(t, r, r, 1, 1, 'SAME', 0.0), w) + b

    def avg(t, p):
        win = _windows(t, p['ksize'][1], p['ksize'][2], 1, 1, p['padding'],
                       np.nan)
        return np.nanmean(win, axis=(3, 4))

    pre = conv(x, v['w1'], v['b1'])
    stem = np.minimum(np.maximum(pre, 0), 6)
    a = np.maximum(conv(stem, v['wa'], v['ba']), 0)
    b = np.maximum(conv(avg(stem, POOL3), v['wb'], v['bb']), 0)
    c = _windows(stem, 3, 3, 1, 1, 'SAME', -np.inf).max(axis=(3, 4))
    h = avg(np.concatenate([a, b, c], 3), HEAD)
    logits = h.reshape(2, 64) @ v['w3'] + v['b3']
    return (logits, pre) if parts else logits


def emulate(v, x=None, fallback=None):
    """The quantize_nodes pipeline in numpy, from the formulas alone."""
    x = np.asarray(v['x'] if x is None else x, F32)

    def down(t):
        p, mn, mx = t
        lo, hi = fallback or np_requantization_range(p, mn, mx)
        return np_requantize(p, mn, mx, lo, hi)

    def layer(t, w, b, conv=True):
        wq, wmn, wmx = np_quantize_const(v[w].astype(F32))
        if conv:
            t = down(np_conv2d(t[0], wq, t[1], t[2], wmn, wmx,
                               SAME1['strides'], SAME1['padding']))
        else:
            t = down(np_matmul(t[0], wq, t[1], t[2], wmn, wmx))
        bq, bmn, bmx = np_quantize_const(v[b].astype(F32))
        return down(np_bias_add(t[0], bq, t[1], t[2], bmn, bmx))

    def on_bytes(fn, t, *args):
        return fn(t[0], *args), t[1], t[2]

    def relu(t):
        return np_relu(*t), t[1], t[2]

    def pool(fn, t, p):
        return on_bytes(fn, t, p['ksize'], p['strides'], p['padding'])

    t = np_quantize_v2(x, x.min(), x.max())
    t = layer(t, 'w1', 'b1')
    stem = np_relu6(*t), t[1], t[2]
    a = relu(layer(stem, 'wa', 'ba'))
    b = relu(layer(pool(np_avg_pool, stem, POOL3), 'wb', 'bb'))
    c = pool(np_max_pool, stem, POOL3)
    branches = (a, b, c)
    t = np_concat(3, [br[0] for br in branches], [br[1] for br in branches],
                  [br[2] for br in branches])
    t = pool(np_avg_pool, t, HEAD)
    t = t[0].reshape(2, 64), t[1], t[2]
    return np_dequantize_u8(*layer(t, 'w3', 'b3', conv=False))


def quantize_fixture(gd, spec='quantize_nodes'):
    return transform_graph.transform_graph(gd, ['x'], ['logits'], [spec])


@pytest.fixture(scope='module')
def seed0():
    v = fixture_values(0)
    gd = fixture_graph_def(v)
    return v, gd, quantize_fixture(gd), quantize_fixture(gd, STATIC)


# quantized op -> nodes of it in the transformed fixture
FIXTURE_CENSUS = {
    'QuantizedConv2D': 3, 'QuantizedMatMul': 1, 'QuantizedBiasAdd': 4,
    'QuantizedRelu': 2, 'QuantizedRelu6': 1, 'QuantizedMaxPool': 1,
    'QuantizedAvgPool': 2, 'QuantizedConcat': 1, 'QuantizedReshape': 1,
    'Requantize': 8,
}
FLOAT_OPS = ('AvgPool', 'Relu6', 'ConcatV2', 'Relu', 'MaxPool', 'Conv2D',
             'MatMul', 'BiasAdd')


@pytest.mark.parametrize('mode', ['dynamic', 'static'])
def test_inception_block_op_census(seed0, mode):
    _, gd, qgd, sgd = seed0
    before = op_census(gd)
    after = op_census(qgd if mode == 'dynamic' else sgd)
    for op in FLOAT_OPS:
        assert op in before and op not in after, op
    assert after['QuantizeV2'] == ['conv_stem/in0/quantize']
    assert after['Dequantize'] == ['logits']
    assert after['Placeholder'] == ['x']
    # the one float Reshape left is the input's quantize group's own
    assert after['Reshape'] == ['conv_stem/in0/reshape']
    for op, count in FIXTURE_CENSUS.items():
        assert len(after[op]) == count, op
    if mode == 'dynamic':
        assert len(after['RequantizationRange']) == 8
        assert len(after['Min']) == 1 and len(after['Max']) == 1
    else:
        assert 'RequantizationRange' not in after
        assert after['Min'] == ['conv_stem/in0/min']
        assert after['Max'] == ['conv_stem/in0/max']
    nodes = {n['name']: n for n in pbreader.parse_graph_def(qgd)}
    # the stem is read as one uint8 triple by all three branches
    stem = ['stem/eightbit:0', 'stem/eightbit:1', 'stem/eightbit:2']
    assert nodes['conv_a/eightbit']['input'] == [
        stem[0], 'wa/quint8_const', stem[1], stem[2], 'wa/min', 'wa/max']
    assert nodes['pool_b/eightbit']['input'] == stem
    assert nodes['c/eightbit']['input'] == stem
    # the axis first, then tensors, all mins, all maxes
    (mixed,) = [n for n in pbreader.parse_graph_def(gd)
                if n['name'] == 'mixed']
    assert mixed['input'][:3] == ['a', 'b', 'c']
    assert nodes['mixed/eightbit']['input'] == [
        mixed['input'][3],
        'a/eightbit:0', 'b/eightbit:0', 'c/eightbit:0',
        'a/eightbit:1', 'b/eightbit:1', 'c/eightbit:1',
        'a/eightbit:2', 'b/eightbit:2', 'c/eightbit:2']
    assert nodes['mixed/eightbit']['attr']['N'][1] == 3
    assert nodes['mixed/eightbit']['attr']['T'][1] == int(tf.uint8)


def test_float_fixture_matches_float64(seed0):
    """The float64 reference is the network the fixture graph computes, and
    the fixture does exercise Relu6's ceiling."""
    v, gd, _, _ = seed0
    ref, pre = float64_forward(v, parts=True)
    assert (pre > 6).mean() > 0.01 and (pre < 0).mean() > 0.1
    got = run_graph(gd, v['x'])
    # f32 against f64 over reductions of at most 256 terms
    assert rel_l2(got.astype(np.float64), ref) < 1e-5


@pytest.mark.parametrize('seed', [0, 11, 12, 13])
def test_inception_block_matches_the_emulation(seed, seed0):
    v, _, qgd, sgd = seed0
    x = v['x'] if seed == 0 else fresh_input(seed)
    want = emulate(v, x=x)
    got = run_graph(qgd, x)
    assert got.dtype == F32 and got.shape == (2, 10)
    assert np.array_equal(got, want)
    assert np.array_equal(run_graph(sgd, x),
                          emulate(v, x=x, fallback=FALLBACK))


def test_inception_block_accuracy(seed0):
    """Relative L2 error of the numpy emulation of the 8-bit pipeline against
    the float64 forward pass. Measured for seed 0 from the emulation alone:
    0.0241. The bound is twice that, 0.0481, rounded up to one significant
    digit."""
    v = seed0[0]
    ref = float64_forward(v)
    err = rel_l2(emulate(v).astype(np.float64), ref)
    print('seed 0: relative L2 error %.4f' % err)
    assert err <= 0.05


def test_inception_block_through_transform_graph(seed0):
    v, gd, qgd, _ = seed0
    again = transform_graph.transform_graph(gd, ['x'], ['logits'],
                                            ['quantize_nodes'])
    assert again == qgd
    direct = quantize_graph_lib.quantize_nodes(gd, ['x'], ['logits'])
    assert np.array_equal(run_graph(direct, v['x']), emulate(v))


def test_legacy_concat_is_rewritten():
    """Concat has the axis first; its values are inputs 1..N."""
    x = tf.placeholder(tf.float32, (2, 3), name='x')
    a = tf.nn.relu(x, name='a')
    b = tf.nn.relu6(x, name='b')
    apply_op('Concat', tf.constant(1, name='dim'), [a, b], name='cat')
    gd = tf.get_default_graph().as_graph_def()
    out = transform_graph.transform_graph(gd, ['x'], ['cat'],
                                          ['quantize_nodes'])
    census = op_census(out)
    assert 'Concat' not in census and census['QuantizedConcat'] == \
        ['cat/eightbit']
    assert census['Dequantize'] == ['cat']
    nodes = {n['name']: n for n in pbreader.parse_graph_def(out)}
    assert nodes['cat/eightbit']['input'] == [
        'dim', 'a/eightbit:0', 'b/eightbit:0', 'a/eightbit:1',
        'b/eightbit:1', 'a/eightbit:2', 'b/eightbit:2']
    xv = np.array([[-1.0, 0.5, 7.0], [2.0, 6.5, -3.0]], F32)
    got = run_graph(out, xv, fetch='cat:0')
    want = np.concatenate([np.maximum(xv, 0), np.clip(xv, 0, 6)], 1)
    # x is quantized over (-3, 7): half a step there, and up to half a step
    # where the floor or the ceiling of a clamp is rounded to the grid; both
    # inputs have the output range, so the concat copies them
    np.testing.assert_allclose(got, want, atol=1.01 * 10.0 / 255)


def test_quantize_nodes_leaves_what_it_cannot_express():
    """A ConcatV2 with an int64 axis, a concat that is not float32, a node
    with a control input and a pool that is not NHWC stay as they are."""
    x = tf.placeholder(tf.float32, (1, 4, 4, 2), name='x')
    i = tf.placeholder(tf.int32, (3,), name='i')
    c64 = apply_op('ConcatV2', [x, x], tf.constant(3, dtype=tf.int64),
                   name='c64')
    tf.concat([i, i], 0, name='ci')
    with tf.control_dependencies([c64.op]):
        tf.nn.relu6(x, name='ctl')
    tf.nn.avg_pool(x, [1, 1, 2, 2], [1, 1, 1, 1], 'VALID',
                   data_format='NCHW', name='nchw')
    outputs = ['c64', 'ci', 'ctl', 'nchw']
    gd = tf.get_default_graph().as_graph_def()
    out = transform_graph.transform_graph(gd, ['x', 'i'], outputs,
                                          ['quantize_nodes'])
    before, after = op_census(gd), op_census(out)
    assert after == before
    assert not any(op.startswith(('Quantize', 'Dequantize'))
                   for op in after)
    assert sorted(after['ConcatV2']) == ['c64', 'ci']
    assert after['Relu6'] == ['ctl'] and after['AvgPool'] == ['nchw']
    xv = np.random.RandomState(3).uniform(-8, 8, (1, 4, 4, 2)).astype(F32)
    iv = np.array([1, 2, 3], np.int32)
    results = []
    for g in (gd, out):
        tf.reset_default_graph()
        fetched = tf.import_graph_def(
            pin(g, '/cpu:0'), return_elements=[o + ':0' for o in outputs],
            name='')
        graph = tf.get_default_graph()
        with tf.Session() as s:
            results.append(s.run(fetched, {
                graph.get_tensor_by_name('x:0'): xv,
                graph.get_tensor_by_name('i:0'): iv}))
    for a, b in zip(*results):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(results[1][0], np.concatenate([xv, xv], 3))
    assert np.array_equal(results[1][2], np.clip(xv, 0, 6))
