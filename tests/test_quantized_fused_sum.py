"""QuantizedConv2DWithBiasSumAndRequantize on the CPU against numpy (int64
accumulation, then stf::QuantFusedSumU8 one f32 operation at a time), and
quantize_nodes' fuse_sum on ResNet blocks. All comparisons are array_equal."""
import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.ops import quantized_ops as q
from simple_tensorflow_amd.python.tools import quantize_graph_lib as qlib
from simple_tensorflow_amd.python.tools import transform_graph

from test_quantized_conv import _step
from test_quantized_fused import (ACTIVATIONS, F32, fused_reference,
                                  fused_value, operands, shape_id)
from test_quantized_inference import op_census, run_graph

# (image, filter, stride, padding): the smallest shapes that reach each path
# of GemmI8FusedSum. A 1x9x15 image is M = 135: a row tail in a second block.
CASES = [
    ((1, 9, 15, 16), (1, 1, 16, 64), 1, 'VALID'),    # WN = 2
    ((2, 9, 15, 16), (1, 1, 16, 128), 1, 'VALID'),   # WN = 4, M = 270
    ((1, 9, 15, 16), (1, 1, 16, 48), 1, 'VALID'),    # a chunk column absent
    ((1, 9, 15, 16), (1, 1, 16, 144), 1, 'VALID'),   # 16 channels in block 2
    ((1, 9, 15, 16), (1, 1, 16, 24), 1, 'VALID'),    # byte path, WN = 2
    ((1, 9, 15, 16), (1, 1, 16, 72), 1, 'VALID'),    # byte path, WN = 4
    ((1, 3, 5, 16), (3, 3, 16, 64), 1, 'SAME'),      # every pixel a border
    ((1, 9, 15, 8), (1, 1, 8, 64), 2, 'VALID'),      # projection, im2col
    ((1, 9, 15, 16), (1, 1, 16, 128), 2, 'VALID'),   # projection, implicit
    ((0, 9, 15, 16), (1, 1, 16, 64), 1, 'VALID'),    # empty output
]
# fill -> (summand range, constant summand); the requested range is (-3, 5),
# (2, 2) for 'degenerate'
FILLS = {'random': ((-1.5, 4.5), None), 'all0': ((-1.5, 4.5), 0),
         'all255': ((-1.5, 4.5), 255), 'nozero': ((1.0, 3.0), None),
         'wide': ((-24.0, 40.0), None), 'degenerate': ((-1.5, 4.5), None)}
# (shape, activation, fill, seed); the extremes at one shape per tile width
PARAMS = [(s, a, 'random', i) for i, s in enumerate(CASES)
          for a in ACTIVATIONS] + \
    [(s, 'None', f, 3) for s in CASES[:2] for f in list(FILLS)[1:]]


def param_id(p):
    return '%s-%s-%s' % (shape_id(p[0]), p[1], p[2])


def sum_reference(acc_value, summand, s_range, activation, req):
    v = acc_value + (F32(s_range[0]) + summand.astype(F32) * _step(*s_range))
    if activation != 'None':
        v = np.where(F32(0) < v, v, F32(0))
    if activation == 'Relu6':
        v = np.where(v < F32(6), v, F32(6))
    return fused_reference(v, req)


def check_sum_case(sess, device, shape, activation, fill, seed):
    s_range, const = FILLS[fill]
    x, w, bias, rx, rw, req = operands(
        shape, 'degenerate' if fill == 'degenerate' else 'random', seed)
    strides = [1, shape[2], shape[2], 1]
    v = fused_value(x, w, bias, rx, rw, 'None', strides, shape[3])
    summand = (np.random.RandomState(seed + 100).randint(0, 256, v.shape)
               if const is None else np.full(v.shape, const)).astype(np.uint8)
    want = sum_reference(v, summand, s_range, activation, req)
    values = (x, w, bias, summand)
    with tf.device(device):
        phs = [tf.placeholder(tf.float32 if a is bias else tf.uint8, a.shape)
               for a in values]
        outs = list(q.quantized_conv2d_with_bias_sum_and_requantize(
            *phs, rx[0], rx[1], rw[0], rw[1], s_range[0], s_range[1], req[0],
            req[1], strides, shape[3], activation=activation))
    feeds = dict(zip(phs, values))
    for g, e in zip(sess.run(outs, feeds), want):
        assert g.dtype == e.dtype and g.shape == np.shape(e)
        assert np.array_equal(g, e), (np.flatnonzero(g != e)[:4], g, e)
    if fill == 'wide' and activation == 'None':  # both ends saturate
        assert (want[0] == 0).any() and (want[0] == 255).any()
    return outs, feeds, want


@pytest.mark.parametrize('param', PARAMS, ids=param_id)
def test_cpu_kernel(param):
    tf.reset_default_graph()
    with tf.Session() as s:
        check_sum_case(s, '/cpu:0', *param)


def test_summand_shape_mismatch():
    tf.reset_default_graph()
    zeros = [np.zeros(s, np.uint8) for s in
             ((1, 4, 4, 16), (1, 1, 16, 8), (1, 1, 1, 8))]  # would broadcast
    ps = [tf.placeholder(tf.uint8, z.shape) for z in zeros]
    with tf.device('/cpu:0'):
        out = q.quantized_conv2d_with_bias_sum_and_requantize(
            ps[0], ps[1], np.zeros(8, F32), ps[2], 0.0, 1.0, 0.0, 1.0, 0.0,
            2.0, 0.0, 1.0, [1, 1, 1, 1], 'VALID')[0]
    with tf.Session() as s:
        with pytest.raises(tf.errors.InvalidArgumentError, match='summand'):
            s.run(out, dict(zip(ps, zeros)))


# fuse_sum: a stem conv and one bottleneck block with folded batch norms,
# x -> c0 -> [c1 -> c2 -> c3] + shortcut -> Relu 'logits'.
FALLBACK = (-8.0, 7.9375)  # holds 0.0 exactly
# name -> (filter, stride, activation). The strides and 'proj' are the
# projection block's; the identity block has stride 1 and the shortcut second.
LAYERS = {'c0': ((3, 3, 16, 16), 1, 'Relu'), 'c1': ((1, 1, 16, 8), 2, 'Relu'),
          'c2': ((3, 3, 8, 8), 1, 'Relu'), 'c3': ((1, 1, 8, 16), 1, 'Relu'),
          'proj': ((1, 1, 16, 16), 2, 'None')}


def block_graph(weights, projection):
    def conv(h, k, relu=True):
        stride = LAYERS[k][1] if projection else 1
        h = tf.nn.conv2d(h, tf.constant(weights[k][0], name=k + '/w'),
                         [1, stride, stride, 1], 'SAME', name=k)
        h = tf.nn.bias_add(h, tf.constant(weights[k][1], name=k + '/b'),
                           name=k + '/a')
        return tf.nn.relu(h, name=k + '/r') if relu else h

    with tf.Graph().as_default() as g:
        r0 = conv(tf.placeholder(tf.float32, (2, 6, 6, 16), name='x'), 'c0')
        main = conv(conv(conv(r0, 'c1'), 'c2'), 'c3', relu=False)
        s = tf.add(conv(r0, 'proj', relu=False), main, name='sum') \
            if projection else tf.add(main, r0, name='sum')
        tf.nn.relu(s, name='logits')
        return g.as_graph_def()


def block_reference(weights, projection, xv):
    """x under its own min/max, nudged weight ranges, the rest in FALLBACK."""
    def layer(h, hr, k, summand=None):
        w, b = weights[k]
        wr = qlib.nudged_range(w.min(), w.max())
        stride, act = LAYERS[k][1] if projection else 1, LAYERS[k][2]
        v = fused_value(h, qlib.quantize_array(w, *wr), b, hr, wr,
                        act if summand is None else 'None',
                        [1, stride, stride, 1], 'SAME')
        if summand is None:
            return fused_reference(v, FALLBACK)[0]
        return sum_reference(v, summand, FALLBACK, act, FALLBACK)[0]

    xr = (xv.min(), xv.max())
    r0 = layer(qlib.quantize_array(xv, *xr), xr, 'c0')
    main = layer(layer(r0, FALLBACK, 'c1'), FALLBACK, 'c2')
    out = layer(main, FALLBACK, 'c3',
                layer(r0, FALLBACK, 'proj') if projection else r0)
    return F32(FALLBACK[0]) + out.astype(F32) * _step(*FALLBACK)


@pytest.mark.parametrize('projection', [False, True],
                         ids=['identity', 'projection'])
def test_fuse_sum_bottleneck(projection):
    rng = np.random.RandomState(7)
    weights = {k: ((rng.randn(*f) / np.sqrt(np.prod(f[:3]))).astype(F32),
                   (.1 * rng.randn(f[3])).astype(F32))
               for k, (f, _, _) in LAYERS.items()}
    gd = block_graph(weights, projection)
    args = (gd, ['x'], ['logits'], FALLBACK[0], FALLBACK[1])
    with pytest.raises(ValueError):
        qlib.quantize_nodes(*args, fuse_sum=True)
    fused = qlib.quantize_nodes(*args, fuse_epilogue=True, fuse_sum=True)
    census = op_census(fused)
    sum_op = 'QuantizedConv2DWithBiasSumAndRequantize'
    fused_op = 'QuantizedConv2DWithBiasAndRequantize'
    assert census[sum_op] == ['logits/eightbit']
    assert len(census[fused_op]) == 3 + projection
    # quint8 from the one QuantizeV2 behind x to the one Dequantize
    assert (census['QuantizeV2'], census['Dequantize']) == \
        (['c0/in0/quantize'], ['logits'])
    assert not {'Add', 'Relu', 'BiasAdd', 'Conv2D'} & set(census)
    assert transform_graph.transform_graph(
        gd, ['x'], ['logits'],
        ['quantize_nodes(fallback_min=-8, fallback_max=7.9375, '
         'fuse_epilogue=true, fuse_sum=true)']) == fused
    # without fuse_sum: the graph of fuse_epilogue alone, with a float Add
    plain = qlib.quantize_nodes(*args, fuse_epilogue=True, fuse_sum=False)
    assert plain == qlib.quantize_nodes(*args, fuse_epilogue=True)
    census = op_census(plain)
    assert sum_op not in census and census['Add'] == ['sum']
    assert census['QuantizedRelu'] == ['logits/eightbit']
    assert len(census[fused_op]) == 4 + projection
    xv = np.random.RandomState(1).uniform(-1, 1, (2, 6, 6, 16)).astype(F32)
    assert np.array_equal(run_graph(fused, xv),
                          block_reference(weights, projection, xv))
