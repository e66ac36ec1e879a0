"""Requantize, QuantizedBiasAdd, QuantizedMaxPool and QuantizedReshape on the
GPU (csrc/kernels/hip/quantized.hip through csrc/kernels/gpu_quantized.cc)
against the CPU kernels, and the quantize_nodes graph end to end on the GPU.

As in test_gpu_quantized.py each case builds the op twice in one graph,
under /cpu:0 and under /gpu:0, feeds both the same placeholders and requires
np.array_equal on every output, the range scalars included. The ranges come
through placeholders as well, so nothing is folded into a constant. The CPU
kernels themselves are pinned against numpy in test_quantized_inference.py,
whose shapes and data this file reuses. All tests need a gfx950 GPU.
"""
import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.ops import quantized_ops as q

from test_gpu_kernels import _sess
from test_gpu_quantized import _check_equal, _trace_run
from test_quantized_inference import (BIAS_CHANNELS, POOL_CASES,
                                      POOL_CHANNELS, RANGES,
                                      REQUANTIZE_CASES, REQUANTIZE_SIZES,
                                      STATIC, bias_add_ranges,
                                      bias_add_shapes, fixture_graph_def,
                                      fixture_values, int32_data, pin,
                                      quantize_fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def sess():
    """One graph and one session for the module; every test only adds
    nodes."""
    tf.reset_default_graph()
    with _sess() as s:
        yield s


def _scalars(n):
    return [tf.placeholder(tf.float32, ()) for _ in range(n)]


def _feed(placeholders, values):
    return {p: np.float32(v) for p, v in zip(placeholders, values)}


# 65536 + 3: many blocks of 16-element groups, and a scalar tail
@pytest.mark.parametrize('n', REQUANTIZE_SIZES + (65536 + 3,))
def test_requantize(sess, n):
    x = int32_data(n, n)
    pi = tf.placeholder(tf.int32, (n,))
    r = _scalars(4)
    with tf.device('/cpu:0'):
        cpu = list(q.requantize(pi, *r))
    with tf.device('/gpu:0'):
        gpu = list(q.requantize(pi, *r))
    for (mn, mx), requested in REQUANTIZE_CASES:
        for lo, hi in requested:
            feeds = _feed(r, (mn, mx, lo, hi))
            feeds[pi] = x
            outs = sess.run(cpu + gpu, feeds)
            for i in range(3):
                assert outs[i].dtype == outs[3 + i].dtype
                assert np.array_equal(outs[i], outs[3 + i]), \
                    (i, (mn, mx), (lo, hi))
            assert outs[3].dtype == np.uint8 and outs[3].shape == (n,)


@pytest.mark.parametrize('c', BIAS_CHANNELS)
def test_quantized_bias_add(sess, c):
    rng = np.random.RandomState(c)
    idx = 0
    # (0, c): an empty tensor still gets its ranges
    for shape in bias_add_shapes(c) + [(0, c)]:
        x = rng.randint(0, 256, shape).astype(np.uint8)
        b = rng.randint(0, 256, (c,)).astype(np.uint8)
        x.reshape(-1)[:2] = [0, 255][:x.size]
        px = tf.placeholder(tf.uint8, shape)
        pb = tf.placeholder(tf.uint8, (c,))
        r = _scalars(4)
        with tf.device('/cpu:0'):
            cpu = list(q.quantized_bias_add(px, pb, *r))
        with tf.device('/gpu:0'):
            gpu = list(q.quantized_bias_add(px, pb, *r))
        for _ in range(5):
            rx, rb = bias_add_ranges(idx)
            idx += 1
            feeds = _feed(r, rx + rb)
            feeds.update({px: x, pb: b})
            outs = sess.run(cpu + gpu, feeds)
            for i in range(3):
                assert outs[i].dtype == outs[3 + i].dtype
                assert outs[i].shape == outs[3 + i].shape
                assert np.array_equal(outs[i], outs[3 + i]), \
                    (i, shape, rx, rb)
            assert outs[3].dtype == np.int32 and outs[3].shape == shape


@pytest.mark.parametrize('c', POOL_CHANNELS)
@pytest.mark.parametrize('case', POOL_CASES,
                         ids=['%dx%d_k%d_s%d_%s' % (p[0], p[0], p[1], p[2],
                                                    p[3]) for p in POOL_CASES])
def test_quantized_max_pool(sess, case, c):
    hw, k, stride, padding = case
    x = np.random.RandomState(c + hw).randint(0, 256, (2, hw, hw, c)) \
        .astype(np.uint8)
    px = tf.placeholder(tf.uint8, x.shape)
    r = _scalars(2)
    feeds = _feed(r, RANGES[c % 4])
    feeds[px] = x
    outs = _check_equal(
        sess, lambda: q.quantized_max_pool(px, r[0], r[1], [1, k, k, 1],
                                           [1, stride, stride, 1], padding),
        feeds, 'QuantizedMaxPool')
    assert outs[0].dtype == np.uint8
    assert (outs[1], outs[2]) == tuple(np.float32(RANGES[c % 4]))


@pytest.mark.parametrize('dtype', [np.uint8, np.int32])
def test_quantized_reshape(sess, dtype):
    x = np.arange(24).reshape(2, 3, 4).astype(dtype)
    px = tf.placeholder(tf.as_dtype(dtype), x.shape)
    r = _scalars(2)
    feeds = _feed(r, (-1.5, 2.5))
    feeds[px] = x
    outs = _check_equal(
        sess, lambda: q.quantized_reshape(px, [4, -1], r[0], r[1]), feeds,
        'QuantizedReshape')
    assert np.array_equal(outs[0], x.reshape(4, 6))


# ---------------------------------------------------------------------------
# the transformed fixture network, on both devices
# ---------------------------------------------------------------------------
QUANTIZED_OPS = ('Quantized', 'Requantize', 'RequantizationRange',
                 'QuantizeV2', 'Dequantize')


@pytest.mark.parametrize('spec', ['quantize_nodes', STATIC],
                         ids=['dynamic', 'static'])
def test_quantized_network_runs_on_the_gpu(sess, spec):
    v = fixture_values(0)
    gd = fixture_graph_def(v)
    qgd = quantize_fixture(gd, spec)
    tag = 'static' if spec == STATIC else 'dynamic'
    # import_graph_def does not apply the device scope: the device goes on
    # the nodes. int32 Consts are shapes and axes, which GPU kernels take in
    # host memory.
    cpu_nodes = pin(qgd, '/cpu:0')
    gpu_nodes = pin(qgd, '/gpu:0', skip_host_consts=True)
    px = tf.placeholder(tf.float32, (2, 16, 16, 8))
    (cpu,) = tf.import_graph_def(cpu_nodes, input_map={'x:0': px},
                                 return_elements=['logits:0'],
                                 name='qnet_cpu_' + tag)
    (gpu,) = tf.import_graph_def(gpu_nodes, input_map={'x:0': px},
                                 return_elements=['logits:0'],
                                 name='qnet_gpu_' + tag)
    prefix = gpu.op.name[:-len('logits')]
    quantized = [prefix + n['name'] for n in gpu_nodes
                 if n['op'].startswith(QUANTIZED_OPS)]
    assert len(quantized) == (19 if spec == STATIC else 25)
    rng = np.random.RandomState(5)

    outs, on_gpu = _trace_run(sess, [cpu, gpu],
                              {px: v['x'].astype(np.float32)})
    assert np.array_equal(outs[0], outs[1])
    for name in quantized:
        assert name in on_gpu, (name, sorted(on_gpu))
    assert not any(n.startswith(cpu.op.name[:-len('logits')])
                   for n in on_gpu)
    # the same graph again and again with fresh inputs
    results = []
    for _ in range(5):
        x = rng.uniform(-1.5, 1.5, (2, 16, 16, 8)).astype(np.float32)
        outs = sess.run([cpu, gpu], {px: x})
        assert np.array_equal(outs[0], outs[1])
        results.append(outs[1])
    assert all(not np.array_equal(results[0], r) for r in results[1:])
