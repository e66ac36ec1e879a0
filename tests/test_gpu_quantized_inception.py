"""QuantizedAvgPool, QuantizedRelu6 and QuantizedConcat on the GPU
(csrc/kernels/hip/quantized.hip through csrc/kernels/gpu_quantized.cc)
against the CPU kernels, and the quantized Inception-style block end to end
on the GPU.

As in test_gpu_quantized_inference.py each case builds the op twice in one
graph, under /cpu:0 and under /gpu:0, feeds both the same placeholders, the
ranges included, and requires np.array_equal on every output. The CPU
kernels themselves are pinned against numpy in test_quantized_inception.py,
whose shapes and data this file reuses. All tests need a gfx950 GPU.
"""
import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.ops import quantized_ops as q

from test_gpu_kernels import _sess
from test_gpu_quantized import _check_equal, _trace_run
from test_quantized_inference import POOL_CASES, POOL_CHANNELS, RANGES, pin
from test_quantized_inception import (CONCAT_CASES, POOL_IDS, RELU6_RANGES,
                                      RELU6_SIZES, SATURATED_CASES, STATIC,
                                      X_SHAPE, avg_pool_input, concat_inputs,
                                      concat_range_sets, fixture_graph_def,
                                      fixture_values, fresh_input,
                                      quantize_fixture, relu6_input)

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


def _avg_pool_equal(sess, x, k, stride, padding, rng):
    px = tf.placeholder(tf.uint8, x.shape)
    r = _scalars(2)
    feeds = _feed(r, rng)
    feeds[px] = x
    outs = _check_equal(
        sess, lambda: q.quantized_avg_pool(px, r[0], r[1], [1, k, k, 1],
                                           [1, stride, stride, 1], padding),
        feeds, 'QuantizedAvgPool')
    assert outs[0].dtype == np.uint8
    assert (outs[1], outs[2]) == tuple(np.float32(rng))
    return outs[0]


@pytest.mark.parametrize('c', POOL_CHANNELS)
@pytest.mark.parametrize('case', POOL_CASES, ids=POOL_IDS)
def test_quantized_avg_pool(sess, case, c):
    _, k, stride, padding = case
    _avg_pool_equal(sess, avg_pool_input(case, c), k, stride, padding,
                    RANGES[c % 4])


def test_quantized_avg_pool_many_blocks(sess):
    # 64 * 4 * 4 * 48 / 16 = 3072 threads of 16 channels: 12 blocks
    x = np.random.RandomState(7).randint(0, 256, (64, 7, 7, 48)) \
        .astype(np.uint8)
    out = _avg_pool_equal(sess, x, 3, 2, 'SAME', (0.0, 6.0))
    assert out.shape == (64, 4, 4, 48)


@pytest.mark.parametrize('case', SATURATED_CASES,
                         ids=['%dx%d_k%d_%s_c%d' % (p[0], p[0], p[1], p[3],
                                                   p[4])
                              for p in SATURATED_CASES])
def test_quantized_avg_pool_of_255_is_255(sess, case):
    hw, k, stride, padding, c = case
    x = np.full((2, hw, hw, c), 255, np.uint8)
    out = _avg_pool_equal(sess, x, k, stride, padding, (0.0, 6.0))
    assert np.all(out == 255)


# 65536 + 3: many blocks of 16-byte groups, and a scalar tail
@pytest.mark.parametrize('n', RELU6_SIZES + (65536 + 3,))
def test_quantized_relu6(sess, n):
    x = relu6_input(n)
    px = tf.placeholder(tf.uint8, (n,))
    r = _scalars(2)
    with tf.device('/cpu:0'):
        cpu = list(q.quantized_relu6(px, *r))
    with tf.device('/gpu:0'):
        gpu = list(q.quantized_relu6(px, *r))
    for rng in RELU6_RANGES:
        feeds = _feed(r, rng)
        feeds[px] = x
        outs = sess.run(cpu + gpu, feeds)
        for i in range(3):
            assert outs[i].dtype == outs[3 + i].dtype
            assert outs[i].shape == outs[3 + i].shape
            assert np.array_equal(outs[i], outs[3 + i]), (i, rng)
        assert outs[3].dtype == np.uint8 and outs[3].shape == (n,)


# vec_*: every width is a multiple of 16, the 16-byte path; bytes_*: the
# byte path; n17: more inputs than one argument table holds
@pytest.mark.parametrize('name', sorted(CONCAT_CASES))
def test_quantized_concat(sess, name):
    axis, xs = concat_inputs(name)
    n = len(xs)
    ps = [tf.placeholder(tf.uint8, x.shape) for x in xs]
    mins, maxes = _scalars(n), _scalars(n)
    with tf.device('/cpu:0'):
        cpu = list(q.quantized_concat(axis, ps, mins, maxes))
    with tf.device('/gpu:0'):
        gpu = list(q.quantized_concat(axis, ps, mins, maxes))
    want_shape = np.concatenate(xs, axis).shape
    for set_name, ranges in concat_range_sets(n).items():
        feeds = _feed(mins, [r[0] for r in ranges])
        feeds.update(_feed(maxes, [r[1] for r in ranges]))
        feeds.update(zip(ps, xs))
        outs = sess.run(cpu + gpu, feeds)
        for i in range(3):
            assert outs[i].dtype == outs[3 + i].dtype
            assert outs[i].shape == outs[3 + i].shape
            assert np.array_equal(outs[i], outs[3 + i]), (i, name, set_name)
        assert outs[3].dtype == np.uint8 and outs[3].shape == want_shape


# ---------------------------------------------------------------------------
# the transformed Inception-style fixture, on both devices
# ---------------------------------------------------------------------------
QUANTIZED_OPS = ('Quantized', 'Requantize', 'RequantizationRange',
                 'QuantizeV2', 'Dequantize')
NEW_OPS = ('QuantizedAvgPool', 'QuantizedRelu6', 'QuantizedConcat')


@pytest.mark.parametrize('spec', ['quantize_nodes', STATIC],
                         ids=['dynamic', 'static'])
def test_quantized_inception_block_runs_on_the_gpu(sess, spec):
    v = fixture_values(0)
    qgd = quantize_fixture(fixture_graph_def(v), spec)
    tag = 'static' if spec == STATIC else 'dynamic'
    # int32 Consts are shapes and axes, which GPU kernels take in host memory
    cpu_nodes = pin(qgd, '/cpu:0')
    gpu_nodes = pin(qgd, '/gpu:0', skip_host_consts=True)
    px = tf.placeholder(tf.float32, X_SHAPE)
    (cpu,) = tf.import_graph_def(cpu_nodes, input_map={'x:0': px},
                                 return_elements=['logits:0'],
                                 name='qmix_cpu_' + tag)
    (gpu,) = tf.import_graph_def(gpu_nodes, input_map={'x:0': px},
                                 return_elements=['logits:0'],
                                 name='qmix_gpu_' + tag)
    prefix = gpu.op.name[:-len('logits')]
    quantized = [prefix + n['name'] for n in gpu_nodes
                 if n['op'].startswith(QUANTIZED_OPS)]
    # 16 Quantized*, 8 Requantize, QuantizeV2, Dequantize; 8
    # RequantizationRange in dynamic mode
    assert len(quantized) == (26 if spec == STATIC else 34)
    assert sum(n['op'] in NEW_OPS for n in gpu_nodes) == 4

    outs, on_gpu = _trace_run(sess, [cpu, gpu],
                              {px: v['x'].astype(np.float32)})
    assert np.array_equal(outs[0], outs[1])
    for name in quantized:
        assert name in on_gpu, (name, sorted(on_gpu))
    assert not any(n.startswith(cpu.op.name[:-len('logits')])
                   for n in on_gpu)
    # the same graph again and again with fresh inputs
    results = []
    for seed in range(20, 25):
        x = fresh_input(seed).astype(np.float32)
        outs = sess.run([cpu, gpu], {px: x})
        assert np.array_equal(outs[0], outs[1])
        results.append(outs[1])
    assert all(not np.array_equal(results[0], r) for r in results[1:])
