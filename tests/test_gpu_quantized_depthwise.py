"""QuantizedDepthwiseConv2D and its fused form on the GPU (DwQ8 in
csrc/kernels/hip/depthwise_q8.hip) against the numpy reference and the case
table of tests/test_quantized_depthwise.py, np.array_equal on all three
outputs. Operands, bias and ranges come through placeholders, so nothing is
folded onto the CPU. All tests need a gfx950 GPU."""
import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.ops import quantized_ops as q

from test_gpu_kernels import _sess
from test_gpu_quantized import _trace_run
from test_quantized_depthwise import (ACTIVATIONS, CASES, FILLS, FILL_SHAPES,
                                      case_id, check_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def sess():
    tf.reset_default_graph()
    with _sess() as s:
        yield s


@pytest.mark.parametrize('activation', [None] + ACTIVATIONS)
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_depthwise_op(sess, case, activation):
    check_case(sess, '/gpu:0', case, activation)


@pytest.mark.parametrize('fill', FILLS)
@pytest.mark.parametrize('shape', FILL_SHAPES, ids=case_id)
def test_depthwise_op_fills(sess, shape, fill):
    check_case(sess, '/gpu:0', (shape, None, 3),
               'Relu6' if fill == 'all255' else 'None', fill)


def test_refused_geometry(sess):
    """The cheapest geometry stf_depthwise_q8_ok refuses: a 1 x 200 filter's
    int32 and packed slices alone pass the kernel's 64 KiB of LDS."""
    px = tf.placeholder(tf.uint8, (1, 1, 1, 1))
    pw = tf.placeholder(tf.uint8, (1, 200, 1, 1))
    with tf.device('/gpu:0'):
        out = q.quantized_depthwise_conv2d(px, pw, 0.0, 1.0, 0.0, 1.0,
                                           [1, 1, 1, 1], 'SAME')[0]
    with pytest.raises(tf.errors.InvalidArgumentError, match='tiles'):
        sess.run(out, {px: np.zeros((1, 1, 1, 1), np.uint8),
                       pw: np.zeros((1, 200, 1, 1), np.uint8)})


def test_fused_node_runs_on_the_gpu(sess):
    """In a trace, and again past the point where the step is captured and
    replayed."""
    outs, feeds, want = check_case(sess, '/gpu:0', CASES[2], 'Relu6')
    name = outs[0].op.name
    got, on_gpu = _trace_run(sess, list(outs), feeds)
    assert name in on_gpu, (name, sorted(on_gpu))
    for _ in range(5):
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        got = sess.run(list(outs), feeds)
