"""QuantizedConv2DWithBiasAndRequantize and
QuantizedMatMulWithBiasAndRequantize on the GPU (GemmI8Fused in
csrc/kernels/hip/gemm_i8_fused.hip) against the numpy reference of
tests/test_quantized_fused.py, np.array_equal on all three outputs. Operands
and bias come through placeholders, so nothing is folded onto the CPU. The
shapes are the smallest that reach each path of the kernel: all-border
pixels, row and column block tails, K tails, both tile widths, the byte-store
path (N % 16 != 0), im2col, packed and unpacked A, an empty output. All tests
need a gfx950 GPU."""
import numpy as np
import pytest

import simple_tensorflow_amd as tf

from test_gpu_kernels import _sess
from test_gpu_quantized import _trace_run
from test_quantized_fused import (ACTIVATIONS, FILLS, FILL_SHAPES, SHAPES,
                                  build_and_expect, check_case, shape_id)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def sess():
    tf.reset_default_graph()
    with _sess() as s:
        yield s


@pytest.mark.parametrize('activation', ACTIVATIONS)
@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_fused_op(sess, shape, activation):
    check_case(sess, '/gpu:0', shape, activation, 'random',
               SHAPES.index(shape))


@pytest.mark.parametrize('fill', FILLS)
@pytest.mark.parametrize('shape', FILL_SHAPES, ids=shape_id)
def test_fused_op_fills(sess, shape, fill):
    check_case(sess, '/gpu:0', shape, 'Relu6' if fill == 'all255' else 'None',
               fill, 3)


def test_fused_node_runs_on_the_gpu(sess):
    """In a trace, and again past the point where the step is captured and
    replayed."""
    with tf.device('/gpu:0'):
        outs, feeds, want, _ = build_and_expect(SHAPES[1], 'Relu', 'random', 1)
    name = outs[0].op.name
    got, on_gpu = _trace_run(sess, outs, feeds)
    assert name in on_gpu, (name, sorted(on_gpu))
    for _ in range(5):
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        got = sess.run(outs, feeds)
