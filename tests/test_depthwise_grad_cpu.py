"""The CPU kernels of DepthwiseConv2dNativeBackpropInput and ...Filter
(csrc/kernels/cpu_nn.cc) for float32, against the float64 tap loops of
test_gpu_nn._depthwise_ref. Operands are small integers, so every sum is an
integer far below 2^24 and the result is exact."""
import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.framework.ops import apply_op

from test_gpu_nn import _depthwise_ref, _geom

# (x shape, (R, S, mult), stride, padding)
CASES = [
    ((2, 9, 13, 36), (3, 3, 1), 2, 'SAME'),   # odd sizes, asymmetric padding
    ((1, 8, 10, 5), (3, 2, 2), 1, 'VALID'),   # mult 2, non-square filter
    ((2, 7, 7, 3), (1, 1, 1), 2, 'VALID'),    # stride over a 1x1 window
]


@pytest.mark.parametrize('xshape,filt,stride,padding', CASES,
                         ids=['3x3-s2-same', '3x2-m2-valid', '1x1-s2-valid'])
def test_depthwise_backprop_on_cpu(xshape, filt, stride, padding):
    n, h, w, c = xshape
    r, s, mult = filt
    g = _geom(h, w, (r, s), (stride, stride), padding)
    rng = np.random.RandomState(7)
    x = rng.randint(-2, 3, xshape).astype(np.float32)
    k = rng.randint(-2, 3, (r, s, c, mult)).astype(np.float32)
    dy = rng.randint(-2, 3, (n, g.P, g.Q, c * mult)).astype(np.float32)
    attrs = dict(strides=[1, stride, stride, 1], padding=padding)
    tf.reset_default_graph()
    with tf.device('/cpu:0'):
        xt, kt, dyt = (tf.constant(a) for a in (x, k, dy))
        y = tf.nn.depthwise_conv2d(xt, kt, **attrs)
        by_grad = tf.gradients(tf.reduce_sum(y * dyt), [xt, kt])
        by_op = [
            apply_op('DepthwiseConv2dNativeBackpropInput',
                     tf.constant(list(xshape), dtype=tf.int32), kt, dyt,
                     **attrs),
            apply_op('DepthwiseConv2dNativeBackpropFilter', xt,
                     tf.constant([r, s, c, mult], dtype=tf.int32), dyt,
                     **attrs)]
    with tf.Session() as sess:
        outs = sess.run(by_op + by_grad)
    _, (dx, _), (dw, _) = _depthwise_ref(x, k, dy, g)
    for out, want in zip(outs, (dx, dw, dx, dw)):
        assert out.dtype == np.float32 and out.shape == want.shape
        np.testing.assert_array_equal(out, want.astype(np.float32))
