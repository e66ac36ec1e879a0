"""BatchNormAddReluMiGrad: the grad-stats kernel stores dside, the grad kernel
reads it back as its gradient and no longer loads dy or y_relu.

Exact-grid data (mean 0, inv_std 1, scale a power of two, x in eighths,
integer dy): every product and sum is exact in f32, so dside, dx, dscale and
doffset must be bit-equal to numpy. y is hand-made: positives, both zeros and
negatives.

The rule for a NaN in y_relu: dside is 0 there and the element contributes
nothing to dx, dscale or doffset (g is what dside holds). A ReLU output
cannot hold a NaN."""
import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.framework.ops import apply_op
from test_gpu_bn_dside import _bf16

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def fresh_graph():
    tf.reset_default_graph()
    yield


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _inputs(rows, C, with_nan):
    rng = np.random.RandomState(rows + C)
    x = rng.randint(-32, 33, (rows, C)).astype(np.float32) / 8
    dy = rng.randint(-3, 4, (rows, C)).astype(np.float32)
    dy[dy == 0] = -0.0             # a kept -0 must stay -0 in dside
    scale = rng.choice([0.5, 1.0, 2.0], C).astype(np.float32)
    y = _bf16(rng.randn(rows, C))
    pick = rng.randint(0, 4, (rows, C))
    y[pick == 0] = 0.0
    y[pick == 1] = -0.0
    if with_nan:
        y[rng.randint(0, 8, (rows, C)) == 0] = np.nan
    return x, dy, y, scale


def _want(x, dy, y, scale):
    rows = x.shape[0]
    dside = np.where(y > 0, dy, np.float32(0.0)).astype(np.float32)
    g, x64 = dside.astype(np.float64), x.astype(np.float64)
    doffset = g.sum(0)
    dscale = (g * x64).sum(0)
    dx = scale * (g - doffset / rows - x64 * dscale / rows)
    return (_bf16(dx.astype(np.float32)), dscale.astype(np.float32),
            doffset.astype(np.float32), dside)


@pytest.mark.parametrize('rows,C,with_nan', [
    (64, 24, False),     # 8-wide kernels: 3 channel windows
    (1024, 16, False),   # 8-wide kernels: several blocks
    (64, 12, False),     # C % 8 != 0: scalar bf16 kernels
    (64, 24, True),      # NaN in y_relu, 8-wide kernels
    (64, 12, True),      # NaN in y_relu, scalar kernels
], ids=['64x24', '1024x16', '64x12', '64x24-nan', '64x12-nan'])
def test_tail_grad_bit_equal_on_exact_data(rows, C, with_nan):
    x, dy, y, scale = _inputs(rows, C, with_nan)
    outs = apply_op('BatchNormAddReluMiGrad',
                    tf.constant(dy, dtype=tf.bfloat16),
                    tf.constant(x, dtype=tf.bfloat16), tf.constant(scale),
                    tf.constant(np.zeros(C, np.float32)),
                    tf.constant(np.ones(C, np.float32)),
                    tf.constant(y, dtype=tf.bfloat16), epsilon=1e-4)
    assert len(outs) == 4
    s = tf.Session()
    assert s.num_gpus() > 0
    with s:
        got = s.run([tf.cast(outs[0], tf.float32), outs[1], outs[2],
                     tf.cast(outs[3], tf.float32)])
    want = _want(x, dy, y, scale)
    if with_nan:
        nan = np.isnan(y)
        assert nan.any() and (_bits(want[3])[nan] == 0).all()
    # masked is +0, a kept -0 stays -0
    assert (_bits(want[3]) == 0x80000000).any()
    for name, g, w in zip(('dx', 'dscale', 'doffset', 'dside'), got, want):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=name)
