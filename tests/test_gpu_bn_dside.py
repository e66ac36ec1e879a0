"""BatchNormAddReluMiGrad: the residual branch's gradient dside is stored by
the BN backward kernel itself. It must be exactly relu_grad(dy, y_relu);
dx / dscale / doffset are checked against a float64 BN backward."""
import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.framework.ops import apply_op

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def fresh_graph():
    tf.reset_default_graph()
    yield


def _bf16(x):
    """round-trip f32 -> bf16 -> f32 (numpy)"""
    bits = np.asarray(x, np.float32).view(np.uint32)
    lsb = (bits >> 16) & 1
    out = ((bits + 0x7FFF + lsb) >> 16).astype(np.uint32) << 16
    return out.view(np.float32)


def _grad_close_bf16(got, want, bound=0.15):
    # the bound test_gpu_vs_torch.py puts on the bf16 BN gradients
    rel = np.abs(got - want) / (np.abs(want) + 0.1)
    assert np.percentile(rel, 99) < bound


def _inputs(rows, C, seed):
    rng = np.random.RandomState(seed)
    x = _bf16(rng.randn(rows, C))
    dy = _bf16(rng.randn(rows, C))
    # hand-made forward output: positive values, exact zeros (both signs) and
    # negative values, which a real ReLU output never holds
    y = _bf16(rng.randn(rows, C))
    pick = rng.randint(0, 4, (rows, C))
    y[pick == 0] = 0.0
    y[pick == 1] = -0.0
    scale = (rng.rand(C) + 0.5).astype(np.float32)
    mean = x.astype(np.float64).mean(0).astype(np.float32)
    inv_std = (1.0 / np.sqrt(x.astype(np.float64).var(0) + 1e-4)) \
        .astype(np.float32)
    return x, dy, y, scale, mean, inv_std


def _reference(x, dy, y, scale, mean, inv_std):
    """float64 BN backward on the ReLU-masked gradient."""
    g = np.where(y > 0, dy, 0.0).astype(np.float64)
    xhat = (x.astype(np.float64) - mean) * inv_std
    doffset = g.sum(0)
    dscale = (g * xhat).sum(0)
    rows = x.shape[0]
    dx = scale * inv_std * (g - doffset / rows - xhat * dscale / rows)
    return dx, dscale, doffset


@pytest.mark.parametrize('rows,C', [
    (35, 24),     # 8-wide kernel: 3 channel windows, inactive tail threads
    (1000, 16),   # 8-wide kernel: several blocks
    (35, 12),     # C % 8 != 0: scalar bf16 kernel
])
def test_bn_add_relu_grad_dside(rows, C):
    x, dy, y, scale, mean, inv_std = _inputs(rows, C, seed=30 + C)
    outs = apply_op('BatchNormAddReluMiGrad',
                    tf.constant(dy, dtype=tf.bfloat16),
                    tf.constant(x, dtype=tf.bfloat16), tf.constant(scale),
                    tf.constant(mean), tf.constant(inv_std),
                    tf.constant(y, dtype=tf.bfloat16), epsilon=1e-4)
    assert len(outs) == 4
    s = tf.Session()
    assert s.num_gpus() > 0
    with s:
        dx, dscale, doffset, dside = s.run(
            [tf.cast(outs[0], tf.float32), outs[1], outs[2],
             tf.cast(outs[3], tf.float32)])

    want_dside = np.where(y > 0, dy, np.float32(0.0))
    np.testing.assert_array_equal(dside, want_dside)
    # bit-exact: a masked element is +0, a kept -0 stays -0
    np.testing.assert_array_equal(dside.view(np.uint32),
                                  want_dside.astype(np.float32)
                                  .view(np.uint32))

    want_dx, want_dscale, want_doffset = _reference(x, dy, y, scale, mean,
                                                    inv_std)
    for name, got, want in (('dx', dx, want_dx), ('dscale', dscale,
                                                  want_dscale),
                            ('doffset', doffset, want_doffset)):
        print(name, 'max abs err', np.abs(got - want).max())
        _grad_close_bf16(got, want)
