"""Implicit-GEMM backward-input of stride-1 convolutions, and the residual
`side` folded into the dx store (8-phase epilogue, col2im).

GPU bf16 conv2d_backprop_input vs the CPU f32 kernel on the same bf16-rounded
values, at the dx tolerance of test_gpu_kernels.py. Every case is also run
with STF_NO_IMPLICIT_DX=1 (GEMM + col2im) in a fresh graph; both maximum
errors are printed."""
import os

import numpy as np
import pytest

import simple_tensorflow_amd as tf

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


def _sess():
    s = tf.Session()
    assert s.num_gpus() > 0
    return s


def _dy_shape(shape, filt, padding):
    n, h, w, _ = shape
    r, s, _, k = filt
    if padding == 'SAME':
        return (n, h, w, k)
    return (n, h - r + 1, w - s + 1, k)


def _dx(shape, filt, padding, w, dy, dtype, device=None):
    def build():
        return tf.nn.conv2d_backprop_input(
            list(shape), tf.constant(w, dtype=dtype),
            tf.constant(dy, dtype=dtype), [1, 1, 1, 1], padding)
    if device is None:
        return build()
    with tf.device(device):
        return build()


def _with_env(name, fn):
    """fn() in a fresh graph with the switch `name` set."""
    os.environ[name] = '1'
    try:
        tf.reset_default_graph()
        return fn()
    finally:
        del os.environ[name]


CASES = [
    ((1, 16, 16, 64), (3, 3, 64, 64), 'SAME'),    # 8-phase, NR=1
    ((1, 16, 16, 128), (3, 3, 128, 64), 'SAME'),  # NR=2
    ((1, 16, 16, 256), (3, 3, 256, 64), 'SAME'),  # NR=4
    ((1, 16, 16, 64), (3, 3, 64, 64), 'VALID'),   # dy is 14x14, pad' = 2
    ((1, 16, 16, 64), (2, 2, 64, 64), 'SAME'),    # even filter, asymmetric pad
    ((1, 16, 16, 64), (1, 7, 64, 64), 'SAME'),    # non-square filter
    ((1, 16, 16, 64), (3, 3, 64, 8), 'SAME'),     # R*S*K = 72, padded to 128
    # M = 200 is outside the 8-phase gate. An implicit dx through the general
    # NT GEMM template was measured slower on Inception v3 and is not built:
    # this shape takes GEMM + col2im
    ((2, 10, 10, 8), (3, 3, 8, 16), 'SAME'),
]


def _run_case(shape, filt, padding):
    rng = np.random.RandomState(9)
    w = _bf16(rng.randn(*filt) * 0.2)
    dy = _bf16(rng.randn(*_dy_shape(shape, filt, padding)) * 0.1)

    with _sess() as s:
        out, ref = s.run([_dx(shape, filt, padding, w, dy, tf.bfloat16),
                          _dx(shape, filt, padding, w, dy, tf.float32,
                              '/cpu:0')])

    def col2im():
        with _sess() as s:
            return s.run(_dx(shape, filt, padding, w, dy, tf.bfloat16))
    old = _with_env('STF_NO_IMPLICIT_DX', col2im)
    print('max abs err vs CPU f32: implicit %.4g, gemm+col2im %.4g'
          % (np.abs(out - ref).max(), np.abs(old - ref).max()))
    return out, old, ref


@pytest.mark.parametrize('shape,filt,padding', CASES)
def test_conv2d_dx_implicit(shape, filt, padding):
    out, old, ref = _run_case(shape, filt, padding)
    assert out.shape == shape
    np.testing.assert_allclose(out, ref, rtol=3e-2, atol=0.1)
    np.testing.assert_allclose(old, ref, rtol=3e-2, atol=0.1)


def test_conv2d_dx_cout_not_multiple_of_8_keeps_col2im():
    # K % 8 != 0 is outside the implicit gate: the switch changes nothing
    shape, filt = (2, 9, 9, 8), (3, 3, 8, 12)
    out, old, ref = _run_case(shape, filt, 'SAME')
    assert out.shape == shape
    np.testing.assert_allclose(out, ref, rtol=3e-2, atol=0.1)
    np.testing.assert_array_equal(out, old)


def _side_add_case(filt, stride):
    """x feeds a conv and an elementwise branch; returns the fused
    (Conv2DBackpropInputAdd) and the unfused (STF_NO_CONV_DX_FUSE) dx."""
    rng = np.random.RandomState(11)
    shape = (2, 16, 16, 64)
    xv = _bf16(rng.randn(*shape) * 0.5)
    wv = _bf16(rng.randn(*filt) * 0.1)
    bv = _bf16(rng.randn(*shape) * 0.5)

    def build():
        x = tf.constant(xv, dtype=tf.bfloat16)
        w = tf.constant(wv, dtype=tf.bfloat16)
        b = tf.constant(bv, dtype=tf.bfloat16)
        y = tf.nn.conv2d(x, w, [1, stride, stride, 1], 'SAME')
        loss = tf.reduce_sum(tf.cast(y, tf.float32)) + \
            tf.reduce_sum(tf.cast(x * b, tf.float32))
        return tf.gradients(loss, [x])[0]

    g = build()
    assert g.op.type == 'Conv2DBackpropInputAdd'
    with _sess() as s:
        fused = s.run(tf.cast(g, tf.float32))

    def unfused():
        g2 = build()
        assert g2.op.type in ('AddN', 'Add')
        with _sess() as s:
            return s.run(tf.cast(g2, tf.float32))
    return fused, _with_env('STF_NO_CONV_DX_FUSE', unfused), bv


def test_conv_dx_3x3_side_add_bit_equal_to_unfused():
    # 8-phase implicit dx: the epilogue rounds to bf16, then adds side
    fused, unfused, bv = _side_add_case((3, 3, 64, 64), 1)
    np.testing.assert_array_equal(fused, unfused)
    assert np.abs(fused - bv).max() > 0.1   # the conv term is there


def test_conv_dx_strided_1x1_side_add_bit_equal_to_unfused():
    # strided conv keeps GEMM + col2im; col2im adds side in its store
    fused, unfused, bv = _side_add_case((1, 1, 64, 128), 2)
    np.testing.assert_array_equal(fused, unfused)
    assert np.abs(fused - bv).max() > 0.1
