"""MI355X HIP-kernel numerics tests: every hot CDNA4 kernel vs a plain fp32
reference (SURVEY.md §4 strategy — same test body, GPU kernel vs numpy/CPU
fp32). All tests here need a real gfx950 GPU (run via gpurun)."""
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


# ---------------------------------------------------------------------------
# GEMM (the MFMA core) — transpose-detecting asymmetric inputs (guide G9/16)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('m,n,k', [
    (128, 128, 128),      # single interior tile
    (256, 256, 256),      # multi-tile
    (100, 60, 147),       # all edges + odd K (conv1 shape class)
    (256, 64, 576),       # 128x64 variant
    (64, 130, 333),       # 64x128 variant + edges
    (512, 1000, 2048),    # fc-like
])
def test_gemm_bf16_vs_numpy(m, n, k):
    rng = np.random.RandomState(hash((m, n, k)) % 2**31)
    a = rng.randn(m, k).astype(np.float32)
    b = rng.randn(k, n).astype(np.float32)
    with _sess() as s:
        am = tf.constant(_bf16(a), dtype=tf.bfloat16)
        bm = tf.constant(_bf16(b), dtype=tf.bfloat16)
        out = s.run(tf.matmul(am, bm))
    ref = _bf16(a) @ _bf16(b)
    # bf16 mantissa ~8 bits; accumulation in f32
    np.testing.assert_allclose(out, ref, rtol=2e-2, atol=2e-2 * np.sqrt(k))


@pytest.mark.parametrize('ta,tb', [(False, False), (True, False),
                                   (False, True), (True, True)])
def test_gemm_bf16_transposes(ta, tb):
    rng = np.random.RandomState(7)
    m, n, k = 192, 160, 224
    a = rng.randn(*((k, m) if ta else (m, k))).astype(np.float32)
    b = rng.randn(*((n, k) if tb else (k, n))).astype(np.float32)
    with _sess() as s:
        out = s.run(tf.matmul(tf.constant(_bf16(a), dtype=tf.bfloat16),
                              tf.constant(_bf16(b), dtype=tf.bfloat16),
                              transpose_a=ta, transpose_b=tb))
    ref = (_bf16(a).T if ta else _bf16(a)) @ (_bf16(b).T if tb else _bf16(b))
    np.testing.assert_allclose(out, ref, rtol=2e-2, atol=0.4)


def test_gemm_f32_vs_numpy():
    rng = np.random.RandomState(3)
    a = rng.randn(200, 300).astype(np.float32)
    b = rng.randn(300, 150).astype(np.float32)
    with _sess() as s:
        out = s.run(tf.matmul(tf.constant(a), tf.constant(b)))
    np.testing.assert_allclose(out, a @ b, rtol=1e-4, atol=1e-3)


# ---------------------------------------------------------------------------
# conv
# ---------------------------------------------------------------------------
def _conv_ref(x, w, stride, padding):
    n, h, wd, c = x.shape
    r, s, _, kout = w.shape
    if padding == 'SAME':
        p = (h + stride - 1) // stride
        q = (wd + stride - 1) // stride
        ph = max(0, (p - 1) * stride + r - h) // 2
        pw = max(0, (q - 1) * stride + s - wd) // 2
    else:
        p = (h - r) // stride + 1
        q = (wd - s) // stride + 1
        ph = pw = 0
    xp = np.zeros((n, h + 2 * ph + r, wd + 2 * pw + s, c), np.float32)
    xp[:, ph:ph + h, pw:pw + wd, :] = x
    out = np.zeros((n, p, q, kout), np.float32)
    for i in range(p):
        for j in range(q):
            patch = xp[:, i * stride:i * stride + r, j * stride:j * stride + s, :]
            out[:, i, j, :] = np.tensordot(patch, w, axes=3)
    return out


@pytest.mark.parametrize('shape,filt,stride,padding', [
    ((2, 16, 16, 8), (3, 3, 8, 16), 1, 'SAME'),
    ((2, 16, 16, 8), (1, 1, 8, 32), 1, 'SAME'),
    ((2, 17, 17, 8), (3, 3, 8, 16), 2, 'SAME'),
    ((2, 32, 32, 3), (7, 7, 3, 64), 2, 'SAME'),  # conv1 class (C=3, odd K)
])
def test_conv2d_fwd(shape, filt, stride, padding):
    rng = np.random.RandomState(1)
    x = _bf16(rng.randn(*shape) * 0.5)
    w = _bf16(rng.randn(*filt) * 0.2)
    with _sess() as s:
        y = tf.nn.conv2d(tf.constant(x, dtype=tf.bfloat16),
                         tf.constant(w, dtype=tf.bfloat16),
                         [1, stride, stride, 1], padding)
        out = s.run(y)
    ref = _conv_ref(x, w, stride, padding)
    np.testing.assert_allclose(out, ref, rtol=3e-2, atol=0.15)


def test_conv2d_grads_vs_cpu():
    """GPU bf16 conv grads vs CPU f32 conv grads on the same values."""
    rng = np.random.RandomState(5)
    x = _bf16(rng.randn(2, 10, 10, 8) * 0.5)
    w = _bf16(rng.randn(3, 3, 8, 16) * 0.2)
    dy_shape = (2, 10, 10, 16)
    dy = _bf16(rng.randn(*dy_shape) * 0.1)
    g = tf.get_default_graph()
    with _sess() as s:
        # GPU bf16
        xg = tf.constant(x, dtype=tf.bfloat16)
        wg = tf.constant(w, dtype=tf.bfloat16)
        dyg = tf.constant(dy, dtype=tf.bfloat16)
        dxg = tf.nn.conv2d_backprop_input([2, 10, 10, 8], wg, dyg,
                                          [1, 1, 1, 1], 'SAME')
        dwg = tf.nn.conv2d_backprop_filter(xg, [3, 3, 8, 16], dyg,
                                           [1, 1, 1, 1], 'SAME')
        # CPU f32 reference
        with tf.device('/cpu:0'):
            xc = tf.constant(x)
            wc = tf.constant(w)
            dyc = tf.constant(dy)
            dxc = tf.nn.conv2d_backprop_input([2, 10, 10, 8], wc, dyc,
                                              [1, 1, 1, 1], 'SAME')
            dwc = tf.nn.conv2d_backprop_filter(xc, [3, 3, 8, 16], dyc,
                                               [1, 1, 1, 1], 'SAME')
        gdx, gdw, cdx, cdw = s.run([dxg, dwg, dxc, dwc])
    np.testing.assert_allclose(gdx, cdx, rtol=3e-2, atol=0.1)
    np.testing.assert_allclose(gdw, cdw, rtol=3e-2, atol=0.3)


# One case per Conv2D dispatch path: GPU bf16 vs the CPU f32 kernels on the
# same bf16-rounded values.
def _conv_out_shape(shape, filt, stride, padding):
    n, h, w, _ = shape
    r, s, _, k = filt
    if padding == 'SAME':
        return (n, -(-h // stride), -(-w // stride), k)
    return (n, (h - r) // stride + 1, (w - s) // stride + 1, k)


def _conv_gpu_vs_cpu(op, shape, filt, stride, padding):
    rng = np.random.RandomState(9)
    x = _bf16(rng.randn(*shape) * 0.5)
    w = _bf16(rng.randn(*filt) * 0.2)
    dy = _bf16(rng.randn(*_conv_out_shape(shape, filt, stride, padding)) * 0.1)
    strides = [1, stride, stride, 1]

    def build(dtype):
        xt, wt, dyt = (tf.constant(v, dtype=dtype) for v in (x, w, dy))
        if op == 'fwd':
            return tf.nn.conv2d(xt, wt, strides, padding)
        if op == 'dw':
            return tf.nn.conv2d_backprop_filter(xt, list(filt), dyt, strides,
                                                padding)
        return tf.nn.conv2d_backprop_input(list(shape), wt, dyt, strides,
                                           padding)

    with _sess() as s:
        gpu = build(tf.bfloat16)
        with tf.device('/cpu:0'):
            cpu = build(tf.float32)
        return s.run([gpu, cpu])


@pytest.mark.parametrize('shape,filt,stride,padding', [
    ((1, 16, 16, 8), (3, 3, 8, 64), 1, 'SAME'),   # implicit 8-phase (M=256)
    ((2, 16, 16, 8), (1, 1, 8, 16), 2, 'SAME'),   # strided 1x1: implicit NT
    ((2, 9, 9, 8), (3, 3, 8, 12), 1, 'SAME'),     # cout%8!=0: im2col + w^T
    ((2, 12, 12, 8), (3, 3, 8, 16), 1, 'VALID'),  # VALID padding
])
def test_conv2d_fwd_paths(shape, filt, stride, padding):
    out, ref = _conv_gpu_vs_cpu('fwd', shape, filt, stride, padding)
    assert out.shape == _conv_out_shape(shape, filt, stride, padding)
    np.testing.assert_allclose(out, ref, rtol=3e-2, atol=0.15)


@pytest.mark.parametrize('shape,filt,stride,padding', [
    ((1, 8, 8, 8), (3, 3, 8, 16), 1, 'SAME'),     # implicit dW, M=64, split 1
    ((4, 16, 16, 8), (3, 3, 8, 16), 1, 'SAME'),   # implicit dW, split 2, arena
    ((1, 16, 16, 3), (7, 7, 3, 8), 2, 'SAME'),    # stem channel-pad + unpad
    ((2, 10, 10, 8), (1, 1, 8, 16), 1, 'SAME'),   # 1x1 K-major direct
    ((2, 9, 9, 8), (3, 3, 8, 12), 1, 'SAME'),     # cout%8!=0: im2col fallback
])
def test_conv2d_dw_paths(shape, filt, stride, padding):
    out, ref = _conv_gpu_vs_cpu('dw', shape, filt, stride, padding)
    assert out.shape == filt
    np.testing.assert_allclose(out, ref, rtol=3e-2, atol=0.3)


def test_conv2d_dx_strided_col2im():
    shape = (2, 17, 17, 8)
    out, ref = _conv_gpu_vs_cpu('dx', shape, (3, 3, 8, 16), 2, 'SAME')
    assert out.shape == shape
    np.testing.assert_allclose(out, ref, rtol=3e-2, atol=0.1)


# ---------------------------------------------------------------------------
# batch norm / softmax / xent
# ---------------------------------------------------------------------------
def test_batch_norm_mi():
    from simple_tensorflow_amd.python.framework.ops import apply_op
    rng = np.random.RandomState(2)
    x = _bf16(rng.randn(64, 32) * 2 + 1)
    scale = rng.rand(32).astype(np.float32) + 0.5
    offset = rng.randn(32).astype(np.float32)
    with _sess() as s:
        y, mean, var, inv = apply_op('BatchNormMi',
                                     tf.constant(x, dtype=tf.bfloat16),
                                     tf.constant(scale), tf.constant(offset),
                                     epsilon=1e-4)
        yv, mv, vv = s.run([y, mean, var])
    m_ref = x.mean(0)
    v_ref = x.var(0)
    np.testing.assert_allclose(mv, m_ref, rtol=1e-2, atol=1e-2)
    np.testing.assert_allclose(vv, v_ref, rtol=2e-2, atol=2e-2)
    y_ref = (x - m_ref) / np.sqrt(v_ref + 1e-4) * scale + offset
    np.testing.assert_allclose(yv, y_ref, rtol=3e-2, atol=5e-2)


def test_softmax_gpu():
    rng = np.random.RandomState(4)
    x = rng.randn(32, 100).astype(np.float32)
    with _sess() as s:
        out = s.run(tf.nn.softmax(tf.constant(x)))
    e = np.exp(x - x.max(1, keepdims=True))
    np.testing.assert_allclose(out, e / e.sum(1, keepdims=True), rtol=1e-4,
                               atol=1e-6)


def test_sparse_xent_gpu():
    rng = np.random.RandomState(6)
    logits = rng.randn(16, 1000).astype(np.float32)
    labels = rng.randint(0, 1000, 16)
    with _sess() as s:
        loss = tf.nn.sparse_softmax_cross_entropy_with_logits(
            labels=tf.constant(labels, dtype=tf.int64),
            logits=tf.constant(logits))
        out = s.run(loss)
    e = np.exp(logits - logits.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    ref = -np.log(p[np.arange(16), labels])
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------
# pooling / reductions / elementwise
# ---------------------------------------------------------------------------
def test_max_pool_fwd_bwd():
    rng = np.random.RandomState(8)
    x = rng.randn(2, 8, 8, 4).astype(np.float32)
    with _sess() as s:
        xg = tf.constant(x)
        y = tf.nn.max_pool(xg, [1, 2, 2, 1], [1, 2, 2, 1], 'VALID')
        (dx,) = tf.gradients(tf.reduce_sum(y), [xg])
        yv, dxv = s.run([y, dx])
    ref = x.reshape(2, 4, 2, 4, 2, 4).max(axis=(2, 4))
    np.testing.assert_allclose(yv, ref, rtol=1e-6)
    # every window contributes 1 to its argmax
    assert dxv.sum() == pytest.approx(2 * 4 * 4 * 4)


def test_reductions_gpu():
    rng = np.random.RandomState(9)
    x = rng.randn(64, 50).astype(np.float32)
    with _sess() as s:
        t = tf.constant(x)
        full = s.run(tf.reduce_sum(t))
        rows = s.run(tf.reduce_sum(t, 1))
        cols = s.run(tf.reduce_mean(t, 0))
        mx = s.run(tf.reduce_max(t))
    np.testing.assert_allclose(full, x.sum(), rtol=1e-4)
    np.testing.assert_allclose(rows, x.sum(1), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(cols, x.mean(0), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(mx, x.max(), rtol=1e-6)


def test_elementwise_bf16():
    rng = np.random.RandomState(10)
    a = _bf16(rng.randn(1000))
    b = _bf16(rng.rand(1000) + 0.5)
    with _sess() as s:
        ag = tf.constant(a, dtype=tf.bfloat16)
        bg = tf.constant(b, dtype=tf.bfloat16)
        add = s.run(ag + bg)
        mul = s.run(ag * bg)
        rl = s.run(tf.nn.relu(ag))
        tnh = s.run(tf.tanh(ag))
    np.testing.assert_allclose(add, _bf16(a + b), rtol=2e-2, atol=2e-2)
    np.testing.assert_allclose(mul, _bf16(a * b), rtol=2e-2, atol=2e-2)
    np.testing.assert_allclose(rl, np.maximum(a, 0), rtol=2e-2, atol=1e-3)
    np.testing.assert_allclose(tnh, np.tanh(a), rtol=3e-2, atol=2e-2)


def test_bias_add_grad_gpu():
    rng = np.random.RandomState(11)
    dy = rng.randn(128, 32).astype(np.float32)
    with _sess() as s:
        from simple_tensorflow_amd.python.framework.ops import apply_op
        db = s.run(apply_op('BiasAddGrad', tf.constant(dy)))
    np.testing.assert_allclose(db, dy.sum(0), rtol=1e-4, atol=1e-3)


def test_transpose_gpu():
    rng = np.random.RandomState(12)
    x = rng.randn(100, 70).astype(np.float32)
    with _sess() as s:
        out = s.run(tf.transpose(tf.constant(x)))
    np.testing.assert_allclose(out, x.T)


def test_random_uniform_gpu():
    with _sess() as s:
        u = s.run(tf.random_uniform([100000], seed=42))
    assert 0.0 <= u.min() and u.max() < 1.0
    assert abs(u.mean() - 0.5) < 0.01


def test_training_step_decreases_loss_mlp():
    """End-to-end GPU training: 2-layer bf16 MLP on synthetic data."""
    rng = np.random.RandomState(13)
    x_np = _bf16(rng.randn(256, 64))
    y_np = rng.randint(0, 10, 256).astype(np.int64)
    from simple_tensorflow_amd.python.ops import variables, array_ops
    x = tf.constant(x_np, dtype=tf.bfloat16)
    labels = tf.constant(y_np, dtype=tf.int64)
    w1 = variables.Variable(tf.truncated_normal([64, 128], stddev=0.1, seed=1))
    w2 = variables.Variable(tf.truncated_normal([128, 10], stddev=0.1, seed=2))
    h = tf.nn.relu(tf.matmul(x, tf.cast(w1.ref(), tf.bfloat16)))
    logits = tf.cast(tf.matmul(h, tf.cast(w2.ref(), tf.bfloat16)), tf.float32)
    loss = tf.reduce_mean(tf.nn.sparse_softmax_cross_entropy_with_logits(
        labels=labels, logits=logits))
    train = tf.train.MomentumOptimizer(0.05, 0.9).minimize(loss)
    with _sess() as s:
        s.run(tf.global_variables_initializer())
        l0 = s.run(loss)
        for _ in range(30):
            s.run(train)
        l1 = s.run(loss)
    assert np.isfinite(l0) and np.isfinite(l1)
    assert l1 < 0.7 * l0


# ---------------------------------------------------------------------------
# Conv2DBackpropInputAdd: residual-gradient add fused into the dx GEMM
# epilogue (8-phase path) — vs the unfused AddN graph and an fp32 reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('cin,cout,hw,fused_path', [
    (64, 128, 16, True),     # M=2*16*16=512 %256, 8ph-eligible
    (64, 72, 16, False),     # cout%8==0 but N=cin... K=72 not %64 -> fallback
])
def test_conv_dx_side_add_fused(cin, cout, hw, fused_path):
    import os
    rng = np.random.RandomState(11)
    n = 2
    xv = rng.randn(n, hw, hw, cin).astype(np.float32) * 0.5
    wv = rng.randn(1, 1, cin, cout).astype(np.float32) * 0.1
    bv = rng.randn(n, hw, hw, cin).astype(np.float32) * 0.5

    def build():
        x = tf.constant(_bf16(xv), dtype=tf.bfloat16)
        w = tf.constant(_bf16(wv), dtype=tf.bfloat16)
        b = tf.constant(_bf16(bv), dtype=tf.bfloat16)
        y = tf.nn.conv2d(x, w, [1, 1, 1, 1], 'SAME')
        loss = tf.reduce_sum(tf.cast(y, tf.float32)) + \
            tf.reduce_sum(tf.cast(x * b, tf.float32))
        return tf.gradients(loss, [x])[0]

    g = build()
    assert g.op.type == 'Conv2DBackpropInputAdd'
    with _sess() as s:
        out = s.run(tf.cast(g, tf.float32))

    os.environ['STF_NO_CONV_DX_FUSE'] = '1'
    try:
        tf.reset_default_graph()
        g2 = build()
        assert g2.op.type in ('AddN', 'Add')
        with _sess() as s:
            out2 = s.run(tf.cast(g2, tf.float32))
    finally:
        del os.environ['STF_NO_CONV_DX_FUSE']

    # fused epilogue does the identical bf16+bf16 add -> bit-exact match
    np.testing.assert_array_equal(out, out2)
    ref = _bf16(wv[0, 0]).sum(axis=1)[None, None, None, :] + _bf16(bv)
    np.testing.assert_allclose(out, ref, rtol=3e-2, atol=3e-2 * cout)
