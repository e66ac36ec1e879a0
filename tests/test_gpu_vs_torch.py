"""HIP kernel numerics vs plain PyTorch fp32 references (CPU torch): the
framework's GPU ops must agree with an independent implementation, not just
our own CPU kernels."""
import numpy as np
import pytest

import simple_tensorflow_amd as tf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


@pytest.fixture(autouse=True)
def fresh_graph():
    tf.reset_default_graph()
    yield


def _run(t):
    with tf.Session() as s:
        return s.run(t)


def test_matmul_bf16_vs_torch():
    rng = np.random.RandomState(0)
    a = rng.randn(192, 320).astype(np.float32)
    b = rng.randn(320, 256).astype(np.float32)
    got = _run(tf.matmul(tf.constant(a, dtype=tf.bfloat16),
                         tf.constant(b, dtype=tf.bfloat16)))
    # bf16 inputs: compare against torch bf16 matmul upcast to f32
    want = (torch.from_numpy(a).bfloat16().float() @
            torch.from_numpy(b).bfloat16().float()).numpy()
    rel = np.abs(got - want) / (np.abs(want) + 1e-2)
    assert np.percentile(rel, 99) < 0.05


def test_conv2d_bf16_vs_torch():
    rng = np.random.RandomState(1)
    x = rng.randn(2, 16, 16, 8).astype(np.float32)
    w = rng.randn(3, 3, 8, 16).astype(np.float32)
    got = _run(tf.nn.conv2d(tf.constant(x, dtype=tf.bfloat16),
                            tf.constant(w, dtype=tf.bfloat16),
                            [1, 1, 1, 1], 'SAME'))
    tx = torch.from_numpy(x).permute(0, 3, 1, 2)
    tw = torch.from_numpy(w).permute(3, 2, 0, 1)
    want = torch.nn.functional.conv2d(tx, tw, padding=1) \
        .permute(0, 2, 3, 1).numpy()
    assert np.abs(got - want).max() / (np.abs(want).max() + 1e-6) < 0.05


def test_batch_norm_vs_torch():
    from simple_tensorflow_amd.python.framework.ops import apply_op
    rng = np.random.RandomState(2)
    x = rng.randn(4, 8, 8, 32).astype(np.float32)
    scale = rng.rand(32).astype(np.float32) + 0.5
    offset = rng.randn(32).astype(np.float32)
    y, mean, var, _ = apply_op('BatchNormMi',
                               tf.constant(x, dtype=tf.bfloat16),
                               tf.constant(scale), tf.constant(offset),
                               epsilon=1e-4)
    got_y, got_mean = _run([y, mean])
    tx = torch.from_numpy(x).permute(0, 3, 1, 2)
    want = torch.nn.functional.batch_norm(
        tx, None, None, torch.from_numpy(scale),
        torch.from_numpy(offset), training=True, eps=1e-4) \
        .permute(0, 2, 3, 1).numpy()
    assert np.abs(got_y - want).max() < 0.1  # bf16 rounding
    np.testing.assert_allclose(got_mean, x.reshape(-1, 32).mean(0),
                               rtol=1e-3, atol=1e-3)


def test_softmax_xent_vs_torch():
    rng = np.random.RandomState(3)
    logits = rng.randn(64, 100).astype(np.float32)
    labels = rng.randint(0, 100, 64).astype(np.int64)
    loss = tf.nn.sparse_softmax_cross_entropy_with_logits(
        labels=tf.constant(labels), logits=tf.constant(logits))
    got = _run(loss)
    want = torch.nn.functional.cross_entropy(
        torch.from_numpy(logits), torch.from_numpy(labels),
        reduction='none').numpy()
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)


def test_max_pool_grad_vs_torch():
    # bf16-exact values with a unique max per 2x2 window: coarse random
    # value per window (5 bits) + in-window position offset (3 frac bits)
    rng = np.random.RandomState(4)
    wr = rng.randint(0, 32, (2, 4, 4, 16)).astype(np.float32)
    x = np.zeros((2, 8, 8, 16), dtype=np.float32)
    for di in range(2):
        for dj in range(2):
            x[:, di::2, dj::2, :] = wr + (di * 2 + dj) * 0.125
    xt = tf.constant(x, dtype=tf.bfloat16)
    y = tf.nn.max_pool(xt, [1, 2, 2, 1], [1, 2, 2, 1], 'VALID')
    loss = tf.reduce_sum(tf.cast(y, tf.float32))
    g = tf.gradients(loss, [xt])[0]
    got = _run(g)
    tx = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    ty = torch.nn.functional.max_pool2d(tx, 2)
    ty.sum().backward()
    want = tx.grad.permute(0, 2, 3, 1).numpy()
    np.testing.assert_allclose(got, want, atol=1e-2)


def test_reduce_and_elementwise_vs_torch():
    rng = np.random.RandomState(5)
    x = rng.randn(1000, 33).astype(np.float32)
    got = _run([tf.reduce_sum(tf.constant(x), axis=0),
                tf.tanh(tf.constant(x[:5])),
                tf.sigmoid(tf.constant(x[:5]))])
    np.testing.assert_allclose(got[0], torch.from_numpy(x).sum(0).numpy(),
                               rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(got[1], np.tanh(x[:5]), rtol=1e-5,
                               atol=1e-5)
    np.testing.assert_allclose(got[2],
                               torch.sigmoid(torch.from_numpy(x[:5]))
                               .numpy(), rtol=1e-5, atol=1e-5)


def test_depthwise_conv_and_grads_vs_torch():
    rng = np.random.RandomState(6)
    x = rng.randn(2, 9, 9, 4).astype(np.float32)
    w = rng.randn(3, 3, 4, 1).astype(np.float32)
    xt = tf.constant(x, dtype=tf.bfloat16)
    wt = tf.constant(w, dtype=tf.bfloat16)
    y = tf.nn.depthwise_conv2d(xt, wt, [1, 1, 1, 1], 'SAME')
    loss = tf.reduce_sum(tf.cast(y, tf.float32))
    gx, gw = tf.gradients(loss, [xt, wt])
    got_y, got_gx, got_gw = _run([y, gx, gw])

    tx = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    twp = torch.from_numpy(w).permute(2, 3, 0, 1).reshape(4, 1, 3, 3) \
        .detach().requires_grad_(True)
    ty = torch.nn.functional.conv2d(tx, twp, padding=1, groups=4)
    ty.sum().backward()
    want_y = ty.detach().permute(0, 2, 3, 1).numpy()
    want_gx = tx.grad.permute(0, 2, 3, 1).numpy()
    want_gw = twp.grad.reshape(4, 1, 3, 3).permute(2, 3, 0, 1).numpy()
    scale = np.abs(want_y).max()
    assert np.abs(got_y - want_y).max() / scale < 0.05
    assert np.abs(got_gx - want_gx).max() / (np.abs(want_gx).max()) < 0.05
    assert np.abs(got_gw - want_gw).max() / (np.abs(want_gw).max()) < 0.05


def test_matmul_bf16_8phase_path_vs_torch():
    """Shapes eligible for the 256x256 8-phase GEMM (M,N mult of 256,
    K mult of 64) — exercises the fast template, not the 128x128 fallback.
    Non-square and transpose-detecting data (gemm_bf16_8ph.hip)."""
    rng = np.random.RandomState(7)
    for (m, n, k) in [(256, 256, 64), (512, 256, 128), (256, 512, 192),
                      (768, 512, 320), (512, 128, 256), (512, 64, 128),
                      (256, 576, 192), (256, 1152, 64)]:
        a = (rng.rand(m, k) * 2 - 1).astype(np.float32)
        b = (rng.rand(n, k) * 2 - 1).astype(np.float32)
        tf.reset_default_graph()
        got = _run(tf.matmul(tf.constant(a, dtype=tf.bfloat16),
                             tf.constant(b, dtype=tf.bfloat16),
                             transpose_b=True))
        want = (torch.from_numpy(a).bfloat16().float() @
                torch.from_numpy(b).bfloat16().float().T).numpy()
        rel = np.abs(got - want) / (np.abs(want) + 1e-2)
        assert np.percentile(rel, 99) < 0.05, (m, n, k)


def _torch_conv_ref(x, w, stride, padding):
    tx = torch.from_numpy(x).permute(0, 3, 1, 2)
    tw = torch.from_numpy(w).permute(3, 2, 0, 1)
    if padding == 'SAME':
        pad = (w.shape[0] - 1) // 2
    else:
        pad = 0
    return torch.nn.functional.conv2d(tx, tw, stride=stride, padding=pad)


def test_implicit_gemm_conv_vs_torch():
    """Shapes eligible for the implicit-GEMM conv paths (C%8==0, NPQ%256==0,
    Cout%64==0): fwd + backprop-input + backprop-filter vs torch autograd."""
    rng = np.random.RandomState(11)
    cases = [(4, 8, 16, 64, 1, 'SAME'), (4, 17, 8, 64, 2, 'VALID'),
             (1, 16, 32, 128, 1, 'SAME')]
    for (nb, hw, cin, cout, stride, padding) in cases:
        tf.reset_default_graph()
        x = (rng.randn(nb, hw, hw, cin) * 0.5).astype(np.float32)
        w = (rng.randn(3, 3, cin, cout) * 0.2).astype(np.float32)
        tx = torch.from_numpy(x).permute(0, 3, 1, 2).bfloat16().float() \
            .requires_grad_(True)
        tw = torch.from_numpy(w).permute(3, 2, 0, 1).bfloat16().float() \
            .requires_grad_(True)
        pad = 1 if padding == 'SAME' else 0
        ty = torch.nn.functional.conv2d(tx, tw, stride=stride, padding=pad)
        ty.backward(torch.ones_like(ty))
        with tf.Session() as s:
            xg = tf.constant(x, dtype=tf.bfloat16)
            wg = tf.constant(w, dtype=tf.bfloat16)
            y = tf.nn.conv2d(xg, wg, [1, stride, stride, 1], padding)
            gx, gw = tf.gradients(tf.reduce_sum(y), [xg, wg])
            got_y, got_gx, got_gw = s.run([y, gx, gw])
        want_y = ty.detach().permute(0, 2, 3, 1).numpy()
        want_gx = tx.grad.permute(0, 2, 3, 1).numpy()
        want_gw = tw.grad.permute(2, 3, 1, 0).numpy()
        scale = np.abs(want_y).max() + 1e-6
        assert got_y.shape == want_y.shape, (got_y.shape, want_y.shape)
        assert np.abs(got_y - want_y).max() / scale < 0.05, (cin, cout, stride)
        assert np.abs(got_gx - want_gx).max() / (np.abs(want_gx).max() + 1e-6) < 0.05
        assert np.abs(got_gw - want_gw).max() / (np.abs(want_gw).max() + 1e-6) < 0.05


def test_batch_matmul_bf16_vs_torch():
    rng = np.random.RandomState(13)
    a = (rng.rand(6, 48, 32) * 2 - 1).astype(np.float32)
    b = (rng.rand(6, 32, 40) * 2 - 1).astype(np.float32)
    got = _run(tf.batch_matmul(tf.constant(a, dtype=tf.bfloat16),
                               tf.constant(b, dtype=tf.bfloat16)))
    want = (torch.from_numpy(a).bfloat16().float() @
            torch.from_numpy(b).bfloat16().float()).numpy()
    rel = np.abs(got - want) / (np.abs(want) + 1e-2)
    assert np.percentile(rel, 99) < 0.05
    # adjoint flags
    got2 = _run(tf.batch_matmul(tf.constant(a, dtype=tf.bfloat16),
                                tf.constant(np.ascontiguousarray(
                                    b.transpose(0, 2, 1)),
                                    dtype=tf.bfloat16), adj_y=True))
    rel2 = np.abs(got2 - want) / (np.abs(want) + 1e-2)
    assert np.percentile(rel2, 99) < 0.05


def test_lrn_gpu_vs_torch():
    rng = np.random.RandomState(14)
    x = rng.randn(2, 5, 5, 16).astype(np.float32)
    t = tf.constant(x)
    y = tf.nn.lrn(t, depth_radius=2, bias=1.0, alpha=1e-3, beta=0.75)
    g = tf.gradients(tf.reduce_sum(y * y), [t])[0]
    got_y, got_g = _run([y, g])
    tx = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    # torch LRN: size = full window, alpha is summed-normalized
    size = 2 * 2 + 1
    ty = torch.nn.functional.local_response_norm(tx, size=size,
                                                 alpha=1e-3 * size, beta=0.75,
                                                 k=1.0)
    (ty * ty).sum().backward()
    want_y = ty.detach().permute(0, 2, 3, 1).numpy()
    want_g = tx.grad.permute(0, 2, 3, 1).numpy()
    np.testing.assert_allclose(got_y, want_y, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(got_g, want_g, rtol=1e-2, atol=1e-3)


def test_batch_norm_non_pow2_channels_vs_torch():
    # exercises the V9 fixed-window kernels with C=48 (Inception-style
    # non-power-of-two channel count) including the backward pass
    from simple_tensorflow_amd.python.framework.ops import apply_op
    rng = np.random.RandomState(9)
    C = 48
    x = rng.randn(8, 9, 9, C).astype(np.float32)
    scale = rng.rand(C).astype(np.float32) + 0.5
    offset = rng.randn(C).astype(np.float32)
    xt = tf.constant(x, dtype=tf.bfloat16)
    y, mean, var, _ = apply_op('BatchNormMi', xt, tf.constant(scale),
                               tf.constant(offset), epsilon=1e-4)
    # random-weighted loss: grad(sum(y^2)) wrt x cancels to ~0 under BN
    # (pure noise); a fixed random weighting stays well-conditioned
    wgt = rng.randn(8, 9, 9, C).astype(np.float32)
    loss = tf.reduce_sum(tf.cast(y, tf.float32) * tf.constant(wgt))
    gx = tf.gradients(loss, [xt])[0]
    got_y, got_mean, got_gx = _run([y, mean, gx])
    txt = torch.from_numpy(x).permute(0, 3, 1, 2).bfloat16().float()
    txt.requires_grad_(True)
    want = torch.nn.functional.batch_norm(
        txt, None, None, torch.from_numpy(scale), torch.from_numpy(offset),
        training=True, eps=1e-4)
    twgt = torch.from_numpy(wgt).permute(0, 3, 1, 2)
    tloss = (want * twgt).sum()
    tloss.backward()
    want_y = want.detach().permute(0, 2, 3, 1).numpy()
    assert np.abs(got_y - want_y).max() < 0.15
    np.testing.assert_allclose(got_mean, x.reshape(-1, C).mean(0),
                               rtol=1e-2, atol=1e-2)
    want_gx = txt.grad.permute(0, 2, 3, 1).numpy()
    denom = np.abs(want_gx) + 0.1
    assert np.percentile(np.abs(got_gx - want_gx) / denom, 99) < 0.15


def test_avg_pool_fwd_and_grad_vs_torch():
    rng = np.random.RandomState(10)
    x = rng.randn(4, 13, 13, 32).astype(np.float32)
    xt = tf.constant(x, dtype=tf.bfloat16)
    y = tf.nn.avg_pool(xt, [1, 3, 3, 1], [1, 1, 1, 1], 'SAME')
    dy = rng.randn(4, 13, 13, 32).astype(np.float32)
    g = tf.gradients(tf.reduce_sum(y * tf.constant(dy, dtype=tf.bfloat16)),
                     [xt])[0]
    got_y, got_g = _run([y, g])
    txt = torch.from_numpy(x).permute(0, 3, 1, 2).bfloat16().float()
    txt.requires_grad_(True)
    want = torch.nn.functional.avg_pool2d(txt, 3, 1, padding=1,
                                          count_include_pad=False)
    tdy = torch.from_numpy(dy).permute(0, 3, 1, 2).bfloat16().float()
    (want * tdy).sum().backward()
    want_y = want.detach().permute(0, 2, 3, 1).numpy()
    want_g = txt.grad.permute(0, 2, 3, 1).numpy()
    assert np.abs(got_y - want_y).max() < 0.05
    denom = np.abs(want_g) + 0.1
    assert np.percentile(np.abs(got_g - want_g) / denom, 99) < 0.1


# ---------------------------------------------------------------------------
# Batch norm and pooling: every dispatch path (dtype x C%8 x fuse_relu), odd
# row counts, and the multi-row V9 loop. Reference: CPU torch in f32 fed the
# same (bf16-rounded where the op is bf16) inputs.
# ---------------------------------------------------------------------------
def _round_bf16(a):
    return torch.from_numpy(a).bfloat16().float().numpy()


def _grad_close_bf16(got, want, bound=0.15):
    rel = np.abs(got - want) / (np.abs(want) + 0.1)
    assert np.percentile(rel, 99) < bound


def _bn_case(dtype, rows, C, fuse_relu, seed, with_side=False):
    """Runs BatchNormMi (or BatchNormAddReluMi) forward + backward on the
    GPU and in torch; returns (got, want) dicts of numpy arrays."""
    from simple_tensorflow_amd.python.framework.ops import apply_op
    rng = np.random.RandomState(seed)
    bf16 = dtype == tf.bfloat16
    rnd = _round_bf16 if bf16 else (lambda a: a)
    x = rnd(rng.randn(rows, C).astype(np.float32))
    side = rnd(rng.randn(rows, C).astype(np.float32))
    wgt = rnd(rng.randn(rows, C).astype(np.float32))
    scale = rng.rand(C).astype(np.float32) + 0.5
    offset = rng.randn(C).astype(np.float32)

    xt = tf.constant(x, dtype=dtype)
    st, ot = tf.constant(scale), tf.constant(offset)
    if with_side:
        sdt = tf.constant(side, dtype=dtype)
        y, mean, var, _ = apply_op('BatchNormAddReluMi', xt, st, ot, sdt,
                                   epsilon=1e-4)
        wrt = [xt, st, ot, sdt]
    else:
        y, mean, var, _ = apply_op('BatchNormMi', xt, st, ot, epsilon=1e-4,
                                   fuse_relu=fuse_relu)
        wrt = [xt, st, ot]
    # fixed random weighting: grad(sum(y)) wrt x cancels to ~0 under BN
    loss = tf.reduce_sum(tf.cast(y, tf.float32) * tf.constant(wgt))
    grads = tf.gradients(loss, wrt)
    out = _run([y, mean, var] + grads)
    names = ['y', 'mean', 'var', 'dx', 'dscale', 'doffset', 'dside']
    got = dict(zip(names, out))

    tx = torch.from_numpy(x).requires_grad_(True)
    ts = torch.from_numpy(scale).requires_grad_(True)
    to = torch.from_numpy(offset).requires_grad_(True)
    tsd = torch.from_numpy(side).requires_grad_(True)
    ty = torch.nn.functional.batch_norm(tx, None, None, ts, to,
                                        training=True, eps=1e-4)
    if with_side:
        ty = torch.relu(ty + tsd)
    elif fuse_relu:
        ty = torch.relu(ty)
    (ty * torch.from_numpy(wgt)).sum().backward()
    want = {'y': ty.detach().numpy(), 'mean': x.mean(0), 'var': x.var(0),
            'dx': tx.grad.numpy(), 'dscale': ts.grad.numpy(),
            'doffset': to.grad.numpy()}
    if with_side:
        want['dside'] = tsd.grad.numpy()
    return got, want


def _check_bn_bf16(got, want):
    for k in sorted(want):
        print(k, 'max abs err', np.abs(got[k] - want[k]).max())
    assert np.abs(got['y'] - want['y']).max() < 0.15
    np.testing.assert_allclose(got['mean'], want['mean'], rtol=1e-2,
                               atol=1e-2)
    np.testing.assert_allclose(got['var'], want['var'], rtol=1e-2, atol=1e-2)
    for k in sorted(set(want) - {'y', 'mean', 'var'}):
        _grad_close_bf16(got[k], want[k])


def _check_bn_f32(got, want):
    for k in sorted(want):
        print(k, 'max abs err', np.abs(got[k] - want[k]).max())
    for k in sorted(want):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-4, atol=1e-4,
                                   err_msg=k)


def test_bn_bf16_fuse_relu_odd_rows_vs_torch():
    # V9 kernels; 37 rows leave inactive threads in the last block
    _check_bn_bf16(*_bn_case(tf.bfloat16, 37, 16, True, seed=20))


def test_bn_add_relu_bf16_vs_torch():
    _check_bn_bf16(*_bn_case(tf.bfloat16, 37, 16, True, seed=21,
                             with_side=True))


@pytest.mark.parametrize('fuse_relu', [False, True])
def test_bn_bf16_scalar_path_vs_torch(fuse_relu):
    # C % 8 != 0 takes the scalar kernels
    _check_bn_bf16(*_bn_case(tf.bfloat16, 37, 12, fuse_relu, seed=22))


@pytest.mark.parametrize('fuse_relu', [False, True])
def test_bn_f32_c12_vs_torch(fuse_relu):
    _check_bn_f32(*_bn_case(tf.float32, 37, 12, fuse_relu, seed=23))


@pytest.mark.parametrize('fuse_relu', [False, True])
def test_bn_f32_c16_vs_torch(fuse_relu):
    # f32 with C % 8 == 0 must not take the 8-wide bf16 kernels
    _check_bn_f32(*_bn_case(tf.float32, 37, 16, fuse_relu, seed=24))


@pytest.mark.parametrize('fuse_relu', [False, True])
def test_bn_bf16_multi_row_loop_vs_torch(fuse_relu):
    # smallest row count with fewer row chunks (65536 at C=16) than rows:
    # some threads of the V9 kernels take two rows, the rest one
    _check_bn_bf16(*_bn_case(tf.bfloat16, 70001, 16, fuse_relu, seed=25))


def _pool_planes(C, seed):
    """x (2, 9, 9, C): every (n, c) plane is a permutation of 0..80 (exact
    in bf16, unique maximum in every window); dy small integers so sums of
    overlapping windows stay exact in bf16."""
    rng = np.random.RandomState(seed)
    x = np.stack([np.stack([rng.permutation(81).reshape(9, 9)
                            for _ in range(C)], axis=-1)
                  for _ in range(2)]).astype(np.float32)
    dy = rng.randint(-3, 4, (2, 5, 5, C)).astype(np.float32)
    return x, dy


@pytest.mark.parametrize('C', [8, 4])
def test_max_pool_3x3s2_same_vs_torch(C):
    # P = Q = 5, pad 1: clipped border windows and overlapping windows.
    # C=8: direct 8-wide gradient kernel; C=4: scalar kernel + f32 scratch.
    x, dy = _pool_planes(C, seed=26)
    xt = tf.constant(x, dtype=tf.bfloat16)
    y = tf.nn.max_pool(xt, [1, 3, 3, 1], [1, 2, 2, 1], 'SAME')
    loss = tf.reduce_sum(tf.cast(y, tf.float32) * tf.constant(dy))
    got_y, got_g = _run([y, tf.gradients(loss, [xt])[0]])
    tx = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    ty = torch.nn.functional.max_pool2d(tx, 3, 2, padding=1)
    (ty * torch.from_numpy(dy).permute(0, 3, 1, 2)).sum().backward()
    assert got_y.shape == (2, 5, 5, C)
    np.testing.assert_allclose(got_y, ty.detach().permute(0, 2, 3, 1).numpy(),
                               atol=1e-2)
    np.testing.assert_allclose(got_g, tx.grad.permute(0, 2, 3, 1).numpy(),
                               atol=1e-2)


@pytest.mark.parametrize('dtype,C', [('bfloat16', 8), ('bfloat16', 4),
                                     ('float32', 4)])
def test_avg_pool_3x3s2_same_vs_torch(dtype, C):
    bf16 = dtype == 'bfloat16'
    rnd = _round_bf16 if bf16 else (lambda a: a)
    rng = np.random.RandomState(27)
    x = rnd(rng.randn(2, 9, 9, C).astype(np.float32))
    dy = rnd(rng.randn(2, 5, 5, C).astype(np.float32))
    xt = tf.constant(x, dtype=getattr(tf, dtype))
    y = tf.nn.avg_pool(xt, [1, 3, 3, 1], [1, 2, 2, 1], 'SAME')
    loss = tf.reduce_sum(tf.cast(y, tf.float32) * tf.constant(dy))
    got_y, got_g = _run([y, tf.gradients(loss, [xt])[0]])
    tx = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    ty = torch.nn.functional.avg_pool2d(tx, 3, 2, padding=1,
                                        count_include_pad=False)
    (ty * torch.from_numpy(dy).permute(0, 3, 1, 2)).sum().backward()
    want_y = ty.detach().permute(0, 2, 3, 1).numpy()
    want_g = tx.grad.permute(0, 2, 3, 1).numpy()
    if bf16:
        assert np.abs(got_y - want_y).max() < 0.05
        _grad_close_bf16(got_g, want_g, bound=0.1)
    else:
        np.testing.assert_allclose(got_y, want_y, rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(got_g, want_g, rtol=1e-4, atol=1e-4)
