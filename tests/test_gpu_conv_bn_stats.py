"""Batch-norm statistics out of the conv GEMM epilogue.

Op level: _Conv2DBnStats against Conv2D on the same inputs. y must be
bit-equal (same kernel and math, no split-K in the forward); sums is compared
with float64 column sums of that bf16 y. Per column, with n rows,
|d sum| <= n * 2^-24 * sum|y| and |d sumsq| <= n * 2^-24 * sum(y^2): the
worst case of f32 summation in any order (the addends themselves are exact:
a bf16 value, and the square of one, which has 16 significant bits).

Graph level: conv -> BatchNormMi(fuse_relu) / BatchNormAddReluMi with
gradients, built once with the FuseConvBnStats pass and once with
STF_NO_CONV_BN_STATS set. mean and var may differ by the summation bound
divided by n; y and the gradients are held to the bounds test_gpu_vs_torch.py
and test_gpu_bn_dside.py put on bf16 batch norm."""
import os

import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.framework.ops import apply_op

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # f32 unit roundoff


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


def _inputs(xs, ws, seed):
    """bf16-exact x, and w with a different offset per output channel, so
    that columns and row tiles have clearly different sums."""
    rng = np.random.RandomState(seed)
    x = _bf16(rng.randn(*xs) + 0.5)
    k = ws[3]
    fan_in = ws[0] * ws[1] * ws[2]
    off = np.linspace(-1.0, 1.0, k) / fan_in
    w = _bf16(rng.randn(*ws) / np.sqrt(fan_in) + off)
    return x, w


# (x shape, w shape, stride, what it reaches)
OP_CASES = [
    ((1, 16, 16, 64), (1, 1, 64, 64), 1, 'NR=1, one tile'),
    ((2, 16, 16, 64), (1, 1, 64, 192), 1, 'NR=1, 3 column x 2 row tiles'),
    ((2, 16, 16, 64), (1, 1, 64, 384), 1, 'NR=2, 3 column tiles'),
    ((2, 16, 16, 64), (1, 1, 64, 512), 1, 'NR=4, 2 column tiles'),
    ((1, 16, 16, 64), (3, 3, 64, 64), 1, 'ConvAG, K=576'),
    ((1, 32, 32, 64), (1, 1, 64, 128), 2, 'strided implicit'),
    ((1, 32, 32, 3), (7, 7, 3, 64), 2, 'stem: channel pad, RSC pad'),
    ((1, 10, 10, 16), (1, 1, 16, 24), 1, 'fallback, V9 stats'),
    ((1, 10, 10, 16), (1, 1, 16, 20), 1, 'fallback, scalar stats'),
    ((4, 64, 64, 64), (1, 1, 64, 64), 1, '64 row tiles: row split'),
]


@pytest.mark.parametrize('xs,ws,stride,what', OP_CASES,
                         ids=[c[3] for c in OP_CASES])
def test_conv2d_bn_stats_op(xs, ws, stride, what):
    xv, wv = _inputs(xs, ws, seed=ws[3])
    x = tf.constant(xv, dtype=tf.bfloat16)
    w = tf.constant(wv, dtype=tf.bfloat16)
    strides = [1, stride, stride, 1]
    ref = tf.nn.conv2d(x, w, strides, 'SAME')
    y, sums = apply_op('_Conv2DBnStats', x, w, strides=strides,
                       padding='SAME')
    with _sess() as s:
        got_y, got_sums, want_y = s.run(
            [tf.cast(y, tf.float32), sums, tf.cast(ref, tf.float32)])

    k = ws[3]
    assert got_y.shape == want_y.shape and got_y.shape[3] == k
    np.testing.assert_array_equal(got_y.view(np.uint32),
                                  want_y.view(np.uint32))
    assert got_sums.shape == (2 * k,)

    y64 = want_y.astype(np.float64).reshape(-1, k)
    n = y64.shape[0]
    want_sum, want_sq = y64.sum(0), (y64 * y64).sum(0)
    # the columns really differ, so a mis-indexed window would show
    assert np.ptp(want_sum) > 0.05 * np.abs(want_sum).max()
    err_sum = np.abs(got_sums[:k] - want_sum)
    err_sq = np.abs(got_sums[k:] - want_sq)
    bound_sum = n * U * np.abs(y64).sum(0)
    bound_sq = n * U * want_sq
    print('%s: n=%d  sum err/bound max %.3g  sumsq err/bound max %.3g'
          % (what, n, (err_sum / bound_sum).max(),
             (err_sq / bound_sq).max()))
    assert (err_sum <= bound_sum).all()
    assert (err_sq <= bound_sq).all()


# ---------------------------------------------------------------------------
# graph level
# ---------------------------------------------------------------------------
def _grad_close_bf16(got, want, bound=0.15):
    # the bound test_gpu_vs_torch.py puts on the bf16 BN gradients
    rel = np.abs(got - want) / (np.abs(want) + 0.1)
    assert np.percentile(rel, 99) < bound


def _with_env(name, fn):
    """fn() in a fresh graph with the switch `name` set."""
    os.environ[name] = '1'
    try:
        tf.reset_default_graph()
        return fn()
    finally:
        del os.environ[name]


def _graph_run(xs, ws, with_side, fetch_conv_node=False):
    """conv -> BN (+ side) -> weighted loss with gradients. Returns the
    fetched values by name and the op types that ran."""
    xv, wv = _inputs(xs, ws, seed=5)
    k = ws[3]
    rng = np.random.RandomState(6)
    ys = xs[:3] + (k,)
    scale = (rng.rand(k) + 0.5).astype(np.float32)
    offset = (rng.randn(k) * 0.5).astype(np.float32)
    side = _bf16(rng.randn(*ys))
    wgt = rng.randn(*ys).astype(np.float32)

    x = tf.constant(xv, dtype=tf.bfloat16)
    w = tf.constant(wv, dtype=tf.bfloat16)
    st, ot = tf.constant(scale), tf.constant(offset)
    conv = tf.nn.conv2d(x, w, [1, 1, 1, 1], 'SAME')
    if with_side:
        y, mean, var, _ = apply_op('BatchNormAddReluMi', conv, st, ot,
                                   tf.constant(side, dtype=tf.bfloat16),
                                   epsilon=1e-4)
    else:
        y, mean, var, _ = apply_op('BatchNormMi', conv, st, ot, epsilon=1e-4,
                                   fuse_relu=True)
    loss = tf.reduce_sum(tf.cast(y, tf.float32) * tf.constant(wgt))
    gx, gw, gs, go = tf.gradients(loss, [x, w, st, ot])
    # A fetched node is preserved by the optimizer, so everything that comes
    # out of the two nodes under test is fetched through another node.
    fetches = {'y': tf.cast(y, tf.float32), 'mean': tf.identity(mean),
               'var': tf.identity(var),
               'gx': tf.cast(gx, tf.float32), 'gw': tf.cast(gw, tf.float32),
               'gscale': gs, 'goffset': go,
               # the conv node itself (then it is preserved and stays a
               # Conv2D), or its value through a Cast (then it may be fused)
               'conv': conv if fetch_conv_node else tf.cast(conv, tf.float32)}
    names = sorted(fetches)
    opts = tf.RunOptions(trace_level=tf.RunOptions.FULL_TRACE)
    md = tf.RunMetadata()
    with _sess() as s:
        vals = s.run([fetches[n] for n in names], options=opts,
                     run_metadata=md)
    ops = {ns.op for ds in md.step_stats.dev_stats for ns in ds.node_stats}
    out = dict(zip(names, vals))
    out['conv'] = np.asarray(out['conv'], np.float32)
    return out, ops


@pytest.mark.parametrize('with_side', [False, True],
                         ids=['bn_relu', 'bn_add_relu'])
@pytest.mark.parametrize('xs,ws', [((2, 16, 16, 64), (1, 1, 64, 64)),
                                   ((1, 16, 16, 64), (3, 3, 64, 64))],
                         ids=['1x1', '3x3'])
def test_conv_bn_stats_graph(xs, ws, with_side):
    bn = 'BatchNormAddReluMi' if with_side else 'BatchNormMi'
    on, on_ops = _graph_run(xs, ws, with_side)
    assert '_Conv2DBnStats' in on_ops and '_%sStats' % bn in on_ops
    assert 'Conv2D' not in on_ops and bn not in on_ops

    off, off_ops = _with_env('STF_NO_CONV_BN_STATS',
                             lambda: _graph_run(xs, ws, with_side))
    assert 'Conv2D' in off_ops and bn in off_ops
    assert not any(o.endswith('Stats') for o in off_ops)

    # a fetched conv node is preserved: no rewrite, the right value
    kept, kept_ops = _graph_run(xs, ws, with_side, fetch_conv_node=True)
    assert 'Conv2D' in kept_ops and bn in kept_ops

    np.testing.assert_array_equal(on['conv'], off['conv'])
    np.testing.assert_array_equal(kept['conv'], off['conv'])
    assert np.abs(kept['y'] - off['y']).max() < 0.15

    y64 = off['conv'].astype(np.float64).reshape(-1, ws[3])
    bound_mean = U * np.abs(y64).sum(0)
    bound_var = U * (y64 * y64).sum(0)
    for key in sorted(off):
        print(key, 'max abs diff on/off', np.abs(on[key] - off[key]).max())
    assert (np.abs(on['mean'] - off['mean']) <= bound_mean).all()
    assert (np.abs(on['var'] - off['var']) <= bound_var).all()
    assert np.abs(on['y'] - off['y']).max() < 0.15
    for key in ('gx', 'gw', 'gscale', 'goffset'):
        _grad_close_bf16(on[key], off[key])
    # and the statistics are those of the conv output. n <= 512 rows: an f32
    # sum is off by at most n * 2^-24 = 3e-5 of sum|y|, and var = E[y^2] -
    # mean^2 loses little more here, where mean^2 is below the variance.
    np.testing.assert_allclose(on['mean'], y64.mean(0), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(on['var'], y64.var(0), rtol=1e-3, atol=1e-5)
