"""BatchNormMiGrad(fuse_relu) without its y_relu read: the RecomputeBnReluMask
pass and the _BatchNormMiGradRecompute kernels.

The kernels form bf16(relu(bn(x))) again and test it <= 0, through the same
device function the forward kernel calls. What can go wrong is one element
whose recomputed value lands on the other side of zero than the stored one.

Mask identity: dy holds integers in +-{1, 2, 3}, so doffset = sum of the
masked dy is a sum of small integers, exact in f32 in any order of the
atomics. One mask mismatch moves it by a non-zero integer: doffset must be
bit-equal to the sum of dy over the y > 0 that the same run's forward stored,
and to the unfused graph's doffset wherever the two runs stored the same mask
(the forward's f32 atomics make mean and inv_std differ in the last bit from
run to run, and with them a few y).

Exact data: with mean 0, inv_std 1, scale a power of two, integer offset, x in
eighths and integer dy, every product and sum of the backward is exact in
f32, so the new op is bit-equal to BatchNormMiGrad and to numpy."""
import os

import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.framework.ops import apply_op
from test_gpu_bn_dside import _bf16, _grad_close_bf16, _reference

pytestmark = pytest.mark.gpu

OFF_SWITCH = 'STF_NO_BN_RELU_RECOMPUTE'
NEW_OP = '_BatchNormMiGradRecompute'
OLD_OP = 'BatchNormMiGrad'


@pytest.fixture(autouse=True)
def fresh_graph():
    tf.reset_default_graph()
    yield


def _sess():
    s = tf.Session()
    assert s.num_gpus() > 0
    return s


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _without_pass(fn):
    """fn() in a fresh graph with the pass switched off."""
    os.environ[OFF_SWITCH] = '1'
    try:
        tf.reset_default_graph()
        return fn()
    finally:
        del os.environ[OFF_SWITCH]


def _run_traced(fetches):
    """Runs the dict of fetches; returns values by name and the op types
    that ran."""
    names = sorted(fetches)
    opts = tf.RunOptions(trace_level=tf.RunOptions.FULL_TRACE)
    md = tf.RunMetadata()
    with _sess() as s:
        vals = s.run([fetches[n] for n in names], options=opts,
                     run_metadata=md)
    ops = {ns.op for ds in md.step_stats.dev_stats for ns in ds.node_stats}
    return dict(zip(names, vals)), ops


# ---------------------------------------------------------------------------
# mask identity through the real forward
# ---------------------------------------------------------------------------
# channels 0..6 are adversarial, the rest ordinary
ZERO_SCALE = {0: 0.0, 1: -0.0, 2: float(np.float32(1e-45))}  # ch -> offset
CONST_CH, NAN_CH, INF_CH = 3, 4, 5
FINITE = [c for c in range(12) if c not in (NAN_CH, INF_CH)]


def _forward_inputs(rows, C, bf16):
    rng = np.random.RandomState(rows + C)
    x = rng.randn(rows, C).astype(np.float32) * 1.5 + 0.25
    scale = (rng.rand(C) + 0.5).astype(np.float32)
    scale[6] = -scale[6]           # a negative scale: the mask flips with x
    offset = (rng.randn(C) * 0.5).astype(np.float32)
    for ch, off in ZERO_SCALE.items():
        scale[ch] = 0.0
        offset[ch] = off
    assert np.signbit(offset[1]) and offset[2] > 0
    x[:, CONST_CH] = 0.7109375     # exact in bf16
    x[rows // 2, NAN_CH] = np.nan
    x[rows // 3, INF_CH] = np.inf
    if bf16:
        x = _bf16(x)
    wgt = rng.choice([-3, -2, -1, 1, 2, 3], (rows, C)).astype(np.float32)
    return x, scale, offset, wgt


def _forward_graph(rows, C, bf16):
    xv, scale, offset, wgt = _forward_inputs(rows, C, bf16)
    dt = tf.bfloat16 if bf16 else tf.float32
    x = tf.constant(xv, dtype=dt)
    st, ot = tf.constant(scale), tf.constant(offset)
    y, mean, _, inv_std = apply_op('BatchNormMi', x, st, ot, epsilon=1e-4,
                                   fuse_relu=True)
    loss = tf.reduce_sum(tf.cast(y, tf.float32) * tf.constant(wgt))
    gx, gs, go = tf.gradients(loss, [x, st, ot])
    # a fetched node is preserved by the optimizer, so everything that comes
    # out of the two nodes under test is fetched through another node (a
    # Cast for bf16; an f32 -> f32 cast would be the tensor itself)
    via = (lambda t: tf.cast(t, tf.float32)) if bf16 else tf.identity
    return _run_traced({
        'y': via(y), 'mean': tf.identity(mean),
        'inv_std': tf.identity(inv_std), 'dx': via(gx),
        'dscale': tf.identity(gs), 'doffset': tf.identity(go)})


@pytest.mark.parametrize('rows,C,bf16', [
    (35, 24, True),     # 8-wide kernels: 3 channel windows, idle tail threads
    (1000, 16, True),   # 8-wide kernels: several blocks
    (4096, 64, True),   # 8-wide kernels: every thread strides over rows
    (35, 12, True),     # C % 8 != 0: scalar bf16 kernels
    (35, 12, False),    # f32: scalar kernels
], ids=['bf16-35x24', 'bf16-1000x16', 'bf16-4096x64', 'bf16-35x12',
        'f32-35x12'])
def test_mask_identity_through_forward(rows, C, bf16):
    on, on_ops = _forward_graph(rows, C, bf16)
    assert NEW_OP in on_ops and OLD_OP not in on_ops
    off, off_ops = _without_pass(lambda: _forward_graph(rows, C, bf16))
    assert OLD_OP in off_ops and NEW_OP not in off_ops

    xv, scale, _, wgt = _forward_inputs(rows, C, bf16)
    kept = (on['y'] > 0).sum(0)
    print('kept per channel', kept[:12], 'of', rows)
    assert (kept[[0, 1, NAN_CH]] == 0).all()
    assert 0 < kept[7] < rows

    # Each run against the y its own forward stored: doffset is the integer
    # sum of dy over y > 0, so one element on the wrong side of zero shows.
    for name, run in (('fused', on), ('unfused', off)):
        want = np.where(run['y'] > 0, wgt, 0).astype(np.float64).sum(0)
        np.testing.assert_array_equal(
            _bits(run['doffset']), _bits(want.astype(np.float32)),
            err_msg=name + ' doffset vs the mask of its own y')
    # Run against run. The forward statistics are summed with f32 atomics, so
    # two runs may differ in the last bit of mean and inv_std and then in a
    # few y; a channel is compared where the two runs stored the same mask.
    same_mask = ((on['y'] > 0) == (off['y'] > 0)).all(0)
    print('channels with the same mask in both runs:', same_mask.sum(), 'of',
          C, '; y words that differ:', (_bits(on['y']) != _bits(off['y'])).sum())
    assert same_mask.sum() >= C - 2
    np.testing.assert_array_equal(_bits(on['doffset'])[same_mask],
                                  _bits(off['doffset'])[same_mask])

    fin = FINITE + list(range(12, C))
    want_dx, want_dscale, _ = _reference(
        xv[:, fin], wgt[:, fin], on['y'][:, fin], scale[fin],
        on['mean'][fin], on['inv_std'][fin])
    for name, got, want in (('dx', on['dx'][:, fin], want_dx),
                            ('dscale', on['dscale'][fin], want_dscale)):
        print(name, 'max abs err', np.abs(got - want).max())
        _grad_close_bf16(got, want)


# ---------------------------------------------------------------------------
# bit-equality on exact data, op called directly
# ---------------------------------------------------------------------------
def _exact_inputs(rows, C, seed):
    """mean 0, inv_std 1, scale in {0.5, 1, 2}, offset in -2..2, x in eighths
    within +-4, dy integers within +-3: |x * scale + offset| <= 10 in
    sixteenths is exact in bf16, and all of the backward is exact in f32."""
    rng = np.random.RandomState(seed)
    x = rng.randint(-32, 33, (rows, C)).astype(np.float32) / 8
    dy = rng.randint(-3, 4, (rows, C)).astype(np.float32)
    scale = rng.choice([0.5, 1.0, 2.0], C).astype(np.float32)
    offset = rng.randint(-2, 3, C).astype(np.float32)
    return x, dy, scale, offset


def _exact_backward(x, g, scale, bf16):
    """The backward formula with mean 0 and inv_std 1 on the masked gradient
    g; float64 holds every intermediate exactly."""
    rows = x.shape[0]
    g, x = g.astype(np.float64), x.astype(np.float64)
    doffset = g.sum(0)
    dscale = (g * x).sum(0)
    dx = (scale * (g - doffset / rows - x * dscale / rows)).astype(np.float32)
    return (_bf16(dx) if bf16 else dx, dscale.astype(np.float32),
            doffset.astype(np.float32))


@pytest.mark.parametrize('rows', [64, 1024])
@pytest.mark.parametrize('C,bf16', [(24, True), (12, True), (12, False)],
                         ids=['bf16-c24', 'bf16-c12', 'f32-c12'])
def test_recompute_op_bit_equal_on_exact_data(rows, C, bf16):
    x, dy, scale, offset = _exact_inputs(rows, C, seed=rows + C)
    y = np.maximum(x * scale + offset, np.float32(0.0))
    if bf16:
        np.testing.assert_array_equal(y, _bf16(y))   # exact, as claimed
    dt = tf.bfloat16 if bf16 else tf.float32
    tdy, tx = tf.constant(dy, dtype=dt), tf.constant(x, dtype=dt)
    ts, to = tf.constant(scale), tf.constant(offset)
    tm = tf.constant(np.zeros(C, np.float32))
    ti = tf.constant(np.ones(C, np.float32))
    new = apply_op(NEW_OP, tdy, tx, ts, to, tm, ti, epsilon=1e-4)
    old = apply_op(OLD_OP, tdy, tx, ts, tm, ti, tf.constant(y, dtype=dt),
                   epsilon=1e-4, fuse_relu=True)
    assert len(new) == 3 and len(old) == 3
    with _sess() as s:
        got = s.run([tf.cast(new[0], tf.float32), new[1], new[2],
                     tf.cast(old[0], tf.float32), old[1], old[2]])
    want = _exact_backward(x, np.where(y > 0, dy, np.float32(0.0)), scale,
                           bf16)
    assert 0.2 < (y > 0).mean() < 0.8
    for i, name in enumerate(('dx', 'dscale', 'doffset')):
        np.testing.assert_array_equal(_bits(got[i]), _bits(got[3 + i]),
                                      err_msg=name + ' new op vs old op')
        np.testing.assert_array_equal(_bits(got[i]), _bits(want[i]),
                                      err_msg=name + ' new op vs numpy')


# ---------------------------------------------------------------------------
# the gate
# ---------------------------------------------------------------------------
def _gate_graph(how):
    rows, C = 35, 12
    rng = np.random.RandomState(7)
    xv = rng.randn(rows, C).astype(np.float32)
    x = tf.constant(xv)
    st = tf.constant((rng.rand(C) + 0.5).astype(np.float32))
    ot = tf.constant((rng.randn(C) * 0.5).astype(np.float32))
    dy = tf.constant(rng.randn(rows, C).astype(np.float32))
    y, mean, _, inv_std = apply_op('BatchNormMi', x, st, ot, epsilon=1e-4,
                                   fuse_relu=True)
    feed = {}
    if how == 'fed_y':
        y = tf.placeholder(tf.float32, [rows, C])
        feed[y] = np.maximum(xv, 0)
    if how == 'foreign_mean':
        mean = mean + tf.constant(np.zeros(C, np.float32))
    dx, ds, do = apply_op(OLD_OP, dy, x, st, mean, inv_std, y, epsilon=1e-4,
                          fuse_relu=True)
    # fetched by name: the node is preserved
    fetches = [dx, ds, do] if how == 'fetched' else \
        [tf.identity(dx), tf.identity(ds), tf.identity(do)]
    opts = tf.RunOptions(trace_level=tf.RunOptions.FULL_TRACE)
    md = tf.RunMetadata()
    with _sess() as s:
        s.run(fetches, feed_dict=feed, options=opts, run_metadata=md)
    return {ns.op for ds_ in md.step_stats.dev_stats
            for ns in ds_.node_stats}


@pytest.mark.parametrize('how', ['fed_y', 'foreign_mean', 'fetched'])
def test_gate_keeps_the_op(how):
    ops = _gate_graph(how)
    assert OLD_OP in ops and NEW_OP not in ops


def test_gate_control_case_is_rewritten():
    # the same graph with none of the three obstacles
    ops = _gate_graph('plain')
    assert NEW_OP in ops and OLD_OP not in ops
