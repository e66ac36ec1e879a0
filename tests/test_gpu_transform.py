"""Pinning tests for the layout / reduce / embedding / optimizer / random HIP
kernels (csrc/kernels/hip/{layout,reduce,embedding,optimizer,random}.hip)
through the ops that launch them. Inputs go through placeholders so constant
folding cannot run an op on the CPU instead. All tests need a gfx950 GPU."""
import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.framework.ops import apply_op

from test_gpu_kernels import _bf16, _sess

pytestmark = pytest.mark.gpu

DTYPES = [tf.float32, tf.bfloat16]
DTYPE_IDS = ['f32', 'bf16']


@pytest.fixture(autouse=True)
def fresh_graph():
    tf.reset_default_graph()
    yield


def _data(rng, shape, dtype):
    """Random values exactly representable in `dtype`."""
    x = rng.randn(*shape).astype(np.float32)
    return _bf16(x) if dtype == tf.bfloat16 else x


def _feed(feeds, x, dtype):
    """Placeholder fed with x. bf16 goes in as f32 and is cast on the device
    (exact: x is already bf16-rounded); a fed bf16 array would reach the
    kernels tagged as uint16."""
    if dtype != tf.bfloat16:
        p = tf.placeholder(dtype, list(x.shape))
        feeds[p] = x
        return p
    p = tf.placeholder(tf.float32, list(x.shape))
    feeds[p] = x
    return tf.cast(p, tf.bfloat16)


# ---------------------------------------------------------------------------
# layout: data movement is bit-equal to numpy
# ---------------------------------------------------------------------------
def test_transpose2d_bf16_tile_edges():
    x = _data(np.random.RandomState(20), (65, 130), tf.bfloat16)
    feeds = {}
    with _sess() as s:
        out = s.run(tf.transpose(_feed(feeds, x, tf.bfloat16)), feeds)
    np.testing.assert_array_equal(out, x.T)


@pytest.mark.parametrize('shape,perm,dtype', [
    ((2, 3, 5, 7), (0, 3, 1, 2), tf.float32),
    ((2, 3, 5, 7), (0, 3, 1, 2), tf.bfloat16),
    ((2, 3, 2, 3, 2, 3), (5, 4, 3, 2, 1, 0), tf.float32),  # PermArgs' max rank
], ids=['rank4-f32', 'rank4-bf16', 'rank6-f32'])
def test_permute(shape, perm, dtype):
    x = _data(np.random.RandomState(21), shape, dtype)
    feeds = {}
    with _sess() as s:
        out = s.run(tf.transpose(_feed(feeds, x, dtype), list(perm)), feeds)
    np.testing.assert_array_equal(out, x.transpose(perm))


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_tile_broadcast(dtype):
    x = _data(np.random.RandomState(22), (1, 5, 1, 3), dtype)
    feeds = {}
    with _sess() as s:
        out = s.run(tf.tile(_feed(feeds, x, dtype), [4, 1, 2, 1]), feeds)
    np.testing.assert_array_equal(out, np.tile(x, (4, 1, 2, 1)))


@pytest.mark.parametrize('shapes,axis,dtype', [
    ([(3, 2, 5), (3, 4, 5), (3, 1, 5)], 1, tf.float32),
    ([(3, 5, 2), (3, 5, 4), (3, 5, 1)], -1, tf.bfloat16),
], ids=['f32-axis1', 'bf16-axis-1'])
def test_concat(shapes, axis, dtype):
    rng = np.random.RandomState(23)
    xs = [_data(rng, sh, dtype) for sh in shapes]
    feeds = {}
    with _sess() as s:
        out = s.run(tf.concat([_feed(feeds, x, dtype) for x in xs], axis),
                    feeds)
    np.testing.assert_array_equal(out, np.concatenate(xs, axis))


def test_split():
    x = _data(np.random.RandomState(24), (4, 6, 5), tf.float32)
    feeds = {}
    with _sess() as s:
        outs = s.run(tf.split(_feed(feeds, x, tf.float32), 3, axis=1), feeds)
    assert len(outs) == 3
    for out, ref in zip(outs, np.split(x, 3, axis=1)):
        np.testing.assert_array_equal(out, ref)


@pytest.mark.parametrize('axis', [0, 1])
def test_pack_unpack(axis):
    rng = np.random.RandomState(25)
    xs = [_data(rng, (3, 5), tf.float32) for _ in range(3)]
    feeds = {}
    with _sess() as s:
        packed = tf.stack([_feed(feeds, x, tf.float32) for x in xs], axis)
        res = s.run([packed] + tf.unstack(packed, num=3, axis=axis), feeds)
    np.testing.assert_array_equal(res[0], np.stack(xs, axis))
    for out, x in zip(res[1:], xs):
        np.testing.assert_array_equal(out, x)


def test_slice():
    x = _data(np.random.RandomState(26), (4, 9, 5), tf.float32)
    feeds = {}
    with _sess() as s:
        p = _feed(feeds, x, tf.float32)
        cut, full = s.run([tf.slice(p, [0, 2, 0], [-1, 4, -1]),
                           tf.slice(p, [0, 0, 0], [-1, -1, -1])], feeds)
    np.testing.assert_array_equal(cut, x[:, 2:6, :])
    np.testing.assert_array_equal(full, x)


# ---------------------------------------------------------------------------
# reductions
# ---------------------------------------------------------------------------
_REDUCERS = {
    'sum': (tf.reduce_sum, np.sum),
    'mean': (tf.reduce_mean, np.mean),
    'max': (tf.reduce_max, np.max),
    'min': (tf.reduce_min, np.min),
}

# (shape, axis, keep_dims): full reduce at one element and at more than one
# block (ElemwiseGrid(n, 256, 8) > 1 above 2048 elements); trailing axis with
# inner below a wave, below the block and above it; leading axis with more
# than one block of columns.
_REDUCE_CASES = [
    ((1,), None, False),
    ((4099,), None, False),
    ((3, 1), 1, False),
    ((3, 50), 1, False),
    ((3, 300), 1, False),
    ((7, 300), 0, False),
    ((3, 50), 1, True),
]


def _check_reduce(kind, dtype, out, ref64):
    if kind in ('max', 'min'):
        # inputs are exact in dtype, so the result is one of them
        np.testing.assert_array_equal(out, ref64.astype(np.float32))
    elif dtype == tf.bfloat16:
        np.testing.assert_allclose(out, _bf16(ref64), rtol=2e-2, atol=2e-2)
    else:
        np.testing.assert_allclose(out, ref64, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('kind', sorted(_REDUCERS))
def test_reduce(kind, dtype):
    tf_fn, np_fn = _REDUCERS[kind]
    rng = np.random.RandomState(27)
    feeds, fetches, refs = {}, [], []
    for shape, axis, keep in _REDUCE_CASES:
        x = _data(rng, shape, dtype)
        fetches.append(tf_fn(_feed(feeds, x, dtype), axis, keep_dims=keep))
        refs.append(np_fn(x.astype(np.float64), axis=axis, keepdims=keep))
    with _sess() as s:
        outs = s.run(fetches, feeds)
    for out, ref in zip(outs, refs):
        assert out.shape == ref.shape
        _check_reduce(kind, dtype, out, ref)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_reduce_identity_values(dtype):
    """Full Max of all-negative and full Min of all-positive data: a wrong
    identity (0 instead of -/+FLT_MAX) would win the multi-block combine."""
    x = np.abs(np.random.RandomState(28).randn(4099)).astype(np.float32) + 0.5
    if dtype == tf.bfloat16:
        x = _bf16(x)
    feeds = {}
    with _sess() as s:
        mx, mn = s.run([tf.reduce_max(_feed(feeds, -x, dtype)),
                        tf.reduce_min(_feed(feeds, x, dtype))], feeds)
    assert mx == (-x).max() and mx < 0
    assert mn == x.min() and mn > 0


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_l2_loss(dtype):
    rng = np.random.RandomState(29)
    feeds, fetches, refs = {}, [], []
    for n in (1, 4099):
        x = _data(rng, (n,), dtype)
        fetches.append(tf.nn.l2_loss(_feed(feeds, x, dtype)))
        refs.append(0.5 * np.sum(x.astype(np.float64) ** 2))
    with _sess() as s:
        outs = s.run(fetches, feeds)
    for out, ref in zip(outs, refs):
        _check_reduce('sum', dtype, out, np.float64(ref))


# ---------------------------------------------------------------------------
# gather / unsorted segment sum
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('itype', [tf.int32, tf.int64], ids=['i32', 'i64'])
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_gather_rows(dtype, itype):
    params = _data(np.random.RandomState(30), (11, 5), dtype)
    idx = np.array([3, 0, 10, 3, 7, 7, 1, 0, 10], itype.as_numpy_dtype)
    feeds = {}
    with _sess() as s:
        # the Gather op directly: tf.gather narrows int64 indices to int32
        out = s.run(apply_op('Gather', _feed(feeds, params, dtype),
                             _feed(feeds, idx, itype)), feeds)
    np.testing.assert_array_equal(out, params[idx])


@pytest.mark.parametrize('itype', [tf.int32, tf.int64], ids=['i32', 'i64'])
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_unsorted_segment_sum(dtype, itype):
    data = _data(np.random.RandomState(31), (9, 5), dtype)
    ids = np.array([0, 1, 2, 3, 0, 1, 2, 3, 2], itype.as_numpy_dtype)
    feeds = {}
    with _sess() as s:
        out = s.run(tf.unsorted_segment_sum(_feed(feeds, data, dtype),
                                            _feed(feeds, ids, itype), 4),
                    feeds)
    ref = np.zeros((4, 5), np.float64)
    np.add.at(ref, ids, data.astype(np.float64))
    if dtype == tf.bfloat16:
        np.testing.assert_allclose(out, _bf16(ref), rtol=2e-2, atol=2e-2)
    else:
        np.testing.assert_allclose(out, ref, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------
# optimizer applies: GPU kernel vs the CPU kernel on the same fed gradients
# ---------------------------------------------------------------------------
_OPTIMIZERS = {
    'sgd': lambda: tf.train.GradientDescentOptimizer(0.1),
    'momentum': lambda: tf.train.MomentumOptimizer(0.1, 0.9),
    'nesterov': lambda: tf.train.MomentumOptimizer(0.1, 0.9,
                                                   use_nesterov=True),
    'adam': lambda: tf.train.AdamOptimizer(0.01),
}


@pytest.mark.parametrize('grad_dtype', DTYPES, ids=['grad-f32', 'grad-bf16'])
@pytest.mark.parametrize('name', sorted(_OPTIMIZERS))
def test_optimizer_apply_vs_cpu(name, grad_dtype):
    """Two steps, so accumulators and Adam's beta powers matter. The bf16
    case feeds the GPU Apply* kernel a bf16 gradient for an f32 variable
    (nothing type-checks that edge, and the kernel has a bf16-grad
    instantiation for it); the CPU kernels only read f32, so the CPU side
    gets the same bf16-rounded values as f32."""
    n = 1027
    rng = np.random.RandomState(32)
    v0 = rng.randn(n).astype(np.float32)
    grads = [_data(rng, (n,), grad_dtype) for _ in range(2)]
    g = tf.placeholder(tf.float32, [n])
    g_gpu = tf.cast(g, tf.bfloat16) if grad_dtype == tf.bfloat16 else g
    var_gpu = tf.Variable(v0)
    train_gpu = _OPTIMIZERS[name]().apply_gradients([(g_gpu, var_gpu)])
    with tf.device('/cpu:0'):
        var_cpu = tf.Variable(v0)
        train_cpu = _OPTIMIZERS[name]().apply_gradients([(g, var_cpu)])
    with _sess() as s:
        s.run(tf.global_variables_initializer())
        for gv in grads:
            s.run([train_gpu, train_cpu], {g: gv})
            out, ref = s.run([var_gpu.value(), var_cpu.value()])
            print('%s %s max abs err %.3g' % (name, grad_dtype,
                                              np.abs(out - ref).max()))
            np.testing.assert_allclose(out, ref, rtol=1e-5, atol=1e-6)
    assert np.abs(ref - v0).max() > 1e-3  # the steps moved the variable


# ---------------------------------------------------------------------------
# random fills
# ---------------------------------------------------------------------------
def test_random_normal_moments():
    with _sess() as s:
        z = s.run(tf.random_normal([100000], seed=43))
    # standard errors 0.0032 (mean) and 0.0022 (std): about 6 sigma
    assert abs(z.mean()) < 0.02
    assert abs(z.std() - 1.0) < 0.02


def test_truncated_normal_moments():
    with _sess() as s:
        z = s.run(tf.truncated_normal([100000], seed=44))
    assert np.abs(z).max() < 2.0
    assert abs(z.std() - 0.8796) < 0.02


def test_random_uniform_tail_and_range():
    """1001 is not a multiple of the 4 values one Philox draw gives."""
    with _sess() as s:
        u32 = s.run(tf.random_uniform([1001], seed=45))
        u16 = s.run(tf.random_uniform([1001], dtype=tf.bfloat16, seed=46))
    assert u32.shape == (1001,) and u16.shape == (1001,)
    assert 0.0 <= u32.min() and u32.max() < 1.0
    # the bf16 cast may round up to exactly 1.0
    assert 0.0 <= u16.min() and u16.max() <= 1.0
    assert u32.std() > 0.2 and u16.std() > 0.2  # filled, tail included
    assert u32[-1] != 0.0 or u32[-2] != 0.0


@pytest.mark.parametrize('fn', [tf.random_uniform, tf.random_normal,
                                tf.truncated_normal],
                         ids=['uniform', 'normal', 'truncated'])
def test_random_counter_advances(fn):
    """Two runs of one op draw different numbers (device-side counter)."""
    with _sess() as s:
        op = fn([1001], seed=47)
        a = s.run(op)
        b = s.run(op)
    assert not np.array_equal(a, b)


# ---------------------------------------------------------------------------
# placement: the ops above really run on the GPU
# ---------------------------------------------------------------------------
def test_transform_ops_run_on_gpu():
    rng = np.random.RandomState(48)
    feeds = {}
    x = _feed(feeds, _data(rng, (4, 6, 5), tf.float32), tf.float32)
    idx = _feed(feeds, np.array([1, 0, 3, 1], np.int32), tf.int32)
    fetches = [
        tf.transpose(x, [2, 0, 1], name='t_permute'),
        tf.tile(tf.reshape(x, [1, 120]), [3, 1], name='t_tile'),
        tf.concat([x, x], 1, name='t_concat'),
        tf.slice(x, [0, 1, 0], [-1, 2, -1], name='t_slice'),
        tf.stack([x, x], name='t_pack'),
        tf.reduce_min(x, 0, name='t_min'),
        tf.nn.l2_loss(x, name='t_l2'),
        apply_op('Gather', x, idx, name='t_gather'),
        tf.unsorted_segment_sum(x, idx, 4, name='t_segsum'),
        tf.random_normal([64], seed=49, name='t_normal'),
    ]
    fetches += tf.split(x, 3, axis=1, name='t_split')
    fetches += tf.unstack(x, num=4, name='t_unpack')
    opts = tf.RunOptions(trace_level=tf.RunOptions.FULL_TRACE)
    md = tf.RunMetadata()
    with _sess() as s:
        s.run(fetches, feeds, options=opts, run_metadata=md)
    on_gpu = {ns.node_name for ds in md.step_stats.dev_stats
              if 'GPU' in ds.device.upper() for ns in ds.node_stats}
    for name in ('t_permute', 't_tile', 't_concat', 't_slice', 't_pack',
                 't_min', 't_l2', 't_gather', 't_segsum', 't_normal',
                 't_split', 't_unpack'):
        assert name in on_gpu, (name, sorted(on_gpu))
