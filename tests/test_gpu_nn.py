"""Pinning tests for the loss, pool, LSTM, LRN and depthwise HIP kernels
(csrc/kernels/hip/{loss,pool,lstm,lrn,depthwise}.hip) through the ops that
launch them. Every input goes through a placeholder so constant folding
cannot run an op on the CPU, and every checked output is a fetched op.
References are plain numpy in float64 on the bf16-exact inputs. All tests
need a gfx950 GPU.

The bounds, each checked on every element:
  exact          max pool forward and every max-pool gradient, and the zeros
                 any gradient kernel writes: inputs are exact in the dtype
                 and dy is small integers, so overlapping sums stay exact
  f32 transc.    rtol 1e-4, atol 1e-5 (softmax, log-softmax, xent loss and
                 backprop, LSTM, LRN): test_softmax_gpu / test_sparse_xent_gpu
  f32 arith.     rtol 1e-5, atol 1e-6 (avg pool, bias add): F32_TOL of
                 test_gpu_elementwise
  f32 col. sums  rtol 1e-4, atol 1e-3 (BiasAddGrad, f32 atomics in any
                 order): _check_reduce of test_gpu_transform
  bf16           one rounding of the f32 result into 8 significant bits:
                 rtol 2^-8 + <the op's f32 rtol>, the op's f32 atol
  bf16 sums      BiasAddGrad: _check_reduce's bf16 bound. Depthwise: rtol
                 2^-8 + 1e-4 against the float64 sum, atol 2^-8 times the
                 float64 sum of the absolute values of the element's terms

Left open on purpose, not tested here:
  - what max pool returns for NaN inputs;
  - what max pool returns for a window holding only -inf (the kernels start
    from -3.4e38, not -inf);
  - data_format='NCHW': no kernel in the project, CPU or GPU, reads the
    attribute."""
import collections

import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.framework.ops import apply_op

from test_gpu_kernels import _bf16, _sess
from test_window_geom import reject_list, rejected_op, window_op

pytestmark = pytest.mark.gpu

DTYPES = [tf.float32, tf.bfloat16]
DTYPE_IDS = ['f32', 'bf16']
ITYPES = [tf.int32, tf.int64]
ITYPE_IDS = ['i32', 'i64']

TRANSC_TOL = dict(rtol=1e-4, atol=1e-5)
ARITH_TOL = dict(rtol=1e-5, atol=1e-6)
# ElemwiseGrid caps the grid at 2048 blocks of 256 threads: a kernel with
# more elements than this (at unroll 1) takes a second grid-stride pass
GRID_CAP = 2048 * 256


@pytest.fixture(scope='module')
def sess():
    """One graph and one session for the whole module: opening a session
    costs more than any case here. Every test only adds nodes."""
    tf.reset_default_graph()
    with _sess() as s:
        yield s


def _rnd(x, dtype):
    """x as float32, exactly representable in `dtype`."""
    x = np.asarray(x, np.float32)
    return _bf16(x) if dtype == tf.bfloat16 else x


def _feed(feeds, x, dtype):
    """Placeholder fed with x. bf16 goes in as f32 and is cast on the device
    (exact: x is already bf16-rounded); a fed bf16 array would reach the
    kernels tagged as uint16."""
    x = np.asarray(x)
    if dtype != tf.bfloat16:
        p = tf.placeholder(dtype, list(x.shape))
        feeds[p] = x
        return p
    p = tf.placeholder(tf.float32, list(x.shape))
    feeds[p] = x
    return tf.cast(p, tf.bfloat16)


def _tol(dtype, f32_tol):
    if dtype != tf.bfloat16:
        return f32_tol
    return dict(rtol=2.0 ** -8 + f32_tol['rtol'], atol=f32_tol['atol'])


def _close(label, out, ref, tol):
    ref = np.asarray(ref, np.float64)
    out = np.asarray(out)
    assert out.shape == ref.shape, (label, out.shape, ref.shape)
    fin = np.isfinite(ref)
    if fin.any():
        err = np.abs(out[fin].astype(np.float64) - ref[fin])
        print('%s: max abs err %.3g, max err/bound %.3g' % (
            label, err.max(),
            (err / (tol['atol'] + tol['rtol'] * np.abs(ref[fin]))).max()))
    np.testing.assert_allclose(out, ref, err_msg=label, **tol)


def _exact(label, out, ref):
    ref = np.asarray(ref)
    assert out.shape == ref.shape, (label, out.shape, ref.shape)
    np.testing.assert_array_equal(out, ref.astype(np.float32), err_msg=label)


def _trace_run(sess, fetches, feeds):
    """Outputs, and the names of the nodes that ran on a GPU."""
    opts = tf.RunOptions(trace_level=tf.RunOptions.FULL_TRACE)
    md = tf.RunMetadata()
    outs = sess.run(fetches, feeds, options=opts, run_metadata=md)
    on_gpu = {ns.node_name for ds in md.step_stats.dev_stats
              if 'GPU' in ds.device.upper() for ns in ds.node_stats}
    return outs, on_gpu


# ---------------------------------------------------------------------------
# softmax, log-softmax
# ---------------------------------------------------------------------------
def _log_softmax64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid='ignore'):
        z = x - x.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def _softmax64(x):
    return np.exp(_log_softmax64(x))


SOFTMAX_COLS = (1, 5, 63, 64, 65, 256, 257, 1000, 10000)
_SOFTMAX_KINDS = [('Softmax', tf.float32), ('Softmax', tf.bfloat16),
                  ('LogSoftmax', tf.float32)]


@pytest.mark.parametrize('op,dtype', _SOFTMAX_KINDS,
                         ids=['softmax-f32', 'softmax-bf16', 'logsoftmax-f32'])
def test_softmax(sess, op, dtype):
    """cols of one, below a wave, either side of a wave and of the block,
    and a 10000-word vocabulary; one rank-3 input."""
    rng = np.random.RandomState(100)
    ref_fn = _log_softmax64 if op == 'LogSoftmax' else _softmax64
    shapes = [(3, c) for c in SOFTMAX_COLS] + [(2, 3, 5)]
    feeds, fetches, xs = {}, [], []
    for shape in shapes:
        x = _rnd(rng.randn(*shape) * 2, dtype)
        xs.append(x)
        fetches.append(apply_op(op, _feed(feeds, x, dtype)))
    outs = sess.run(fetches, feeds)
    for shape, x, out in zip(shapes, xs, outs):
        _close('%s %s' % (op, shape), out, ref_fn(x), _tol(dtype, TRANSC_TOL))


@pytest.mark.parametrize('op', ['Softmax', 'LogSoftmax'])
def test_softmax_wide_spread_and_inf(sess, op):
    """Logits from uniform(-80, 80), and the same row moved up by 150: the
    result is the same, but exp(230) overflows f32 unless the row maximum
    is subtracted first (exp(80) alone does not). A row holding -inf:
    softmax is exactly 0 there and log-softmax is -inf."""
    rng = np.random.RandomState(101)
    ref_fn = _log_softmax64 if op == 'LogSoftmax' else _softmax64
    wide = rng.uniform(-80, 80, (1, 257)).astype(np.float32)
    high = wide + np.float32(150)
    holed = rng.randn(1, 7).astype(np.float32)
    holed[0, [1, 5]] = -np.inf
    feeds = {}
    fetches = [apply_op(op, _feed(feeds, x, tf.float32))
               for x in (wide, high, holed)]
    out_wide, out_high, out_holed = sess.run(fetches, feeds)
    assert np.isfinite(out_wide).all() and np.isfinite(out_high).all()
    _close(op + ' +-80', out_wide, ref_fn(wide), TRANSC_TOL)
    _close(op + ' +-80 + 150', out_high, ref_fn(high), TRANSC_TOL)
    want = -np.inf if op == 'LogSoftmax' else 0.0
    assert (out_holed[0, [1, 5]] == want).all(), out_holed
    assert np.isfinite(out_holed[0, [0, 2, 3, 4, 6]]).all(), out_holed
    _close(op + ' -inf', out_holed, ref_fn(holed), TRANSC_TOL)


# ---------------------------------------------------------------------------
# fused softmax cross-entropy, sparse and dense labels
# ---------------------------------------------------------------------------
def _sparse_xent_ref(logits, labels):
    lsm = _log_softmax64(logits)
    rows = np.arange(logits.shape[0])
    bp = np.exp(lsm)
    bp[rows, labels] -= 1.0
    return -lsm[rows, labels], bp


def _check_sparse_xent(label, dtype, loss, bp, logits, labels):
    ref_loss, ref_bp = _sparse_xent_ref(logits, labels)
    _close(label + ' loss', loss, ref_loss, _tol(dtype, TRANSC_TOL))
    _close(label + ' backprop', bp, ref_bp, _tol(dtype, TRANSC_TOL))


@pytest.mark.parametrize('itype', ITYPES, ids=ITYPE_IDS)
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_sparse_xent(sess, dtype, itype):
    """Both outputs of the op, labels 0 and cols - 1 among them."""
    rng = np.random.RandomState(102)
    feeds, fetches, cases = {}, [], []
    for cols in (1, 7, 257, 10000):
        logits = _rnd(rng.randn(5, cols) * 2, dtype)
        labels = rng.randint(0, cols, 5).astype(itype.as_numpy_dtype)
        labels[0], labels[1] = 0, cols - 1
        fetches += apply_op('SparseSoftmaxCrossEntropyWithLogits',
                            _feed(feeds, logits, dtype),
                            _feed(feeds, labels, itype))
        cases.append((cols, logits, labels))
    outs = sess.run(fetches, feeds)
    for k, (cols, logits, labels) in enumerate(cases):
        _check_sparse_xent('sparse xent cols=%d' % cols, dtype,
                           outs[2 * k], outs[2 * k + 1], logits, labels)


@pytest.mark.parametrize('itype', ITYPES, ids=ITYPE_IDS)
def test_sparse_xent_extremes(sess, itype):
    """+-80 logits with the label on the smallest logit (loss about 160),
    the same moved up by 150 (exp overflows f32 unless the row maximum is
    subtracted), and confident correct rows (loss near 0: the atol
    decides)."""
    rng = np.random.RandomState(103)
    wide = rng.uniform(-80, 80, (5, 257)).astype(np.float32)
    wide[:, 3] = -80.0
    wide[:, 200] = 80.0
    wide_lbl = wide.argmin(1).astype(itype.as_numpy_dtype)
    sure = rng.randn(5, 7).astype(np.float32)
    sure_lbl = np.array([0, 6, 3, 2, 5], itype.as_numpy_dtype)
    sure[np.arange(5), sure_lbl] = 12.0
    feeds = {}
    fetches = []
    high = wide + np.float32(150)
    for logits, labels in ((wide, wide_lbl), (sure, sure_lbl),
                           (high, wide_lbl)):
        fetches += apply_op('SparseSoftmaxCrossEntropyWithLogits',
                            _feed(feeds, logits, tf.float32),
                            _feed(feeds, labels, itype))
    outs = sess.run(fetches, feeds)
    _check_sparse_xent('sparse xent +-80 + 150', tf.float32, outs[4], outs[5],
                       high, wide_lbl)
    assert (outs[0] > 150).all() and (outs[2] < 1e-3).all(), (outs[0], outs[2])
    _check_sparse_xent('sparse xent +-80', tf.float32, outs[0], outs[1],
                       wide, wide_lbl)
    _check_sparse_xent('sparse xent confident', tf.float32, outs[2], outs[3],
                       sure, sure_lbl)


@pytest.mark.parametrize('itype', ITYPES, ids=ITYPE_IDS)
def test_sparse_xent_label_out_of_range(sess, itype):
    """Labels -1 and cols: NaN loss and an all-NaN backprop row for those
    two rows; the other three rows are not disturbed. GPU kernel only: the
    node is checked to have run there."""
    rng = np.random.RandomState(104)
    cols = 7
    logits = rng.randn(5, cols).astype(np.float32)
    labels = np.array([2, -1, 0, cols, cols - 1], itype.as_numpy_dtype)
    bad, good = [1, 3], [0, 2, 4]
    feeds = {}
    name = 'n_xent_oor_' + itype.name
    fetches = apply_op('SparseSoftmaxCrossEntropyWithLogits',
                       _feed(feeds, logits, tf.float32),
                       _feed(feeds, labels, itype), name=name)
    (loss, bp), on_gpu = _trace_run(sess, fetches, feeds)
    assert name in on_gpu, sorted(on_gpu)
    assert np.isnan(loss[bad]).all(), loss
    assert np.isnan(bp[bad]).all(), bp
    _check_sparse_xent('sparse xent in-range rows', tf.float32, loss[good],
                       bp[good], logits[good], labels[good])


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_dense_xent(sess, dtype):
    """Both outputs; one-hot rows, soft rows that sum to 1 and one row that
    does not."""
    rng = np.random.RandomState(105)
    feeds, fetches, cases = {}, [], []
    for cols in (1, 7, 257, 1000):
        logits = _rnd(rng.randn(4, cols) * 2, dtype)
        labels = rng.rand(4, cols)
        labels /= labels.sum(1, keepdims=True)
        labels[0] = 0.0
        labels[0, cols // 2] = 1.0
        labels[3] *= 1.75
        labels = _rnd(labels, dtype)
        fetches += apply_op('SoftmaxCrossEntropyWithLogits',
                            _feed(feeds, logits, dtype),
                            _feed(feeds, labels, dtype))
        cases.append((cols, logits, labels))
    outs = sess.run(fetches, feeds)
    for k, (cols, logits, labels) in enumerate(cases):
        lsm = _log_softmax64(logits)
        lab = labels.astype(np.float64)
        tol = _tol(dtype, TRANSC_TOL)
        _close('xent cols=%d loss' % cols, outs[2 * k], -(lab * lsm).sum(1),
               tol)
        _close('xent cols=%d backprop' % cols, outs[2 * k + 1],
               np.exp(lsm) - lab, tol)


# ---------------------------------------------------------------------------
# bias add and its gradient
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_bias_add(sess, dtype):
    rng = np.random.RandomState(106)
    shapes = [(5, 3), (2, 3, 3, 7), (4, 1)]
    if dtype == tf.float32:
        # 2048*256*4 + 1 elements: ElemwiseGrid(n, 256, 4) hits its cap and
        # the grid-stride loop takes a second pass
        shapes.append((699051, 3))
        assert 699051 * 3 == GRID_CAP * 4 + 1
    feeds, fetches, cases = {}, [], []
    for shape in shapes:
        x = _rnd(rng.randn(*shape), dtype)
        b = _rnd(rng.randn(shape[-1]), dtype)
        fetches.append(apply_op('BiasAdd', _feed(feeds, x, dtype),
                                _feed(feeds, b, dtype)))
        cases.append((shape, x, b))
    outs = sess.run(fetches, feeds)
    for (shape, x, b), out in zip(cases, outs):
        _close('BiasAdd %s' % (shape,), out,
               x.astype(np.float64) + b.astype(np.float64),
               _tol(dtype, ARITH_TOL))


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_bias_add_grad(sess, dtype):
    """(1, 5): one row. (3, 257): one row chunk (the plain store) and two
    column blocks. (20, 600): an LSTM timestep. (2051, 32): 411 chunks of 5
    rows, the last with one row. Rank 4."""
    rng = np.random.RandomState(107)
    shapes = [(1, 5), (3, 257), (20, 600), (2051, 32), (2, 3, 3, 8)]
    feeds, fetches, refs = {}, [], []
    for shape in shapes:
        dy = _rnd(rng.randn(*shape), dtype)
        fetches.append(apply_op('BiasAddGrad', _feed(feeds, dy, dtype)))
        refs.append(dy.astype(np.float64).reshape(-1, shape[-1]).sum(0))
    outs = sess.run(fetches, feeds)
    for shape, out, ref in zip(shapes, outs, refs):
        if dtype == tf.bfloat16:
            _close('BiasAddGrad %s' % (shape,), out, _bf16(ref),
                   dict(rtol=2e-2, atol=2e-2))
        else:
            _close('BiasAddGrad %s' % (shape,), out, ref,
                   dict(rtol=1e-4, atol=1e-3))


# ---------------------------------------------------------------------------
# empty inputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_empty(sess, dtype):
    """Zero rows: an empty output of the right shape and no error;
    BiasAddGrad sums nothing into c zeros."""
    def empty(*shape):
        return _feed(feeds, np.zeros(shape, np.float32), dtype)

    feeds = {}
    pool = dict(ksize=[1, 2, 2, 1], strides=[1, 2, 2, 1], padding='VALID')
    fetches = [apply_op('Softmax', empty(0, 5))]
    shapes = [(0, 5)]
    fetches += apply_op('SparseSoftmaxCrossEntropyWithLogits', empty(0, 5),
                        _feed(feeds, np.zeros((0,), np.int64), tf.int64))
    shapes += [(0,), (0, 5)]
    fetches += apply_op('SoftmaxCrossEntropyWithLogits', empty(0, 5),
                        empty(0, 5))
    shapes += [(0,), (0, 5)]
    fetches.append(apply_op('BiasAdd', empty(0, 3),
                            _feed(feeds, np.ones(3, np.float32), dtype)))
    shapes.append((0, 3))
    fetches.append(apply_op('MaxPool', empty(0, 4, 4, 8), **pool))
    shapes.append((0, 2, 2, 8))
    fetches.append(apply_op('AvgPool', empty(0, 4, 4, 8), **pool))
    shapes.append((0, 2, 2, 8))
    fetches += apply_op('LSTMGates', empty(0, 8), empty(0, 2))
    shapes += [(0, 2)] * 7
    fetches.append(apply_op('BiasAddGrad', empty(0, 5)))
    outs = sess.run(fetches, feeds)
    for out, shape in zip(outs[:-1], shapes):
        assert out.shape == shape, (out.shape, shape)
    _exact('BiasAddGrad of no rows', outs[-1], np.zeros(5))


# ---------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------
Geom = collections.namedtuple('Geom', 'H W kh kw sh sw ph pw P Q')


def _geom(H, W, ksize, strides, padding):
    (kh, kw), (sh, sw) = ksize, strides
    if padding == 'SAME':
        P, Q = -(-H // sh), -(-W // sw)
        ph = max(0, (P - 1) * sh + kh - H) // 2
        pw = max(0, (Q - 1) * sw + kw - W) // 2
    else:
        P, Q = (H - kh) // sh + 1, (W - kw) // sw + 1
        ph = pw = 0
    return Geom(H, W, kh, kw, sh, sw, ph, pw, P, Q)


def _padded(a, g, fill):
    """a (N, H, W, C) inside a frame of `fill` wide enough for every tap."""
    n, _, _, c = a.shape
    ap = np.full((n, g.ph + g.H + g.kh + g.sh, g.pw + g.W + g.kw + g.sw, c),
                 fill, a.dtype)
    ap[:, g.ph:g.ph + g.H, g.pw:g.pw + g.W] = a
    return ap


def _tap(ap, g, a, b):
    """View (N, P, Q, C) of the padded array: element (a, b) of every
    window."""
    return ap[:, a:a + (g.P - 1) * g.sh + 1:g.sh,
              b:b + (g.Q - 1) * g.sw + 1:g.sw]


def _taps(g):
    """Window offsets in row-major scan order."""
    return [(a, b) for a in range(g.kh) for b in range(g.kw)]


def _crop(ap, g):
    return ap[:, g.ph:g.ph + g.H, g.pw:g.pw + g.W]


def _max_pool_ref(x, dy, g):
    """y, and dx with every dy routed to np.argmax of its window in
    row-major scan order, that is to the first maximum."""
    xp = _padded(x, g, -np.inf)
    wins = np.stack([_tap(xp, g, a, b) for a, b in _taps(g)], -1)
    arg = wins.argmax(-1)
    dxp = np.zeros(xp.shape, np.float64)
    for k, (a, b) in enumerate(_taps(g)):
        view = _tap(dxp, g, a, b)
        view += np.where(arg == k, dy, 0.0)
    return wins.max(-1), _crop(dxp, g)


def _avg_pool_ref(x, dy, g):
    xp = _padded(x.astype(np.float64), g, 0.0)
    ones = _padded(np.ones((1, g.H, g.W, 1)), g, 0.0)
    total = sum(_tap(xp, g, a, b) for a, b in _taps(g))
    count = sum(_tap(ones, g, a, b) for a, b in _taps(g))
    dxp = np.zeros(xp.shape, np.float64)
    for a, b in _taps(g):
        view = _tap(dxp, g, a, b)
        view += dy.astype(np.float64) / count
    return total / count, _crop(dxp, g)


def _pool_attrs(ksize, strides, padding):
    return dict(ksize=[1, ksize[0], ksize[1], 1],
                strides=[1, strides[0], strides[1], 1], padding=padding)


# (H, W, ksize, strides, padding) on x of (2, H, W, C)
POOL_GEOMS = [
    (9, 9, (3, 3), (2, 2), 'SAME'),      # the ResNet stem pool
    (8, 8, (2, 2), (2, 2), 'VALID'),
    (10, 10, (3, 3), (2, 2), 'VALID'),   # row and column 9 uncovered
    (7, 7, (1, 1), (2, 2), 'VALID'),
    (8, 8, (2, 2), (3, 3), 'VALID'),     # stride larger than the kernel
    (7, 10, (3, 2), (2, 1), 'SAME'),     # non-square kernel and stride
    (5, 5, (2, 2), (1, 1), 'SAME'),      # pads below and right only
    (6, 6, (6, 6), (1, 1), 'VALID'),     # global
    (2, 2, (3, 3), (1, 1), 'SAME'),      # kernel larger than the input
]
# bf16 C=8: the 8-wide kernels. bf16 C=4, f32 C=8, f32 C=4: the scalar
# forward, the atomic max gradient, the scalar avg gradient.
POOL_PATHS = [(tf.bfloat16, 8), (tf.bfloat16, 4), (tf.float32, 8),
              (tf.float32, 4)]
POOL_PATH_IDS = ['bf16-c8', 'bf16-c4', 'f32-c8', 'f32-c4']


def _pool_x(rng, data, H, W, C):
    if data == 'ties':
        # what a ReLU leaves: many ties and all-zero windows
        return np.maximum(rng.randint(-3, 3, (2, H, W, C)), 0).astype(
            np.float32)
    # every (n, c) plane a permutation of 0..H*W-1 (at most 99: exact in
    # bf16): a unique maximum in every window
    return np.stack([np.stack([rng.permutation(H * W).reshape(H, W)
                               for _ in range(C)], axis=-1)
                     for _ in range(2)]).astype(np.float32)


def _geom_label(spec):
    H, W, ksize, strides, padding = spec
    return '%dx%d k%s s%s %s' % (H, W, ksize, strides, padding)


@pytest.mark.parametrize('data', ['unique', 'ties'])
@pytest.mark.parametrize('dtype,C', POOL_PATHS, ids=POOL_PATH_IDS)
def test_max_pool_and_grad(sess, dtype, C, data):
    """Bit-equal forward and gradient. dy is integers in [-3, 3], so the
    sums over overlapping windows are exact in bf16 too."""
    rng = np.random.RandomState(108)
    feeds, fetches, cases = {}, [], []
    for spec in POOL_GEOMS:
        g = _geom(*spec)
        x = _pool_x(rng, data, g.H, g.W, C)
        dy = rng.randint(-3, 4, (2, g.P, g.Q, C)).astype(np.float32)
        attrs = _pool_attrs(*spec[2:])
        xt = _feed(feeds, x, dtype)
        y = apply_op('MaxPool', xt, **attrs)
        dx = apply_op('MaxPoolGrad', xt, y, _feed(feeds, dy, dtype), **attrs)
        fetches += [y, dx]
        cases.append((spec, g, x, dy))
    outs = sess.run(fetches, feeds)
    for k, (spec, g, x, dy) in enumerate(cases):
        label = 'max pool %s %s' % (data, _geom_label(spec))
        got_y, got_dx = outs[2 * k], outs[2 * k + 1]
        ref_y, ref_dx = _max_pool_ref(x, dy, g)
        _exact(label + ' y', got_y, ref_y)
        _exact(label + ' dx', got_dx, ref_dx)
        if spec[0] == 10:
            # no window covers row 9 or column 9: written as zero
            assert (got_dx[:, 9] == 0).all() and (got_dx[:, :, 9] == 0).all()
        if data == 'ties':
            # every dy lands exactly once, whichever maximum takes it
            np.testing.assert_array_equal(got_dx.sum((1, 2)), dy.sum((1, 2)),
                                          err_msg=label + ' plane sums')


@pytest.mark.parametrize('dtype,C', POOL_PATHS, ids=POOL_PATH_IDS)
def test_avg_pool_and_grad(sess, dtype, C):
    rng = np.random.RandomState(109)
    feeds, fetches, cases = {}, [], []
    for spec in POOL_GEOMS:
        g = _geom(*spec)
        x = _rnd(rng.randn(2, g.H, g.W, C), dtype)
        dy = _rnd(rng.randn(2, g.P, g.Q, C), dtype)
        attrs = _pool_attrs(*spec[2:])
        fetches += [
            apply_op('AvgPool', _feed(feeds, x, dtype), **attrs),
            apply_op('AvgPoolGrad',
                     tf.constant([2, g.H, g.W, C], dtype=tf.int32),
                     _feed(feeds, dy, dtype), **attrs)]
        cases.append((spec, g, x, dy))
    outs = sess.run(fetches, feeds)
    tol = _tol(dtype, ARITH_TOL)
    for k, (spec, g, x, dy) in enumerate(cases):
        label = 'avg pool ' + _geom_label(spec)
        ref_y, ref_dx = _avg_pool_ref(x, dy, g)
        _close(label + ' y', outs[2 * k], ref_y, tol)
        _close(label + ' dx', outs[2 * k + 1], ref_dx, tol)
        if spec[0] == 10:
            got_dx = outs[2 * k + 1]
            assert (got_dx[:, 9] == 0).all() and (got_dx[:, :, 9] == 0).all()


@pytest.mark.parametrize('dtype,C', [(tf.bfloat16, 256), (tf.float32, 32)],
                         ids=['bf16-c256', 'f32-c32'])
def test_pool_second_pass(sess, dtype, C):
    """2x2 s1 VALID at 130x130: each kernel's own element count (outputs
    for the forwards and the atomic gradient, inputs for the 8-wide and avg
    gradients, an eighth of that for the 8-wide kernels) exceeds 2048*256,
    so its grid-stride loop takes a second pass."""
    per_thread = 8 if dtype == tf.bfloat16 else 1
    assert 129 * 129 * C // per_thread > GRID_CAP
    spec = (130, 130, (2, 2), (1, 1), 'VALID')
    g = _geom(*spec)
    attrs = _pool_attrs(*spec[2:])
    rng = np.random.RandomState(110)
    xm = np.maximum(rng.randint(-3, 3, (1, 130, 130, C)), 0).astype(
        np.float32)
    dym = rng.randint(-3, 4, (1, 129, 129, C)).astype(np.float32)
    xa = _rnd(rng.randn(1, 130, 130, C), dtype)
    dya = _rnd(rng.randn(1, 129, 129, C), dtype)
    feeds = {}
    xt = _feed(feeds, xm, dtype)
    y = apply_op('MaxPool', xt, **attrs)
    fetches = [
        y, apply_op('MaxPoolGrad', xt, y, _feed(feeds, dym, dtype), **attrs),
        apply_op('AvgPool', _feed(feeds, xa, dtype), **attrs),
        apply_op('AvgPoolGrad', tf.constant([1, 130, 130, C], dtype=tf.int32),
                 _feed(feeds, dya, dtype), **attrs)]
    got_y, got_dx, got_ay, got_adx = sess.run(fetches, feeds)
    ref_y, ref_dx = _max_pool_ref(xm, dym, g)
    _exact('big max pool y', got_y, ref_y)
    _exact('big max pool dx', got_dx, ref_dx)
    ref_ay, ref_adx = _avg_pool_ref(xa, dya, g)
    tol = _tol(dtype, ARITH_TOL)
    _close('big avg pool y', got_ay, ref_ay, tol)
    _close('big avg pool dx', got_adx, ref_adx, tol)


# ---------------------------------------------------------------------------
# LSTM cell pointwise kernels
# ---------------------------------------------------------------------------
LSTM_FWD_NAMES = ('i', 'f', 'o', 'ci', 'cs', 'co', 'h')


def _sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-x))


def _lstm_fwd_ref(gates, c_prev, forget_bias):
    gi, gj, gf, go = np.split(gates.astype(np.float64), 4, axis=1)
    i, ci = _sigmoid64(gi), np.tanh(gj)
    f, o = _sigmoid64(gf + forget_bias), _sigmoid64(go)
    cs = f * c_prev.astype(np.float64) + i * ci
    co = np.tanh(cs)
    return i, f, o, ci, cs, co, o * co


def _lstm_gates_in(rng, B, H, dtype):
    """[B, 4H] in split order i, j, f, o. Every block has its own mean, a
    few sigmas from the next, so no two blocks can be swapped unnoticed."""
    blocks = [rng.randn(B, H) * 0.5 + mean for mean in (2.0, -1.0, -2.5, 0.5)]
    return (_rnd(np.concatenate(blocks, 1), dtype),
            _rnd(rng.randn(B, H), dtype))


def _check_lstm_fwd(label, dtype, outs, gates, c_prev, forget_bias):
    refs = _lstm_fwd_ref(gates, c_prev, forget_bias)
    for name, out, ref in zip(LSTM_FWD_NAMES, outs, refs):
        _close('%s %s' % (label, name), out, ref, _tol(dtype, TRANSC_TOL))


LSTM_SHAPES = [(1, 1), (3, 33), (20, 200)]


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_lstm_gates(sess, dtype):
    """All seven outputs, at H of 1, an odd H and the PTB cell's shape, with
    forget_bias of 0, the default 1 and 2.5."""
    rng = np.random.RandomState(111)
    feeds, fetches, cases = {}, [], []
    for B, H in LSTM_SHAPES:
        for fb in (0.0, 1.0, 2.5):
            gates, c_prev = _lstm_gates_in(rng, B, H, dtype)
            fetches += apply_op('LSTMGates', _feed(feeds, gates, dtype),
                                _feed(feeds, c_prev, dtype), forget_bias=fb)
            cases.append((B, H, fb, gates, c_prev))
    outs = sess.run(fetches, feeds)
    for k, (B, H, fb, gates, c_prev) in enumerate(cases):
        _check_lstm_fwd('LSTMGates (%d, %d) fb=%g' % (B, H, fb), dtype,
                        outs[7 * k:7 * k + 7], gates, c_prev, fb)


def test_lstm_gates_saturated(sess):
    """Pre-activations of +-30 and +-100: exp overflows inside the sigmoid;
    the outputs stay finite and the gates stay in [0, 1]."""
    rng = np.random.RandomState(112)
    gates = rng.choice([-100.0, -30.0, 30.0, 100.0], (3, 4 * 33)).astype(
        np.float32)
    c_prev = rng.randn(3, 33).astype(np.float32)
    feeds = {}
    outs = sess.run(apply_op('LSTMGates', _feed(feeds, gates, tf.float32),
                             _feed(feeds, c_prev, tf.float32)), feeds)
    for name, out in zip(LSTM_FWD_NAMES, outs):
        assert np.isfinite(out).all(), name
        if name in ('i', 'f', 'o'):
            assert (out >= 0).all() and (out <= 1).all(), name
    _check_lstm_fwd('LSTMGates saturated', tf.float32, outs, gates, c_prev,
                    1.0)


def _lstm_grad_in(rng, B, H, dtype):
    """c_prev, i, f, o, ci, co, dh, dcs_next: the saved activations are
    independent draws from their ranges, not a forward pass's outputs."""
    return [_rnd(a, dtype) for a in (
        rng.randn(B, H),
        rng.uniform(0.05, 0.95, (B, H)), rng.uniform(0.05, 0.95, (B, H)),
        rng.uniform(0.05, 0.95, (B, H)),
        rng.uniform(-0.9, 0.9, (B, H)), rng.uniform(-0.9, 0.9, (B, H)),
        rng.randn(B, H), rng.randn(B, H))]


def _lstm_grad_ref(c_prev, i, f, o, ci, co, dh, dcs_next):
    c_prev, i, f, o, ci, co, dh, dcs_next = (
        a.astype(np.float64) for a in (c_prev, i, f, o, ci, co, dh, dcs_next))
    dcs = dh * o * (1 - co * co) + dcs_next
    di = dcs * ci * i * (1 - i)
    dj = dcs * i * (1 - ci * ci)
    df = dcs * c_prev * f * (1 - f)
    do = dh * co * o * (1 - o)
    return np.concatenate([di, dj, df, do], 1), dcs * f


def _check_lstm_grad(label, dtype, dgates, dc_prev, ins):
    ref_dgates, ref_dc = _lstm_grad_ref(*ins)
    tol = _tol(dtype, TRANSC_TOL)
    assert dgates.shape == ref_dgates.shape, (label, dgates.shape)
    H = ref_dc.shape[1]
    for k, name in enumerate(('di', 'dj', 'df', 'do')):
        _close('%s %s' % (label, name), dgates[:, k * H:(k + 1) * H],
               ref_dgates[:, k * H:(k + 1) * H], tol)
    _close(label + ' dc_prev', dc_prev, ref_dc, tol)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_lstm_gates_grad(sess, dtype):
    """The four blocks of the packed dgates [B, 4H] (order i, j, f, o) and
    dc_prev, with dh and dcs_next both nonzero."""
    rng = np.random.RandomState(113)
    feeds, fetches, cases = {}, [], []
    for B, H in LSTM_SHAPES:
        ins = _lstm_grad_in(rng, B, H, dtype)
        fetches += apply_op('LSTMGatesGrad',
                            *[_feed(feeds, a, dtype) for a in ins])
        cases.append((B, H, ins))
    outs = sess.run(fetches, feeds)
    for k, (B, H, ins) in enumerate(cases):
        _check_lstm_grad('LSTMGatesGrad (%d, %d)' % (B, H), dtype,
                         outs[2 * k], outs[2 * k + 1], ins)


def test_lstm_second_pass(sess):
    """B*H = 2 * 262147 = 2048*256 + 6: both kernels' grid-stride loops
    take a second pass, across a row boundary of an odd H."""
    B, H = 2, 262147
    assert B * H > GRID_CAP
    rng = np.random.RandomState(114)
    gates, c_prev = _lstm_gates_in(rng, B, H, tf.float32)
    ins = _lstm_grad_in(rng, B, H, tf.float32)
    feeds = {}
    fetches = apply_op('LSTMGates', _feed(feeds, gates, tf.float32),
                       _feed(feeds, c_prev, tf.float32), forget_bias=1.0)
    fetches += apply_op('LSTMGatesGrad',
                        *[_feed(feeds, a, tf.float32) for a in ins])
    outs = sess.run(fetches, feeds)
    _check_lstm_fwd('big LSTMGates', tf.float32, outs[:7], gates, c_prev, 1.0)
    _check_lstm_grad('big LSTMGatesGrad', tf.float32, outs[7], outs[8], ins)


# ---------------------------------------------------------------------------
# LRN
# ---------------------------------------------------------------------------
def _lrn_ref(x, radius, bias, alpha, beta):
    x = x.astype(np.float64)
    c = x.shape[-1]
    sq = x * x
    s = np.empty_like(x)
    for k in range(c):
        s[..., k] = sq[..., max(0, k - radius):min(c, k + radius + 1)].sum(-1)
    return x * (bias + alpha * s) ** -beta


def test_lrn(sess):
    """bias = alpha = 1 on randn inputs: one channel more or less in the
    window moves y by tens of percent, far above the bound. Radius 0, a
    window inside the row, and a radius of at least c."""
    rng = np.random.RandomState(115)
    feeds, fetches, cases = {}, [], []
    for c in (1, 5, 16, 96):
        x = rng.randn(2, 3, 3, c).astype(np.float32)
        xt = _feed(feeds, x, tf.float32)
        for radius in (0, 2, 5):
            for beta in (0.5, 0.75, 1.0):
                fetches.append(apply_op('LRN', xt, depth_radius=radius,
                                        bias=1.0, alpha=1.0, beta=beta))
                cases.append((x, radius, 1.0, 1.0, beta))
    # the AlexNet setting
    x = rng.randn(2, 3, 3, 96).astype(np.float32)
    fetches.append(apply_op('LRN', _feed(feeds, x, tf.float32),
                            depth_radius=5, bias=2.0, alpha=1e-4, beta=0.75))
    cases.append((x, 5, 2.0, 1e-4, 0.75))
    outs = sess.run(fetches, feeds)
    for (x, radius, bias, alpha, beta), out in zip(cases, outs):
        _close('LRN c=%d r=%d bias=%g alpha=%g beta=%g' % (
            x.shape[-1], radius, bias, alpha, beta), out,
            _lrn_ref(x, radius, bias, alpha, beta), TRANSC_TOL)


# ---------------------------------------------------------------------------
# depthwise convolution
# ---------------------------------------------------------------------------
def _depthwise_ref(x, w, dy, g):
    """float64 loops over the filter taps. Returns (sum, sum of absolute
    values of the terms) for y, dx and dw."""
    x, w, dy = (a.astype(np.float64) for a in (x, w, dy))
    n, _, _, c = x.shape
    mult = w.shape[3]
    dy5 = dy.reshape(n, g.P, g.Q, c, mult)
    xp = _padded(x, g, 0.0)
    y, y_abs = np.zeros(dy5.shape), np.zeros(dy5.shape)
    dxp, dxp_abs = np.zeros(xp.shape), np.zeros(xp.shape)
    dw, dw_abs = np.zeros(w.shape), np.zeros(w.shape)
    for r, s in _taps(g):
        xs = _tap(xp, g, r, s)[..., None]            # (N, P, Q, C, 1)
        term = xs * w[r, s]
        y += term
        y_abs += np.abs(term)
        term = dy5 * w[r, s]
        view, view_abs = _tap(dxp, g, r, s), _tap(dxp_abs, g, r, s)
        view += term.sum(-1)
        view_abs += np.abs(term).sum(-1)
        term = xs * dy5
        dw[r, s] = term.sum((0, 1, 2))
        dw_abs[r, s] = np.abs(term).sum((0, 1, 2))
    return ((y.reshape(dy.shape), y_abs.reshape(dy.shape)),
            (_crop(dxp, g), _crop(dxp_abs, g)), (dw, dw_abs))


def _check_bf16_sum(label, out, ref, ref_abs):
    """f32 accumulation rounded once to bf16, against the float64 sum."""
    assert out.shape == ref.shape, (label, out.shape, ref.shape)
    err = np.abs(out.astype(np.float64) - ref)
    bound = 2.0 ** -8 * ref_abs + (2.0 ** -8 + 1e-4) * np.abs(ref)
    ratio = err / np.maximum(bound, 1e-300)
    print('%s: max abs err %.3g, max err/bound %.3g' % (label, err.max(),
                                                        ratio.max()))
    bad = err > bound
    assert not bad.any(), '%s: %d of %d elements out of bound, worst %g' % (
        label, bad.sum(), bad.size, ratio.max())


# (x shape, filter (R, S, mult), stride, padding)
DEPTHWISE_CASES = [
    ((2, 9, 9, 4), (3, 3, 1), 1, 'SAME'),
    ((2, 9, 9, 4), (3, 3, 3), 1, 'SAME'),
    ((2, 9, 9, 8), (3, 3, 2), 2, 'SAME'),
    ((1, 8, 10, 5), (3, 2, 2), 1, 'VALID'),
    ((2, 7, 7, 3), (1, 1, 1), 2, 'VALID'),
]


@pytest.mark.parametrize('xshape,filt,stride,padding', DEPTHWISE_CASES,
                         ids=['3x3-m1', '3x3-m3', '3x3-m2-s2', '3x2-m2-valid',
                              '1x1-s2-valid'])
def test_depthwise(sess, xshape, filt, stride, padding):
    n, H, W, c = xshape
    R, S, mult = filt
    g = _geom(H, W, (R, S), (stride, stride), padding)
    rng = np.random.RandomState(116)
    x = _bf16(rng.randn(*xshape) * 0.5)
    w = _bf16(rng.randn(R, S, c, mult) * 0.5)
    dy = _bf16(rng.randn(n, g.P, g.Q, c * mult) * 0.5)
    attrs = dict(strides=[1, stride, stride, 1], padding=padding)
    feeds = {}
    xt, wt, dyt = (_feed(feeds, a, tf.bfloat16) for a in (x, w, dy))
    fetches = [
        apply_op('DepthwiseConv2dNative', xt, wt, **attrs),
        apply_op('DepthwiseConv2dNativeBackpropInput',
                 tf.constant(list(xshape), dtype=tf.int32), wt, dyt, **attrs),
        apply_op('DepthwiseConv2dNativeBackpropFilter', xt,
                 tf.constant([R, S, c, mult], dtype=tf.int32), dyt, **attrs)]
    outs = sess.run(fetches, feeds)
    refs = _depthwise_ref(x, w, dy, g)
    for name, out, (ref, ref_abs) in zip(('y', 'dx', 'dw'), outs, refs):
        _check_bf16_sum('depthwise ' + name, out, ref, ref_abs)


# ---------------------------------------------------------------------------
# window geometry (csrc/kernels/window_geom.h) in front of the GPU kernels
# ---------------------------------------------------------------------------
def test_window_geometry(sess):
    """The GPU MaxPool, Conv2D (bf16) and QuantizedMaxPool refuse what the
    CPU kernels refuse (tests/test_window_geom.py), in the host op and so
    before any launch. One MaxPool and one Conv2D with odd SAME padding (5x5,
    window 3, stride 2) then agree with the CPU kernels: max pool exactly,
    the conv within the bf16 sum bound of this file, its CPU result and the
    CPU conv of the absolute values standing in for the float64 sums."""
    gpu_ops = ('MaxPool', 'Conv2D', 'QuantizedMaxPool')
    # A failed run leaves no trace to read the placement from, and a node
    # without a GPU kernel falls back to the CPU, whose kernels raise the
    # same text. Placement looks at the op, its types and the requested
    # device only, never at ksize, strides or padding: the valid twin of
    # each rejected node, built the same way, has to run on the GPU.
    for op in gpu_ops:
        twin, feeds = window_op(op, (1, 2, 2, 8), 2, [1, 2, 2, 1],
                                [1, 1, 1, 1], 'SAME', '/gpu:0',
                                bf16=op == 'Conv2D')
        out, on_gpu = _trace_run(sess, twin, feeds)
        assert twin.op.name in on_gpu, (op, sorted(on_gpu))
        assert out.shape[:3] == (1, 2, 2), (op, out.shape)
    # a session of its own, on the module's graph: the failed runs must not
    # be the shared session's
    with _sess() as s:
        for op, case in reject_list(gpu_ops):
            fetch, feeds = rejected_op(op, case, '/gpu:0', n=1, c=8,
                                       bf16=op == 'Conv2D')
            with pytest.raises(tf.errors.InvalidArgumentError,
                               match=op + ': '):
                s.run(fetch, feeds)

    rng = np.random.RandomState(118)
    x = _bf16(rng.randn(2, 5, 5, 8) * 0.5)
    w = _bf16(rng.randn(3, 3, 8, 8) * 0.5)
    pool = _pool_attrs((3, 3), (2, 2), 'SAME')
    conv = dict(strides=[1, 2, 2, 1], padding='SAME')
    feeds = {}
    xf, wf = _feed(feeds, x, tf.float32), _feed(feeds, w, tf.float32)
    xa, wa = _feed(feeds, np.abs(x), tf.float32), \
        _feed(feeds, np.abs(w), tf.float32)
    with tf.device('/gpu:0'):
        fetches = [
            apply_op('MaxPool', xf, name='g_maxpool', **pool),
            apply_op('MaxPool', tf.cast(xf, tf.bfloat16), name='g_maxpool_bf',
                     **pool),
            apply_op('Conv2D', tf.cast(xf, tf.bfloat16),
                     tf.cast(wf, tf.bfloat16), name='g_conv', **conv)]
    with tf.device('/cpu:0'):
        fetches += [apply_op('MaxPool', xf, **pool),
                    apply_op('Conv2D', xf, wf, **conv),
                    apply_op('Conv2D', xa, wa, **conv)]
    outs, on_gpu = _trace_run(sess, fetches, feeds)
    for name in ('g_maxpool', 'g_maxpool_bf', 'g_conv'):
        assert name in on_gpu, (name, sorted(on_gpu))
    pool_f32, pool_bf16, conv_bf16, pool_cpu, conv_cpu, conv_abs = outs
    assert pool_cpu.shape == (2, 3, 3, 8) and conv_cpu.shape == (2, 3, 3, 8)
    _exact('max pool f32 vs cpu', pool_f32, pool_cpu)
    _exact('max pool bf16 vs cpu', pool_bf16, pool_cpu)
    _check_bf16_sum('conv2d bf16 vs cpu', conv_bf16,
                    conv_cpu.astype(np.float64), conv_abs.astype(np.float64))


# ---------------------------------------------------------------------------
# placement: the ops above really run on the GPU
# ---------------------------------------------------------------------------
def test_nn_ops_run_on_gpu(sess):
    rng = np.random.RandomState(117)
    feeds = {}

    def f32(*shape):
        return _feed(feeds, rng.randn(*shape).astype(np.float32), tf.float32)

    def bf16(*shape):
        return _feed(feeds, _bf16(rng.randn(*shape)), tf.bfloat16)

    x2 = f32(4, 6)
    x4 = f32(2, 4, 4, 8)
    pool = dict(ksize=[1, 2, 2, 1], strides=[1, 2, 2, 1], padding='VALID')
    conv = dict(strides=[1, 1, 1, 1], padding='SAME')
    lbl = _feed(feeds, np.array([1, 0, 5, 2], np.int32), tf.int32)
    y = apply_op('MaxPool', x4, name='n_maxpool', **pool)
    dwx, dww, dwdy = bf16(1, 5, 5, 4), bf16(3, 3, 4, 2), bf16(1, 5, 5, 8)
    fetches = [
        apply_op('Softmax', x2, name='n_softmax'),
        apply_op('LogSoftmax', x2, name='n_logsoftmax'),
        apply_op('BiasAdd', x2, f32(6), name='n_biasadd'),
        apply_op('BiasAddGrad', x2, name='n_biasgrad'),
        y,
        apply_op('MaxPoolGrad', x4, y, f32(2, 2, 2, 8), name='n_maxpoolgrad',
                 **pool),
        apply_op('AvgPool', x4, name='n_avgpool', **pool),
        apply_op('AvgPoolGrad', tf.constant([2, 4, 4, 8], dtype=tf.int32),
                 f32(2, 2, 2, 8), name='n_avgpoolgrad', **pool),
        apply_op('LRN', x4, name='n_lrn'),
        apply_op('DepthwiseConv2dNative', dwx, dww, name='n_dw', **conv),
        apply_op('DepthwiseConv2dNativeBackpropInput',
                 tf.constant([1, 5, 5, 4], dtype=tf.int32), dww, dwdy,
                 name='n_dw_dx', **conv),
        apply_op('DepthwiseConv2dNativeBackpropFilter', dwx,
                 tf.constant([3, 3, 4, 2], dtype=tf.int32), dwdy,
                 name='n_dw_dw', **conv),
    ]
    fetches += apply_op('SparseSoftmaxCrossEntropyWithLogits', x2, lbl,
                        name='n_sparse_xent')
    fetches += apply_op('SoftmaxCrossEntropyWithLogits', x2, f32(4, 6),
                        name='n_xent')
    fetches += apply_op('LSTMGates', f32(4, 24), x2, name='n_lstm')
    fetches += apply_op('LSTMGatesGrad', *[f32(4, 6) for _ in range(8)],
                        name='n_lstmgrad')
    _, on_gpu = _trace_run(sess, fetches, feeds)
    for name in ('n_softmax', 'n_logsoftmax', 'n_biasadd', 'n_biasgrad',
                 'n_maxpool', 'n_maxpoolgrad', 'n_avgpool', 'n_avgpoolgrad',
                 'n_lrn', 'n_dw', 'n_dw_dx', 'n_dw_dw', 'n_sparse_xent',
                 'n_xent', 'n_lstm', 'n_lstmgrad'):
        assert name in on_gpu, (name, sorted(on_gpu))
