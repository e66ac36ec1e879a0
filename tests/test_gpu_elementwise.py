"""Pinning tests for the elementwise HIP kernels
(csrc/kernels/hip/elementwise.hip through csrc/kernels/gpu_elementwise.cc):
unary, binary (same-shape, scalar, broadcast), Cast, AddN, Fill, ZerosLike,
OnesLike, Mean's scale and the _FusedElementwise interpreter. Every input goes
through a placeholder so constant folding cannot run an op on the CPU, and
sections 1-5 fetch a single op per output: a fetched node is never fused.
References are plain numpy. All tests need a gfx950 GPU.

The four bounds used here:
  exact f32   bit-equal to the same float32 arithmetic in numpy (none of the
              ops offers a mul-then-add to contract; f32 divide and sqrt are
              correctly rounded in the default hipcc build)
  exact bf16  bit-equal to _bf16(<that f32 result>): the kernels compute in
              f32 and round once to nearest-even
  tol f32     rtol 1e-5, atol 1e-6 against float64 (the project's own bound
              for these ops in test_fusion.py)
  tol bf16    rtol 4e-3, atol 1e-6 against float64 on the bf16-exact inputs:
              one rounding into 8 significant bits costs at most 2^-8 =
              3.906e-3, the f32 evaluation at most the 1e-5 above

Left open on purpose: what the selecting ops (Sign, Relu, Relu6, Maximum,
Minimum, ReluGrad, Relu6Grad) return for a NaN input. The fused (fmaxf) and
unfused (a > b ? a : b) forms differ there."""
import itertools

import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.framework.ops import apply_op

from test_gpu_kernels import _bf16, _sess

pytestmark = pytest.mark.gpu

DTYPES = [tf.float32, tf.bfloat16]
DTYPE_IDS = ['f32', 'bf16']

# below one vector, exactly one (4 f32 / 8 bf16), one plus a tail, many plus
# a tail
SIZES = (1, 3, 7, 8, 9, 1027)
# 2048*256*8 + 5: ElemwiseGrid hits its cap of 2048 blocks in every kernel of
# the file, so each grid-stride loop takes a second pass, and a tail remains
N_BIG = 2048 * 256 * 8 + 5

F32_TOL = dict(rtol=1e-5, atol=1e-6)
BF16_TOL = dict(rtol=4e-3, atol=1e-6)


@pytest.fixture(scope='module')
def sess():
    """One graph and one session for the whole module: opening a session
    costs more than any case here. Every test only adds nodes."""
    tf.reset_default_graph()
    with _sess() as s:
        yield s


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def _with_specials(x, specials):
    """Overwrite the end of x (the vector tail) with the special values."""
    k = min(len(specials), x.size)
    if k:
        x.reshape(-1)[x.size - k:] = specials[:k]
    return x


def _domain(kind, rng, shape):
    """float32 inputs from the issue's domain table (before bf16 rounding)."""
    n = int(np.prod(shape))
    if kind == 'randn':
        x = rng.randn(n)
    elif kind == 'pos':        # log-uniform in [1e-3, 1e3]
        x = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n))
    elif kind == 'log':
        x = _with_specials(np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n)),
                           [1 + 2.0 ** -10, 1 - 2.0 ** -10, 1 + 2.0 ** -7])
    elif kind == 'log1p':
        x = rng.uniform(-0.9, 8, n)
    elif kind == 'pm8':
        x = rng.uniform(-8, 8, n)
    elif kind == 'div':        # +-[0.5, 2]
        x = rng.uniform(0.5, 2, n) * rng.choice([-1.0, 1.0], n)
    elif kind == 'pow_base':
        x = rng.uniform(0.25, 4, n)
    elif kind == 'pow_exp':
        x = rng.uniform(-3, 3, n)
    elif kind == 'sigmoid_y':
        x = rng.uniform(0.05, 0.95, n)
    elif kind == 'tanh_y':
        x = rng.uniform(-0.9, 0.9, n)
    elif kind == 'y':
        x = rng.uniform(0.5, 2, n)
    elif kind == 'relu6':      # both sides of 0 and 6, and exactly 0 and 6
        x = _with_specials(rng.randn(n) * 4 + 3, [0.0, 6.0, -1.0, 7.0, 3.0])
    elif kind == 'steps':      # negative fractions, exact integers, +-0
        x = _with_specials(rng.randn(n) * 3,
                           [-0.5, 0.0, -0.0, 2.0, -3.0, -1.5, 0.5, -0.25])
    else:
        raise KeyError(kind)
    return x.astype(np.float32).reshape(shape)


def _data(kind, rng, shape, dtype):
    """Values from a domain, exactly representable in `dtype`."""
    x = _domain(kind, rng, shape)
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


# ---------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.uint32)


def _check_exact(label, dtype, out, ref32):
    assert ref32.dtype == np.float32, (label, ref32.dtype)
    if dtype == tf.bfloat16:
        ref32 = _bf16(ref32)
    assert out.shape == ref32.shape, (label, out.shape, ref32.shape)
    bad = np.flatnonzero(_bits(out).ravel() != _bits(ref32).ravel())
    print('%s %s exact: %d of %d differ'
          % (label, dtype.name, bad.size, out.size))
    if bad.size:
        i = bad[0]
        raise AssertionError(
            '%s: %d of %d not bit-equal; first at %d: got %r want %r'
            % (label, bad.size, out.size, i, out.ravel()[i],
               ref32.ravel()[i]))


def _check_tol(label, dtype, out, ref64):
    tol = BF16_TOL if dtype == tf.bfloat16 else F32_TOL
    ref64 = np.asarray(ref64, np.float64)
    assert out.shape == ref64.shape, (label, out.shape, ref64.shape)
    if out.size:
        with np.errstate(invalid='ignore'):
            err = np.abs(out.astype(np.float64) - ref64)
            err = np.where(out == ref64, 0.0, err)   # equal infinities
            bound = tol['atol'] + tol['rtol'] * np.abs(ref64)
            print('%s %s max err %.3g, %.3g of the bound'
                  % (label, dtype.name, np.nanmax(err),
                     np.nanmax(err / bound)))
    np.testing.assert_allclose(out, ref64, err_msg=label, **tol)


def _relu(x):
    return np.where(x > 0, x, x.dtype.type(0))


def _relu6(x):
    t = x.dtype.type
    return np.where(x < 0, t(0), np.where(x > 6, t(6), x))


def _sign(x):
    t = x.dtype.type
    return np.where(x > 0, t(1), np.where(x < 0, t(-1), t(0)))


def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


# op -> (exact, numpy function, input domain). An exact op's function is run
# on float32 arrays, a tolerance op's on float64.
UNARY = {
    'Neg': (True, lambda x: -x, 'randn'),
    'Abs': (True, np.abs, 'randn'),
    'Sign': (True, _sign, 'steps'),
    'Square': (True, lambda x: x * x, 'randn'),
    'Sqrt': (True, np.sqrt, 'pos'),
    'Reciprocal': (True, lambda x: 1 / x, 'div'),
    'Floor': (True, np.floor, 'steps'),
    'Ceil': (True, np.ceil, 'steps'),
    'Relu': (True, _relu, 'randn'),
    'Relu6': (True, _relu6, 'relu6'),
    'Rsqrt': (False, lambda x: 1 / np.sqrt(x), 'pos'),
    'Exp': (False, np.exp, 'pm8'),
    'Log': (False, np.log, 'log'),
    'Log1p': (False, np.log1p, 'log1p'),
    'Tanh': (False, np.tanh, 'pm8'),
    'Sigmoid': (False, _sigmoid, 'pm8'),
    'Softplus': (False, lambda x: np.logaddexp(0, x), 'pm8'),
    'Sin': (False, np.sin, 'pm8'),
    'Cos': (False, np.cos, 'pm8'),
}

# op -> (exact, numpy function, first operand's domain, second's). Argument
# order is the op's: (y, dy) for the y/dy grads, (gradient, feature) for the
# selecting grads and SoftplusGrad.
BINARY = {
    'Add': (True, lambda a, b: a + b, 'randn', 'randn'),
    'Sub': (True, lambda a, b: a - b, 'randn', 'randn'),
    'Mul': (True, lambda a, b: a * b, 'randn', 'randn'),
    'RealDiv': (True, lambda a, b: a / b, 'randn', 'div'),
    'Div': (True, lambda a, b: a / b, 'randn', 'div'),
    'Maximum': (True, lambda a, b: np.where(a > b, a, b), 'randn', 'randn'),
    'Minimum': (True, lambda a, b: np.where(a < b, a, b), 'randn', 'randn'),
    'SquaredDifference': (True, lambda a, b: (a - b) * (a - b),
                          'randn', 'randn'),
    'ReluGrad': (True, lambda g, f: np.where(f > 0, g, g.dtype.type(0)),
                 'randn', 'randn'),
    'Relu6Grad': (True, lambda g, f: np.where((f > 0) & (f < 6), g,
                                              g.dtype.type(0)),
                  'randn', 'relu6'),
    'Pow': (False, np.power, 'pow_base', 'pow_exp'),
    'SigmoidGrad': (False, lambda y, dy: dy * y * (1 - y),
                    'sigmoid_y', 'randn'),
    'TanhGrad': (False, lambda y, dy: dy * (1 - y * y), 'tanh_y', 'randn'),
    'RsqrtGrad': (False, lambda y, dy: -0.5 * dy * y ** 3, 'y', 'randn'),
    'SqrtGrad': (False, lambda y, dy: dy / (2 * y), 'y', 'randn'),
    'SoftplusGrad': (False, lambda g, f: g * _sigmoid(f), 'randn', 'pm8'),
}


def _check_unary(label, op, dtype, out, x):
    exact, fn, _ = UNARY[op]
    if exact:
        _check_exact(label, dtype, out, fn(x))
    else:
        _check_tol(label, dtype, out, fn(x.astype(np.float64)))


def _check_binary(label, op, dtype, out, a, b):
    exact, fn, _, _ = BINARY[op]
    if exact:
        ref = fn(*np.broadcast_arrays(a, b))
        _check_exact(label, dtype, out, np.ascontiguousarray(ref))
    else:
        _check_tol(label, dtype, out,
                   fn(a.astype(np.float64), b.astype(np.float64)))


def _seed(*parts):
    return sum(ord(c) * (i + 1) for i, c in enumerate(''.join(parts))) + 1000


# ---------------------------------------------------------------------------
# 1. unary ops
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('op', sorted(UNARY))
def test_unary(sess, op, dtype):
    rng = np.random.RandomState(_seed(op))
    feeds, fetches, xs = {}, [], []
    for n in SIZES:
        x = _data(UNARY[op][2], rng, (n,), dtype)
        xs.append(x)
        fetches.append(apply_op(op, _feed(feeds, x, dtype)))
    outs = sess.run(fetches, feeds)
    for x, out in zip(xs, outs):
        _check_unary('%s n=%d' % (op, x.size), op, dtype, out, x)


def test_unary_special_values(sess):
    """Overflow and underflow ends in f32. Softplus(100) = 100 is where the
    unstable log1p(exp(x)) form gives inf."""
    x = np.array([np.inf, -np.inf, 0.0, -0.0, 100.0, -100.0, 1e4, -1e4],
                 np.float32)
    lx = np.array([0.0, np.inf], np.float32)
    ops = ['Exp', 'Sigmoid', 'Tanh', 'Softplus', 'Neg', 'Abs', 'Square',
           'Relu']
    feeds = {}
    p = _feed(feeds, x, tf.float32)
    fetches = [apply_op(op, p) for op in ops]
    fetches.append(apply_op('Log', _feed(feeds, lx, tf.float32)))
    outs = sess.run(fetches, feeds)
    with np.errstate(all='ignore'):
        for op, out in zip(ops, outs):
            # rounded to f32, so that what overflows f32 is inf in both
            ref = UNARY[op][1](x.astype(np.float64)).astype(np.float32)
            _check_tol(op + ' special', tf.float32, out, ref)
        _check_tol('Log special', tf.float32, outs[-1],
                   np.log(lx.astype(np.float64)))
    softplus = outs[ops.index('Softplus')]
    assert softplus[4] == 100.0
    # 3.7e-44: zero or the denormal
    assert 0.0 <= softplus[5] <= 1e-40


def test_nan_propagates(sess):
    """Only for the non-selecting ops; see the module docstring."""
    x = np.array([np.nan, 1.0, np.nan, 2.0, 0.5], np.float32)
    y = np.array([1.0, np.nan, np.nan, 3.0, 0.25], np.float32)
    feeds = {}
    px = _feed(feeds, x, tf.float32)
    py = _feed(feeds, y, tf.float32)
    unary = ['Neg', 'Exp', 'Log', 'Tanh', 'Sigmoid']
    fetches = [apply_op(op, px) for op in unary]
    fetches += [apply_op('Add', px, py), apply_op('Mul', px, py)]
    outs = sess.run(fetches, feeds)
    for op, out in zip(unary, outs):
        np.testing.assert_array_equal(np.isnan(out), np.isnan(x), err_msg=op)
    for op, out in zip(['Add', 'Mul'], outs[len(unary):]):
        np.testing.assert_array_equal(np.isnan(out),
                                      np.isnan(x) | np.isnan(y), err_msg=op)


# ---------------------------------------------------------------------------
# 2. binary ops: same shape, scalar, broadcast, one-element operands
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('op', sorted(BINARY))
def test_binary_same_shape(sess, op, dtype):
    rng = np.random.RandomState(_seed(op, 'same'))
    _, _, dom_a, dom_b = BINARY[op]
    feeds, fetches, args = {}, [], []
    for n in SIZES:
        a = _data(dom_a, rng, (n,), dtype)
        b = _data(dom_b, rng, (n,), dtype)
        args.append((a, b))
        fetches.append(apply_op(op, _feed(feeds, a, dtype),
                                _feed(feeds, b, dtype)))
    outs = sess.run(fetches, feeds)
    for (a, b), out in zip(args, outs):
        _check_binary('%s n=%d' % (op, a.size), op, dtype, out, a, b)


# op -> (scalar used as the first operand, scalar used as the second), each
# bf16-exact and inside that operand's domain. ReluGrad's scalar feature is
# negative and Relu6Grad's is inside (0, 6): selecting on the gradient
# instead would give a mix of zeros and gradients in both.
SCALARS = {
    'Sub': (0.75, -1.25),
    'RealDiv': (1.5, -0.75),
    'Pow': (2.5, 1.5),
    'SquaredDifference': (0.75, -1.25),
    'SigmoidGrad': (0.25, -1.25),
    'TanhGrad': (0.5, -1.25),
    'RsqrtGrad': (1.25, -1.25),
    'SqrtGrad': (1.25, -1.25),
    'ReluGrad': (0.75, -1.25),
    'Relu6Grad': (0.75, 3.0),
    'SoftplusGrad': (0.75, -1.25),
}


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('op', sorted(SCALARS))
def test_binary_scalar(sess, op, dtype):
    """op(x, c) and op(c, x) with c a placeholder of shape []: operand
    order on the two scalar paths."""
    n = 1027
    rng = np.random.RandomState(_seed(op, 'scalar'))
    _, _, dom_a, dom_b = BINARY[op]
    c_first, c_second = (np.float32(c) for c in SCALARS[op])
    xa = _data(dom_a, rng, (n,), dtype)
    xb = _data(dom_b, rng, (n,), dtype)
    feeds = {}
    right = apply_op(op, _feed(feeds, xa, dtype),
                     _feed(feeds, c_second, dtype))
    left = apply_op(op, _feed(feeds, c_first, dtype),
                    _feed(feeds, xb, dtype))
    out_r, out_l = sess.run([right, left], feeds)
    _check_binary(op + ' scalar right', op, dtype, out_r, xa,
                  np.asarray(c_second))
    _check_binary(op + ' scalar left', op, dtype, out_l,
                  np.asarray(c_first), xb)


BCAST_SHAPES = [
    ((4, 1, 5), (1, 3, 1)),                        # both sides broadcast
    ((6, 5), (5,)),
    ((6, 5), (6, 1)),
    ((2, 1, 3, 1, 2, 3), (1, 3, 1, 2, 1, 3)),      # rank 6: BcastArgs' limit
]


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('op', ['Sub', 'RealDiv'])
def test_binary_broadcast(sess, op, dtype):
    rng = np.random.RandomState(_seed(op, 'bcast'))
    feeds, fetches, args = {}, [], []
    for sa, sb in BCAST_SHAPES:
        a = _data('randn', rng, sa, dtype)
        b = _data('div', rng, sb, dtype)
        args.append((a, b))
        fetches.append(apply_op(op, _feed(feeds, a, dtype),
                                _feed(feeds, b, dtype)))
    outs = sess.run(fetches, feeds)
    for (a, b), out in zip(args, outs):
        assert out.shape == np.broadcast(a, b).shape
        _check_binary('%s %s %s' % (op, a.shape, b.shape), op, dtype, out,
                      a, b)


def test_binary_broadcast_rank7_raises(sess):
    rng = np.random.RandomState(60)
    a = _data('randn', rng, (2, 1, 1, 1, 1, 1, 3), tf.float32)
    b = _data('randn', rng, (1, 1, 1, 1, 1, 2, 1), tf.float32)
    feeds = {}
    z = apply_op('Sub', _feed(feeds, a, tf.float32),
                 _feed(feeds, b, tf.float32))
    # a session of its own, on the module's graph (hence the fixture): the
    # failed run must not be the shared session's
    with _sess() as s:
        with pytest.raises(tf.errors.InvalidArgumentError,
                           match='bad broadcast'):
            s.run(z, feeds)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_binary_one_element_higher_rank(sess, dtype):
    """A one-element operand whose rank exceeds the other side's still
    broadcasts: [3] + [1,1] is [1,3], not [3]."""
    rng = np.random.RandomState(61)
    cases = [('Add', (3,), (1, 1)), ('Sub', (1, 1), (3,)),
             ('Add', (1,), (1, 1))]
    feeds, fetches, args = {}, [], []
    for op, sa, sb in cases:
        a = _data('randn', rng, sa, dtype)
        b = _data('randn', rng, sb, dtype)
        args.append((op, a, b))
        fetches.append(apply_op(op, _feed(feeds, a, dtype),
                                _feed(feeds, b, dtype)))
    outs = sess.run(fetches, feeds)
    for (op, a, b), out in zip(args, outs):
        assert out.shape == np.broadcast(a, b).shape, (op, a.shape, b.shape)
        _check_binary('%s %s %s' % (op, a.shape, b.shape), op, dtype, out,
                      a, b)


# ---------------------------------------------------------------------------
# 3. Cast
# ---------------------------------------------------------------------------
_I32 = [16777217, -16777217, 2 ** 31 - 1, -2 ** 31 + 1]
_TO_INT = [1.7, -1.7, 0.5, -0.5, 2.0, -2.0]   # truncation toward zero


def _ints(rng, n, dtype, specials):
    x = rng.randint(-2 ** 31 + 1, 2 ** 31 - 1, n).astype(dtype)
    return _with_specials(x, np.array(specials, dtype))


def _cast_input(src, dst, rng, n):
    """Inputs for one cast pair, the issue's required values at the tail."""
    if src == tf.bool:
        return rng.rand(n) < 0.5
    if src == tf.int32:
        specials = [0, 1, -1, 2 ** 24 + 1] if dst == tf.bool else _I32
        x = _ints(rng, n, np.int32, specials)
    elif src == tf.int64:
        if dst == tf.bool:
            specials = [0, 1, -1, 2 ** 24 + 1, 2 ** 32]
        elif dst == tf.int32:
            specials = _I32           # only values an int32 holds
        else:
            specials = _I32 + [2 ** 40 + 1, -2 ** 40 - 1, 2 ** 53 + 1]
        x = _ints(rng, n, np.int64, specials)
    elif dst == tf.bool:
        x = _with_specials(rng.randn(n), [0.0, -0.0, 0.5, -3.0])
        x[:n // 2] = 0.0
    elif dst == tf.int32:
        x = _with_specials(rng.randn(n) * 1e3, _TO_INT + [2.0 ** 30, -2e9])
    elif dst == tf.int64:
        x = _with_specials(rng.randn(n) * 1e3,
                           _TO_INT + [3e9, -3e9, 2.0 ** 40, -2.0 ** 62])
    else:
        # ties between two bf16 neighbours, which round to even
        x = _with_specials(rng.randn(n),
                           [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,
                            -1 - 2.0 ** -8, -1 - 3 * 2.0 ** -8])
    if src in (tf.float32, tf.bfloat16):
        x = x.astype(np.float32)
        if src == tf.bfloat16:
            x = _bf16(x)
    return x


# the 17 pairs stf_cast lists
CAST_PAIRS = [
    (tf.float32, tf.bfloat16), (tf.bfloat16, tf.float32),
    (tf.float32, tf.int32), (tf.int32, tf.float32),
    (tf.int64, tf.float32), (tf.float32, tf.int64),
    (tf.int32, tf.int64), (tf.int64, tf.int32),
    (tf.bfloat16, tf.bfloat16), (tf.float32, tf.float32),
    (tf.bool, tf.float32), (tf.bool, tf.bfloat16),
    (tf.bool, tf.int32), (tf.bool, tf.int64),
    (tf.float32, tf.bool), (tf.int32, tf.bool), (tf.int64, tf.bool),
]
_NAMES = {tf.float32: 'f32', tf.bfloat16: 'bf16', tf.int32: 'i32',
          tf.int64: 'i64', tf.bool: 'bool'}


def _cast_ref(x, dst):
    """ndarray.astype; a bf16 result comes back from the session as f32."""
    if dst == tf.bfloat16:
        return _bf16(x.astype(np.float32))
    return x.astype(dst.as_numpy_dtype)


@pytest.mark.parametrize('src,dst', CAST_PAIRS,
                         ids=['%s-%s' % (_NAMES[s], _NAMES[d])
                              for s, d in CAST_PAIRS])
def test_cast(sess, src, dst):
    n = 1027
    rng = np.random.RandomState(70 + CAST_PAIRS.index((src, dst)))
    x = _cast_input(src, dst, rng, n)
    feeds = {}
    y = apply_op('Cast', _feed(feeds, x, src), DstT=dst)
    out = sess.run(y, feeds)
    ref = _cast_ref(x, dst)
    assert out.dtype == ref.dtype and out.shape == ref.shape
    # bit-equal, element by element
    bad = np.flatnonzero((out.view(np.uint8).reshape(n, -1)
                          != ref.view(np.uint8).reshape(n, -1)).any(axis=1))
    assert bad.size == 0, ('%d differ; first: in %r got %r want %r'
                           % (bad.size, x[bad[0]], out[bad[0]], ref[bad[0]]))


# ---------------------------------------------------------------------------
# 4. AddN, Fill, ZerosLike, OnesLike
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('count', [1, 2, 3, 5])
def test_add_n(sess, count, dtype):
    """The kernel adds pairwise, left to right, and stores `dtype` after
    each add; so does the reference."""
    n = 1027
    rng = np.random.RandomState(80 + count)
    xs = [_data('randn', rng, (n,), dtype) for _ in range(count)]
    feeds = {}
    y = apply_op('AddN', [_feed(feeds, x, dtype) for x in xs])
    out = sess.run(y, feeds)
    ref = xs[0]
    for x in xs[1:]:
        ref = ref + x
        if dtype == tf.bfloat16:
            ref = _bf16(ref)
    _check_exact('AddN %d' % count, tf.float32, out, ref)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_fill_zeros_ones(sess, dtype):
    n = 1027
    rng = np.random.RandomState(85)
    feeds = {}
    dims = _feed(feeds, np.array([13, 79], np.int32), tf.int32)
    value = _feed(feeds, np.float32(0.1), dtype)
    x = _feed(feeds, _data('randn', rng, (n,), dtype), dtype)
    fetches = [apply_op('Fill', dims, value), apply_op('ZerosLike', x),
               apply_op('OnesLike', x)]
    filled, zeros, ones = sess.run(fetches, feeds)
    want = np.float32(0.1)
    if dtype == tf.bfloat16:
        want = _bf16(want)
    _check_exact('Fill', tf.float32, filled,
                 np.full((13, 79), want, np.float32))
    assert filled[-1, -1] == want
    _check_exact('ZerosLike', tf.float32, zeros, np.zeros(n, np.float32))
    _check_exact('OnesLike', tf.float32, ones, np.ones(n, np.float32))


# ---------------------------------------------------------------------------
# 5. Mean's scale kernel
# ---------------------------------------------------------------------------
def test_mean_scale_tail(sess):
    """reduce_mean is stf_scale's only caller: three adds and a multiply by
    fl(1/3), five roundings of 2^-24 each at the most, under rtol 1e-6 as
    long as nothing cancels; so the inputs are positive."""
    x = np.random.RandomState(90).uniform(0.5, 2, (3, 1027))
    x = x.astype(np.float32)
    feeds = {}
    y = tf.reduce_mean(_feed(feeds, x, tf.float32), 0)
    out = sess.run(y, feeds)
    assert out.shape == (1027,)
    np.testing.assert_allclose(out, x.astype(np.float64).mean(0), rtol=1e-6)


# ---------------------------------------------------------------------------
# 6. the fused interpreter
# ---------------------------------------------------------------------------
def _trace_run(sess, fetches, feeds):
    """test_fusion._trace_run's idiom: names of the nodes that ran on a GPU."""
    opts = tf.RunOptions(trace_level=tf.RunOptions.FULL_TRACE)
    md = tf.RunMetadata()
    outs = sess.run(fetches, feeds, options=opts, run_metadata=md)
    on_gpu = {ns.node_name for ds in md.step_stats.dev_stats
              if 'GPU' in ds.device.upper() for ns in ds.node_stats}
    return outs, on_gpu


def _const(v, dtype):
    return tf.constant(v, dtype=dtype)


_names = itertools.count()


def _uniq(base):
    """Node names are checked against the trace, and the module shares one
    graph, so each is used once."""
    return '%s_%d' % (base, next(_names))


def _run_fused(sess, build, feeds, expect_fused=True):
    """Run identity(build(exit)), where build names its last node `exit`. A
    fetched node is never fused, so the Identity keeps the whole chain
    fusable; the fused node is then called <exit>/_fused."""
    exit_name = _uniq('exit')
    out, on_gpu = _trace_run(sess, tf.identity(build(exit_name)), feeds)
    if expect_fused:
        assert exit_name + '/_fused' in on_gpu, sorted(on_gpu)
    return out, on_gpu


# the unary opcodes of kernels/fused_ew.h; constant added after the op. 8
# keeps log's result away from zero, where its absolute error (relative to
# |log x| <= 6.9) would meet a relative bound.
FUSED_UNARY = ['Relu', 'Relu6', 'Sigmoid', 'Tanh', 'Exp', 'Log', 'Log1p',
               'Neg', 'Sqrt', 'Rsqrt', 'Square', 'Abs', 'Softplus', 'Sign',
               'Floor', 'Reciprocal']
# (id, op, form): x op c, c op x or x op x
FUSED_BINARY = (
    [(op, op, 'xc') for op in ('Add', 'Sub', 'Mul', 'RealDiv', 'Div',
                               'Maximum', 'Minimum', 'SquaredDifference',
                               'Pow')] +
    [(op + '-cx', op, 'cx') for op in ('Sub', 'Div', 'Pow')] +
    [(op + '-xx', op, 'xx') for op in ('Mul', 'SquaredDifference')])


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('op', FUSED_UNARY)
def test_fused_unary_opcode(sess, op, dtype):
    n = 1027
    c = 8.0 if op in ('Log', 'Log1p') else 1.5
    x = _data(UNARY[op][2], np.random.RandomState(_seed(op, 'fused')), (n,),
              dtype)
    feeds = {}
    p = _feed(feeds, x, dtype)
    op_name = _uniq('fz_' + op)
    out, on_gpu = _run_fused(
        sess, lambda exit_name: apply_op(
            'Add', apply_op(op, p, name=op_name), _const(c, dtype),
            name=exit_name), feeds)
    assert op_name not in on_gpu
    _check_tol('fused ' + op, dtype, out,
               UNARY[op][1](x.astype(np.float64)) + c)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('case,op,form', FUSED_BINARY,
                         ids=[c[0] for c in FUSED_BINARY])
def test_fused_binary_opcode(sess, case, op, form, dtype):
    n = 1027
    _, fn, dom_a, dom_b = BINARY[op]
    rng = np.random.RandomState(_seed(case, 'fused'))
    c_first, c_second = {'Pow': (2.5, 1.5), 'Div': (1.5, -0.75),
                         'RealDiv': (1.5, -0.75)}.get(op, (0.75, -1.25))
    x = _data(dom_b if form == 'cx' else dom_a, rng, (n,), dtype)
    feeds = {}
    p = _feed(feeds, x, dtype)
    x64 = x.astype(np.float64)
    if form == 'xc':
        args, ref = (p, _const(c_second, dtype)), fn(x64, c_second)
    elif form == 'cx':
        args, ref = (_const(c_first, dtype), p), fn(c_first, x64)
    else:
        args, ref = (p, p), fn(x64, x64)
    op_name = _uniq('fz_' + op)
    out, on_gpu = _run_fused(
        sess, lambda exit_name: apply_op(
            'Neg', apply_op(op, *args, name=op_name), name=exit_name), feeds)
    assert op_name not in on_gpu
    _check_tol('fused ' + case, dtype, out, -ref)


def test_softplus_fused_matches_unfused(sess):
    x = np.array([100.0, -100.0, 0.0, 3.0], np.float32)
    feeds = {}
    p = _feed(feeds, x, tf.float32)
    unfused = apply_op('Softplus', p)
    exit_name = _uniq('exit')
    fused = tf.identity(apply_op('Add', apply_op('Softplus', p),
                                 _const(0.0, tf.float32), name=exit_name))
    (out_u, out_f), on_gpu = _trace_run(sess, [unfused, fused], feeds)
    assert exit_name + '/_fused' in on_gpu, sorted(on_gpu)
    np.testing.assert_allclose(out_f, out_u, **F32_TOL)
    assert out_f[0] == 100.0 and out_u[0] == 100.0


def _flip_chain(p, length, dtype, exit_name):
    """`length` instructions alternating Neg and Add 1: each pair maps x to
    1 - x, every step is exact for the inputs below in f32 and in bf16."""
    t = p
    for k in range(length):
        name = exit_name if k == length - 1 else None
        if k % 2 == 0:
            t = apply_op('Neg', t, name=name)
        else:
            t = apply_op('Add', t, _const(1.0, dtype), name=name)
    return t


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('length', [24, 25])
def test_fused_chain_length(sess, length, dtype):
    """24 instructions (kMaxInstr) fuse into one node; 25 must still be
    right however the optimizer splits them. Inputs are multiples of 2^-5 in
    [2, 3], so x, -x and 1 - x are all exact in bf16 too and the unfused
    bf16 chain does not round either."""
    n = 1027
    rng = np.random.RandomState(95)
    x = (2 + rng.randint(0, 33, n) / 32.0).astype(np.float32)
    feeds = {}
    p = _feed(feeds, x, dtype)
    out, _ = _run_fused(
        sess, lambda exit_name: _flip_chain(p, length, dtype, exit_name),
        feeds, expect_fused=(length == 24))
    ref = x.astype(np.float64)
    for k in range(length):
        ref = -ref if k % 2 == 0 else ref + 1
    _check_tol('chain %d' % length, dtype, out, ref)


@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize('consts', [6, 7])
def test_fused_input_count(sess, consts, dtype):
    """The root plus six distinct scalar constants (kMaxInputs = 7) fuse
    into one node; seven constants must still be right. Small integers, so
    every partial sum is exact in bf16 as well."""
    n = 1027
    rng = np.random.RandomState(96)
    x = rng.randint(-64, 65, n).astype(np.float32)
    feeds = {}
    p = _feed(feeds, x, dtype)

    def build(exit_name):
        t = p
        for k in range(consts):
            t = apply_op('Add', t, _const(float(k + 1), dtype),
                         name=exit_name if k == consts - 1 else None)
        return t
    out, _ = _run_fused(sess, build, feeds, expect_fused=(consts == 6))
    _check_tol('%d constants' % consts, dtype, out,
               x.astype(np.float64) + sum(range(1, consts + 1)))


# ---------------------------------------------------------------------------
# the capped grid's second pass, one op per kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_second_pass(sess, dtype):
    rng = np.random.RandomState(97)
    rows = N_BIG // 3                      # N_BIG = 3 * 1398103
    x = _data('randn', rng, (N_BIG,), dtype)
    y = _data('randn', rng, (N_BIG,), dtype)
    col = _data('randn', rng, (rows, 1), dtype)
    c = np.float32(-1.25)
    feeds = {}
    px = _feed(feeds, x, dtype)
    py = _feed(feeds, y, dtype)
    exit_name = _uniq('exit')
    fetches = [
        apply_op('Relu', px),
        apply_op('Sub', px, py),
        apply_op('Sub', px, _feed(feeds, c, dtype)),
        apply_op('Sub', tf.reshape(px, [rows, 3]), _feed(feeds, col, dtype)),
        tf.identity(apply_op('Neg', apply_op('Mul', px, _const(1.5, dtype)),
                             name=exit_name)),
    ]
    if dtype == tf.float32:
        fetches.append(apply_op('Cast', px, DstT=tf.bfloat16))
    outs, on_gpu = _trace_run(sess, fetches, feeds)
    _check_unary('big Relu', 'Relu', dtype, outs[0], x)
    _check_binary('big Sub', 'Sub', dtype, outs[1], x, y)
    _check_binary('big Sub scalar', 'Sub', dtype, outs[2], x, np.asarray(c))
    _check_binary('big Sub bcast', 'Sub', dtype, outs[3],
                  x.reshape(rows, 3), col)
    assert exit_name + '/_fused' in on_gpu, sorted(on_gpu)
    _check_tol('big fused', dtype, outs[4], -(x.astype(np.float64) * 1.5))
    if dtype == tf.float32:
        _check_exact('big Cast', tf.float32, outs[5], _bf16(x))


def test_empty(sess):
    """n = 0: an empty output and no error."""
    e = np.zeros((0,), np.float32)
    feeds = {}
    p = _feed(feeds, e, tf.float32)
    fetches = [apply_op('Relu', p),
               apply_op('Sub', p, _feed(feeds, e, tf.float32)),
               apply_op('Cast', p, DstT=tf.bfloat16)]
    outs = sess.run(fetches, feeds)
    for out in outs:
        assert out.shape == (0,)


# ---------------------------------------------------------------------------
# 7. placement: the ops above really run on the GPU
# ---------------------------------------------------------------------------
def test_elementwise_ops_run_on_gpu(sess):
    rng = np.random.RandomState(98)
    feeds = {}
    x = _feed(feeds, _data('randn', rng, (6, 5), tf.float32), tf.float32)
    y = _feed(feeds, _data('randn', rng, (6, 5), tf.float32), tf.float32)
    row = _feed(feeds, _data('randn', rng, (5,), tf.float32), tf.float32)
    c = _feed(feeds, np.float32(0.5), tf.float32)
    idx = _feed(feeds, np.array([1, 0, 3], np.int32), tf.int32)
    mask = _feed(feeds, np.array([True, False, True]), tf.bool)
    dims = _feed(feeds, np.array([13, 79], np.int32), tf.int32)
    fetches = [
        apply_op('Tanh', x, name='e_unary'),
        apply_op('Sub', x, y, name='e_same'),
        apply_op('Sub', x, c, name='e_scalar'),
        apply_op('Sub', x, row, name='e_bcast'),
        apply_op('Cast', idx, DstT=tf.int64, name='e_cast_i'),
        apply_op('Cast', mask, DstT=tf.float32, name='e_cast_b'),
        apply_op('AddN', [x, y, x], name='e_addn'),
        apply_op('Fill', dims, c, name='e_fill'),
        apply_op('ZerosLike', x, name='e_zeros'),
    ]
    _, on_gpu = _trace_run(sess, fetches, feeds)
    for name in ('e_unary', 'e_same', 'e_scalar', 'e_bcast', 'e_cast_i',
                 'e_cast_b', 'e_addn', 'e_fill', 'e_zeros'):
        assert name in on_gpu, (name, sorted(on_gpu))
