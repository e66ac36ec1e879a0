"""The quantized ops on the GPU (csrc/kernels/hip/gemm_i8.hip and
quantized.hip through csrc/kernels/gpu_quantized.cc) against the CPU kernels
(csrc/kernels/cpu_quantized.cc).

Each case builds the op twice in one graph, under /cpu:0 and under /gpu:0,
feeds both the same placeholders and requires np.array_equal on every output,
the two range scalars included: the GPU arithmetic is integer (wrapping
32-bit) where the CPU's is, and the same IEEE operations in the same order
where it is floating point. Activations always come through placeholders, so
constant folding cannot run an op on the CPU; the placement test checks in a
trace that the GPU copies really ran on the GPU. All tests need a gfx950 GPU.
"""
import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.ops import quantized_ops as q

from test_gpu_kernels import _sess
from test_quantized_conv import CASES as CPU_CONV_CASES

pytestmark = pytest.mark.gpu

RANGES = [(-1.0, 1.0), (0.0, 6.0), (0.5, 4.0), (-4.0, -0.5)]
SIZES = (1, 7, 1027, 65536 + 3)


@pytest.fixture(scope='module')
def sess():
    """One graph and one session for the module; every test only adds
    nodes."""
    tf.reset_default_graph()
    with _sess() as s:
        yield s


def _on_both(build):
    """build() -> list of tensors; once per device."""
    with tf.device('/cpu:0'):
        cpu = list(build())
    with tf.device('/gpu:0'):
        gpu = list(build())
    return cpu, gpu


def _check_equal(sess, build, feeds, what):
    cpu, gpu = _on_both(build)
    outs = sess.run(cpu + gpu, feeds)
    n = len(cpu)
    for i in range(n):
        c, g = outs[i], outs[n + i]
        assert c.dtype == g.dtype and c.shape == g.shape, (what, i)
        if not np.array_equal(c, g):
            bad = np.flatnonzero(np.asarray(c).ravel() !=
                                 np.asarray(g).ravel())
            raise AssertionError(
                '%s output %d: %d of %d differ, first at %d: cpu %r gpu %r'
                % (what, i, bad.size, np.asarray(c).size, bad[0],
                   np.asarray(c).ravel()[bad[0]],
                   np.asarray(g).ravel()[bad[0]]))
    return outs[:n]


# ---------------------------------------------------------------------------
# QuantizedMatMul
# ---------------------------------------------------------------------------
# (M, N, K, transpose_a, transpose_b)
MATMUL_SHAPES = (
    [(1, 1, 1, False, False)] +
    [(17, 19, 65, ta, tb) for ta in (False, True) for tb in (False, True)] +
    [(128, 128, 64, False, False), (130, 72, 200, False, False),
     (64, 48, 4096, False, False),
     # K % 16 == 0 but K % 64 != 0: A is staged unpacked, with a K tail
     (33, 40, 80, False, False),
     # an empty output still gets its ranges
     (0, 19, 16, False, False)])


def _matmul_id(p):
    return '%dx%dx%d%s%s' % (p[0], p[1], p[2], '_ta' if p[3] else '',
                             '_tb' if p[4] else '')


@pytest.mark.parametrize('fill', ['random', 'all255', 'all0'])
@pytest.mark.parametrize('shape', MATMUL_SHAPES,
                         ids=[_matmul_id(p) for p in MATMUL_SHAPES])
def test_quantized_matmul(sess, shape, fill):
    m, n, k, ta, tb = shape
    idx = MATMUL_SHAPES.index(shape)
    a_shape = (k, m) if ta else (m, k)
    b_shape = (n, k) if tb else (k, n)
    rng = np.random.RandomState(100 + idx)
    if fill == 'random':
        a = rng.randint(0, 256, a_shape).astype(np.uint8)
        b = rng.randint(0, 256, b_shape).astype(np.uint8)
        # the four ranges, mixed across A and B
        ra = RANGES[idx % 4]
        rb = RANGES[(idx // 4 + idx + 1) % 4]
    elif fill == 'all255':
        a = np.full(a_shape, 255, np.uint8)
        b = np.full(b_shape, 255, np.uint8)
        ra, rb = (0.0, 6.0), (0.0, 2.5)
    else:
        a = np.zeros(a_shape, np.uint8)
        b = np.zeros(b_shape, np.uint8)
        ra, rb = (-6.0, 0.0), (-2.5, 0.0)
    pa = tf.placeholder(tf.uint8, a_shape)
    pb = tf.placeholder(tf.uint8, b_shape)
    outs = _check_equal(
        sess, lambda: q.quantized_matmul(pa, pb, ra[0], ra[1], rb[0], rb[1],
                                         transpose_a=ta, transpose_b=tb),
        {pa: a, pb: b}, 'QuantizedMatMul')
    assert outs[0].shape == (m, n) and outs[0].dtype == np.int32


@pytest.mark.parametrize('a_shape, b_shape, match', [
    ((2, 3), (4, 2), 'inner dim'), ((3,), (3, 2), 'matrices')])
def test_quantized_matmul_rejects_bad_shapes(sess, a_shape, b_shape, match):
    """The shape check fails the op before any kernel is launched."""
    pa = tf.placeholder(tf.uint8, a_shape)
    pb = tf.placeholder(tf.uint8, b_shape)
    with tf.device('/gpu:0'):
        out = q.quantized_matmul(pa, pb, 0.0, 1.0, 0.0, 1.0)[0]
    # a session of its own, on the module's graph (hence the fixture): the
    # failed run must not be the shared session's
    with _sess() as s:
        with pytest.raises(tf.errors.InvalidArgumentError, match=match):
            s.run(out, {pa: np.zeros(a_shape, np.uint8),
                        pb: np.zeros(b_shape, np.uint8)})


# ---------------------------------------------------------------------------
# QuantizedConv2D
# ---------------------------------------------------------------------------
GPU_CONV_CASES = CPU_CONV_CASES + [
    # implicit path, full tiles
    ('implicit_16x16x64', (1, 16, 16, 64), (3, 3, 64, 64), [1, 1, 1, 1],
     'SAME', (-1.0, 1.0), (0.0, 6.0)),
    ('implicit_1x1', (1, 8, 8, 64), (1, 1, 64, 64), [1, 1, 1, 1], 'SAME',
     (0.0, 6.0), (-1.0, 1.0)),
    # M = 32 and N = 24 are tile tails
    ('implicit_tails_s2', (2, 7, 7, 32), (3, 3, 32, 24), [1, 2, 2, 1], 'SAME',
     (-1.0, 1.0), (-1.0, 1.0)),
    # C % 16 != 0: the column-matrix path
    ('im2col_c20', (1, 10, 10, 20), (3, 3, 20, 8), [1, 1, 1, 1], 'SAME',
     (-1.0, 1.0), (0.5, 4.0)),
    # border correction under the MFMA path, zero points no byte can hold
    ('implicit_negative_zero_point', (1, 16, 16, 16), (3, 3, 16, 16),
     [1, 1, 1, 1], 'SAME', (0.5, 4.0), (-1.0, 1.0)),
    ('implicit_zero_point_above_255', (1, 16, 16, 16), (3, 3, 16, 16),
     [1, 1, 1, 1], 'SAME', (-4.0, -0.5), (-1.0, 1.0)),
]


@pytest.mark.parametrize('case', GPU_CONV_CASES,
                         ids=[c[0] for c in GPU_CONV_CASES])
def test_quantized_conv2d(sess, case):
    _, xs, ws, strides, padding, in_range, f_range = case
    rng = np.random.RandomState(7)
    x = rng.randint(0, 256, xs).astype(np.uint8)
    w = rng.randint(0, 256, ws).astype(np.uint8)
    px = tf.placeholder(tf.uint8, xs)
    pw = tf.placeholder(tf.uint8, ws)
    outs = _check_equal(
        sess, lambda: q.quantized_conv2d(px, pw, in_range[0], in_range[1],
                                         f_range[0], f_range[1], strides,
                                         padding),
        {px: x, pw: w}, 'QuantizedConv2D')
    assert outs[0].dtype == np.int32


# ---------------------------------------------------------------------------
# elementwise and range ops
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_quantize_v2(sess, n):
    rng = np.random.RandomState(n)
    # range (0, 255): scale is exactly 1, so k + 0.5 sits exactly on a
    # rounding boundary; some values lie outside the range
    halves = (rng.randint(-3, 259, n) + 0.5).astype(np.float32)
    halves[::5] = rng.randint(-3, 259, halves[::5].shape)
    px = tf.placeholder(tf.float32, (n,))
    _check_equal(sess, lambda: q.quantize_v2(px, 0.0, 255.0), {px: halves},
                 'QuantizeV2 halves')
    # a step that is not a power of two; boundaries hit through the f32
    # product, values outside on both sides
    x = rng.uniform(-1.5, 1.5, n).astype(np.float32)
    step = np.float32(2.0) / np.float32(255.0)
    x[::3] = (np.float32(-1.0) +
              (rng.randint(0, 255, x[::3].shape) + 0.5).astype(np.float32)
              * step)
    for mn, mx in [(-1.0, 1.0), (0.5, 4.0)]:
        _check_equal(sess, lambda: q.quantize_v2(px, mn, mx), {px: x},
                     'QuantizeV2 (%g, %g)' % (mn, mx))


@pytest.mark.parametrize('n', SIZES)
def test_dequantize_both_carriers(sess, n):
    rng = np.random.RandomState(n)
    u = rng.randint(0, 256, n).astype(np.uint8)
    pu = tf.placeholder(tf.uint8, (n,))
    for mn, mx in RANGES:
        _check_equal(sess, lambda: [q.dequantize(pu, mn, mx)], {pu: u},
                     'Dequantize u8 (%g, %g)' % (mn, mx))
    i = rng.randint(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    i[:2] = [-2 ** 31, 2 ** 31 - 1][:n]
    pi = tf.placeholder(tf.int32, (n,))
    for mn, mx in [(-1000.0, 1000.0), (-3.0, 50.0), (-131586.0, 131586.0)]:
        _check_equal(sess, lambda: [q.dequantize(pi, mn, mx)], {pi: i},
                     'Dequantize i32 (%g, %g)' % (mn, mx))


@pytest.mark.parametrize('n', SIZES)
def test_quantized_relu(sess, n):
    u = np.random.RandomState(n).randint(0, 256, n).astype(np.uint8)
    pu = tf.placeholder(tf.uint8, (n,))
    for mn, mx in RANGES:
        _check_equal(sess, lambda: q.quantized_relu(pu, mn, mx), {pu: u},
                     'QuantizedRelu (%g, %g)' % (mn, mx))


def _int32_data(kind, n, seed):
    rng = np.random.RandomState(seed)
    if kind == 'positive':
        return rng.randint(1, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    if kind == 'negative':
        return rng.randint(-2 ** 31, 0, n, dtype=np.int64).astype(np.int32)
    return rng.randint(-2 ** 24, 2 ** 24, n, dtype=np.int64).astype(np.int32)


@pytest.mark.parametrize('kind', ['positive', 'negative', 'mixed'])
@pytest.mark.parametrize('n', SIZES)
def test_range_ops(sess, n, kind):
    x = _int32_data(kind, n, n)
    pi = tf.placeholder(tf.int32, (n,))
    for mn, mx in [(-1000.0, 1000.0), (-3.0, 50.0)]:
        _check_equal(sess, lambda: q.requantization_range(pi, mn, mx),
                     {pi: x}, 'RequantizationRange %s' % kind)
        _check_equal(sess,
                     lambda: q.quantize_down_and_shrink_range(pi, mn, mx),
                     {pi: x}, 'QuantizeDownAndShrinkRange %s' % kind)


# ---------------------------------------------------------------------------
# placement: the whole chain runs on the GPU, repeatedly
# ---------------------------------------------------------------------------
def _trace_run(sess, fetches, feeds):
    """test_gpu_elementwise._trace_run's idiom: names of the nodes that ran
    on a GPU."""
    opts = tf.RunOptions(trace_level=tf.RunOptions.FULL_TRACE)
    md = tf.RunMetadata()
    outs = sess.run(fetches, feeds, options=opts, run_metadata=md)
    on_gpu = {ns.node_name for ds in md.step_stats.dev_stats
              if 'GPU' in ds.device.upper() for ns in ds.node_stats}
    return outs, on_gpu


CHAIN_OPS = ['quantize', 'conv', 'down', 'relu', 'matmul', 'range',
             'dequantize']


def _chain(prefix, px, pw, pb):
    qx, mn, mx = q.quantize_v2(px, -1.0, 1.0, name=prefix + 'quantize')
    qc, mnc, mxc = q.quantized_conv2d(qx, pw, mn, mx, -1.0, 1.0, [1, 1, 1, 1],
                                      'SAME', name=prefix + 'conv')
    q8, mn8, mx8 = q.quantize_down_and_shrink_range(qc, mnc, mxc,
                                                    name=prefix + 'down')
    qr, mnr, mxr = q.quantized_relu(q8, mn8, mx8, name=prefix + 'relu')
    flat = tf.reshape(qr, [2, 8 * 8 * 16])
    qm, mnm, mxm = q.quantized_matmul(flat, pb, mnr, mxr, 0.0, 6.0,
                                      name=prefix + 'matmul')
    rmin, rmax = q.requantization_range(qm, mnm, mxm, name=prefix + 'range')
    deq = q.dequantize(qm, mnm, mxm, name=prefix + 'dequantize')
    return [qm, rmin, rmax, deq, q8, mn8, mx8]


def test_chain_runs_on_the_gpu(sess):
    px = tf.placeholder(tf.float32, (2, 8, 8, 16))
    pw = tf.placeholder(tf.uint8, (3, 3, 16, 16))
    pb = tf.placeholder(tf.uint8, (8 * 8 * 16, 10))
    with tf.device('/cpu:0'):
        cpu = _chain('qchain_cpu_', px, pw, pb)
    with tf.device('/gpu:0'):
        gpu = _chain('qchain_gpu_', px, pw, pb)
    rng = np.random.RandomState(3)

    def feeds():
        return {px: rng.uniform(-1.2, 1.2, (2, 8, 8, 16)).astype(np.float32),
                pw: rng.randint(0, 256, (3, 3, 16, 16)).astype(np.uint8),
                pb: rng.randint(0, 256, (8 * 8 * 16, 10)).astype(np.uint8)}

    def check(outs):
        n = len(cpu)
        for i in range(n):
            assert np.array_equal(outs[i], outs[n + i]), i

    outs, on_gpu = _trace_run(sess, cpu + gpu, feeds())
    for op in CHAIN_OPS:
        assert 'qchain_gpu_' + op in on_gpu, (op, sorted(on_gpu))
        assert 'qchain_cpu_' + op not in on_gpu, (op, sorted(on_gpu))
    check(outs)
    # the same run again and again, past the point where the step is
    # captured and replayed
    results = []
    for _ in range(5):
        outs = sess.run(cpu + gpu, feeds())
        check(outs)
        results.append(outs[0])
    assert any(not np.array_equal(results[0], r) for r in results[1:])
