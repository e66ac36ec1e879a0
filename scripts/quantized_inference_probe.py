"""Times the memory-bound kernels of the quantized inference path against the
existing kernels they stand beside, all at the shape (32,56,56,64):

  Requantize        vs QuantizeDownAndShrinkRange, on the int32 output of a
                       3x3x64x64 QuantizedConv2D (one pass against two);
  QuantizedMaxPool  vs the bf16 MaxPool, 3x3 stride 2 SAME (half the bytes);
  QuantizedBiasAdd  vs the f32 BiasAdd.

Prints a markdown table. The method is that of quantized_gemm_probe.py: one
graph holds `reps` copies of the op chained by control dependencies, run as
a single step that ends in a device synchronise; the step is timed at two
values of `reps`, and the per-op time is the difference of the two medians
over the difference in copies, which cancels the per-step host cost and the
ops that prepare the operands (they run once per step). The two chain
lengths are timed in three alternating rounds; the table gives the median
over the rounds, and the lowest and highest round as the spread against
which a ratio is to be read.

With --fused it times one quantized layer instead, and nothing else: the
chain QuantizedConv2D -> Requantize -> QuantizedBiasAdd -> Requantize ->
QuantizedRelu (constant requested ranges) against the one
QuantizedConv2DWithBiasAndRequantize, at the shape above with a 3x3x64x64
filter, with the bf16 Conv2D beside them for orientation; and the same pair
for a MatMul at (256*14*14, 256, 2304). The chain, the fused op and the bf16
op take turns inside each of five rounds.

With --fused-sum it times the closing conv of a ResNet stage-2 bottleneck
block with its residual sum, (32,56,56,64) * 1x1x64x256 plus a
(32,56,56,256) shortcut, Relu, in three forms: what quantize_nodes(
fuse_epilogue=True) makes of Conv2D -> BiasAdd -> Add -> Relu without
fuse_sum (the fused conv, two Dequantize, the f32 Add, the
Reshape/Min/Max/QuantizeV2 group and QuantizedRelu), the plain fused conv
alone, and the one QuantizedConv2DWithBiasSumAndRequantize. --tree DIR loads
the package from another checkout, so that the chain can be timed on a build
of the parent commit in a process of its own; a package without the sum op
times the first two forms only.

Needs a GPU; run it under a time limit:
  timeout 600 python scripts/quantized_inference_probe.py
"""
import argparse
import os
import sys
import time

import numpy as np

# --tree DIR: the checkout whose package is loaded, this one by default
_TREE = sys.argv[sys.argv.index('--tree') + 1] if '--tree' in sys.argv else \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _TREE)

import simple_tensorflow_amd as tf  # noqa: E402
from simple_tensorflow_amd.python.framework.ops import apply_op  # noqa: E402
from simple_tensorflow_amd.python.ops import quantized_ops as q  # noqa: E402

SHAPE = (32, 56, 56, 64)
FILTER = (3, 3, 64, 64)
POOL = dict(ksize=[1, 3, 3, 1], strides=[1, 2, 2, 1], padding='SAME')


def _chained(make, reps):
    """`reps` copies of make() in sequence; returns an op to run."""
    prev, outs = None, []
    for _ in range(reps):
        if prev is None:
            t = make()
        else:
            with tf.control_dependencies([prev]):
                t = make()
        prev = t.op
        outs.append(t.op)
    return tf.group(*outs)


def _median_step(sess, op, warmup, iters):
    for _ in range(warmup):
        sess.run(op)
    sess.sync()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        sess.run(op)
        sess.sync()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


def _per_op_seconds(sess, make, lo, hi, warmup, iters, rounds=3):
    """(median, lowest, highest) per-op time over the alternating rounds."""
    with tf.device('/gpu:0'):
        op_lo = _chained(make, lo)
        op_hi = _chained(make, hi)
    per_op = []
    for _ in range(rounds):
        # alternate the two so drift hits both alike
        t_lo = _median_step(sess, op_lo, warmup, iters)
        t_hi = _median_step(sess, op_hi, warmup, iters)
        print('#   step medians: %d copies %.3f ms, %d copies %.3f ms'
              % (lo, t_lo * 1e3, hi, t_hi * 1e3), file=sys.stderr,
              flush=True)
        per_op.append((t_hi - t_lo) / (hi - lo))
    return float(np.median(per_op)), min(per_op), max(per_op)


def _cases():
    n = int(np.prod(SHAPE))
    pooled = SHAPE[0] * 28 * 28 * SHAPE[3]
    with tf.device('/gpu:0'):
        x = tf.Variable(tf.random_uniform(SHAPE, -1.0, 1.0))
        w = tf.Variable(tf.random_uniform(FILTER, -1.0, 1.0))
        b = tf.Variable(tf.random_uniform((SHAPE[3],), -1.0, 1.0))
        x8, xmn, xmx = q.quantize_v2(x, -1.0, 1.0)
        w8, wmn, wmx = q.quantize_v2(w, -1.0, 1.0)
        b8, bmn, bmx = q.quantize_v2(b, -1.0, 1.0)
        x16 = tf.cast(x, tf.bfloat16)
        c32, cmn, cmx = q.quantized_conv2d(x8, w8, xmn, xmx, wmn, wmx,
                                           [1, 1, 1, 1], 'SAME')
        rmn, rmx = q.requantization_range(c32, cmn, cmx)
    # (case, new op, bytes it moves, yardstick, yardstick op, its bytes)
    return [
        ('qint32 -> quint8',
         'Requantize', lambda: q.requantize(c32, cmn, cmx, rmn, rmx)[0],
         5 * n,
         'QuantizeDownAndShrinkRange',
         lambda: q.quantize_down_and_shrink_range(c32, cmn, cmx)[0], 9 * n),
        ('max pool 3x3/2',
         'QuantizedMaxPool',
         lambda: q.quantized_max_pool(x8, xmn, xmx, **POOL)[0], n + pooled,
         'MaxPool bf16', lambda: tf.nn.max_pool(x16, **POOL),
         2 * (n + pooled)),
        ('bias add',
         'QuantizedBiasAdd',
         lambda: q.quantized_bias_add(x8, b8, xmn, xmx, bmn, bmx)[0], 5 * n,
         'BiasAdd f32', lambda: tf.nn.bias_add(x, b), 8 * n),
    ]


# ---------------------------------------------------------------------------
# --fused: one quantized layer as the chain of five ops against the fused op
# ---------------------------------------------------------------------------
GEMM = (256 * 14 * 14, 256, 2304)  # quantized_gemm_probe.py's stage shape
REQ = (-8.0, 8.0)                   # the constant requested range


def _layer_chain(acc):
    """Requantize -> QuantizedBiasAdd -> Requantize -> QuantizedRelu behind
    the qint32 triple acc, with constant requested ranges."""
    def make(b8, bmn, bmx):
        c8, mn, mx = q.requantize(acc[0], acc[1], acc[2], REQ[0], REQ[1])
        s32, smn, smx = q.quantized_bias_add(c8, b8, mn, mx, bmn, bmx)
        s8, mn, mx = q.requantize(s32, smn, smx, REQ[0], REQ[1])
        return q.quantized_relu(s8, mn, mx)[0]
    return make


def _fused_cases():
    """(case, chain, fused op, bf16 op or None)."""
    m, n, k = GEMM
    with tf.device('/gpu:0'):
        x = tf.Variable(tf.random_uniform(SHAPE, -1.0, 1.0))
        w = tf.Variable(tf.random_uniform(FILTER, -1.0, 1.0))
        b = tf.Variable(tf.random_uniform((FILTER[3],), -1.0, 1.0))
        a = tf.Variable(tf.random_uniform((m, k), -1.0, 1.0))
        wm = tf.Variable(tf.random_uniform((k, n), -1.0, 1.0))
        bm = tf.Variable(tf.random_uniform((n,), -1.0, 1.0))
        x8, w8, b8 = [q.quantize_v2(t, -1.0, 1.0) for t in (x, w, b)]
        a8, wm8, bm8 = [q.quantize_v2(t, -1.0, 1.0) for t in (a, wm, bm)]
        x16, w16 = tf.cast(x, tf.bfloat16), tf.cast(w, tf.bfloat16)

    def conv_chain():
        acc = q.quantized_conv2d(x8[0], w8[0], x8[1], x8[2], w8[1], w8[2],
                                 [1, 1, 1, 1], 'SAME')
        return _layer_chain(acc)(*b8)

    def conv_fused():
        return q.quantized_conv2d_with_bias_and_requantize(
            x8[0], w8[0], b, x8[1], x8[2], w8[1], w8[2], REQ[0], REQ[1],
            [1, 1, 1, 1], 'SAME', activation='Relu')[0]

    def matmul_chain():
        acc = q.quantized_matmul(a8[0], wm8[0], a8[1], a8[2], wm8[1], wm8[2])
        return _layer_chain(acc)(*bm8)

    def matmul_fused():
        return q.quantized_matmul_with_bias_and_requantize(
            a8[0], wm8[0], bm, a8[1], a8[2], wm8[1], wm8[2], REQ[0], REQ[1],
            activation='Relu')[0]

    return [('conv %s * %s' % (SHAPE, FILTER), conv_chain, conv_fused,
             lambda: tf.nn.conv2d(x16, w16, [1, 1, 1, 1], 'SAME')),
            ('matmul %dx%dx%d' % GEMM, matmul_chain, matmul_fused, None)]


def _alternating(sess, makes, lo, hi, warmup, iters, rounds=5):
    """Per-op seconds of each make, one list per make with a value per
    round; the makes take turns inside every round."""
    ops = []
    for make in makes:
        with tf.device('/gpu:0'):
            ops.append((_chained(make, lo), _chained(make, hi)))
    per_op = [[] for _ in makes]
    for _ in range(rounds):
        for i, (op_lo, op_hi) in enumerate(ops):
            t_lo = _median_step(sess, op_lo, warmup, iters)
            t_hi = _median_step(sess, op_hi, warmup, iters)
            per_op[i].append((t_hi - t_lo) / (hi - lo))
    return per_op


def _fused_main(sess, args):
    cases = _fused_cases()
    sess.run(tf.global_variables_initializer())
    if args.profile:  # for a kernel trace: a few runs of each, no timing
        for _, chain, fused, _ in cases:
            for make in (chain, fused):
                with tf.device('/gpu:0'):
                    op = _chained(make, 4)
                for _ in range(3):
                    sess.run(op)
                sess.sync()
        return
    print('| case | five-op chain us (rounds) | fused op us (rounds) | '
          'chain / fused (rounds) | bf16 us |')
    print('|---|---|---|---|---|')
    for case, chain, fused, bf16 in cases:
        makes = [chain, fused] + ([bf16] if bf16 else [])
        t = _alternating(sess, makes, args.lo, args.hi, args.warmup,
                         args.iters)
        us = [[v * 1e6 for v in r] for r in t]
        ratio = [c / f for c, f in zip(us[0], us[1])]
        print('| %s | %.1f (%.1f-%.1f) | %.1f (%.1f-%.1f) | '
              '%.2f (%.2f-%.2f) | %s |'
              % (case, np.median(us[0]), min(us[0]), max(us[0]),
                 np.median(us[1]), min(us[1]), max(us[1]), np.median(ratio),
                 min(ratio), max(ratio),
                 '%.1f' % np.median(us[2]) if bf16 else '-'), flush=True)


# ---------------------------------------------------------------------------
# --fused-sum: the closing conv of a bottleneck block with its residual sum
# ---------------------------------------------------------------------------
SUM_FILTER = (1, 1, 64, 256)
HAS_SUM = hasattr(q, 'quantized_conv2d_with_bias_sum_and_requantize')


def _sum_makes():
    """[(name, make)]: the unfused chain, the plain fused conv, the sum op."""
    short_shape = SHAPE[:3] + (SUM_FILTER[3],)
    with tf.device('/gpu:0'):
        x = tf.Variable(tf.random_uniform(SHAPE, -1.0, 1.0))
        w = tf.Variable(tf.random_uniform(SUM_FILTER, -1.0, 1.0))
        b = tf.Variable(tf.random_uniform((SUM_FILTER[3],), -1.0, 1.0))
        sc = tf.Variable(tf.random_uniform(short_shape, 0.0, 4.0))
        x8, w8 = [q.quantize_v2(t, -1.0, 1.0) for t in (x, w)]
        s8 = q.quantize_v2(sc, REQ[0], REQ[1])

    def conv(activation):
        return q.quantized_conv2d_with_bias_and_requantize(
            x8[0], w8[0], b, x8[1], x8[2], w8[1], w8[2], REQ[0], REQ[1],
            [1, 1, 1, 1], 'VALID', activation=activation)

    def chain():
        y = tf.add(q.dequantize(*conv('None')), q.dequantize(*s8))
        flat = tf.reshape(y, [-1])
        # the wrapper takes constants only; the range is measured here
        y8 = apply_op('QuantizeV2', y, tf.reduce_min(flat, [0]),
                      tf.reduce_max(flat, [0]), mode='MIN_COMBINED')
        return q.quantized_relu(*y8)[0]

    def fused_sum():
        return q.quantized_conv2d_with_bias_sum_and_requantize(
            x8[0], w8[0], b, s8[0], x8[1], x8[2], w8[1], w8[2], s8[1], s8[2],
            REQ[0], REQ[1], [1, 1, 1, 1], 'VALID', activation='Relu')[0]

    makes = [('chain', chain), ('fused conv', lambda: conv('Relu')[0])]
    return makes + ([('fused sum', fused_sum)] if HAS_SUM else [])


def _fused_sum_main(sess, args):
    makes = _sum_makes()
    sess.run(tf.global_variables_initializer())
    if args.profile:  # for a kernel trace: a few runs of each, no timing
        for _, make in makes:
            with tf.device('/gpu:0'):
                op = _chained(make, 4)
            for _ in range(3):
                sess.run(op)
            sess.sync()
        return
    t = _alternating(sess, [m for _, m in makes], args.lo, args.hi,
                     args.warmup, args.iters)
    print('| tree | form | us, median (rounds) |')
    print('|---|---|---|')
    for (name, _), r in zip(makes, t):
        us = [v * 1e6 for v in r]
        print('| %s | %s | %.1f (%s) |'
              % (_TREE, name, np.median(us),
                 ', '.join('%.1f' % v for v in us)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lo', type=int, default=4)
    ap.add_argument('--hi', type=int, default=44)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--fused', action='store_true',
                    help='time one quantized layer as the chain of five ops '
                         'against the fused op, and nothing else')
    ap.add_argument('--fused-sum', action='store_true',
                    help='time the conv + residual sum + Relu of a '
                         'bottleneck block as the unfused chain, the plain '
                         'fused conv and the fused-sum op, and nothing else')
    ap.add_argument('--tree', default=_TREE,
                    help='the checkout whose package is loaded (a build of '
                         'the parent commit as the yardstick)')
    ap.add_argument('--profile', action='store_true',
                    help='with --fused or --fused-sum: run each form a few '
                         'times and exit, for rocprofv3 --kernel-trace '
                         '--stats in a run of its own')
    args = ap.parse_args()

    sess = tf.Session()
    assert sess.num_gpus() > 0, 'the probe needs a GPU'
    if args.fused:
        return _fused_main(sess, args)
    if args.fused_sum:
        return _fused_sum_main(sess, args)
    cases = _cases()
    sess.run(tf.global_variables_initializer())

    def timed(make):
        return _per_op_seconds(sess, make, args.lo, args.hi, args.warmup,
                               args.iters)

    def cell(t, nbytes):
        return '%.1f (%.1f-%.1f) | %.2f' % (t[0] * 1e6, t[1] * 1e6,
                                            t[2] * 1e6, nbytes / t[0] / 1e12)

    print('| case | op | us (rounds) | TB/s | yardstick | us (rounds) | TB/s '
          '| time ratio (rounds) |')
    print('|---|---|---|---|---|---|---|---|')
    for case, name, make, nbytes, yname, ymake, ybytes in cases:
        t, y = timed(make), timed(ymake)
        print('| %s | %s | %s | %s | %s | %.2f (%.2f-%.2f) |'
              % (case, name, cell(t, nbytes), yname, cell(y, ybytes),
                 t[0] / y[0], t[1] / y[2], t[2] / y[1]), flush=True)


if __name__ == '__main__':
    main()
