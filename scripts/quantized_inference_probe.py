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

Needs a GPU; run it under a time limit:
  timeout 600 python scripts/quantized_inference_probe.py
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simple_tensorflow_amd as tf  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lo', type=int, default=4)
    ap.add_argument('--hi', type=int, default=44)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    args = ap.parse_args()

    sess = tf.Session()
    assert sess.num_gpus() > 0, 'the probe needs a GPU'
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
