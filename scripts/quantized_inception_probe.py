"""Times QuantizedConcat, QuantizedAvgPool and QuantizedRelu6 against the
kernels they stand beside, at batch 32 and Inception-v3 shapes:

  QuantizedConcat   of (32,35,35,{64,64,96,32}) on axis 3, once with four
                    different ranges (every input is requantized) and once
                    with four equal ranges (every input is copied), vs the
                    f32 ConcatV2 of the same shapes;
  QuantizedAvgPool  3x3 stride 1 SAME on (32,35,35,192) and 8x8 VALID on
                    (32,8,8,2048), vs the bf16 AvgPool, the dtype
                    models/inception.py pools in;
  QuantizedRelu6    vs QuantizedRelu at (32,56,56,64).

Prints a markdown table. The method is that of quantized_inference_probe.py:
one graph holds `reps` copies of the op chained by control dependencies, run
as a single step that ends in a device synchronise; the step is timed at two
values of `reps`, and the per-op time is the difference of the two medians
over the difference in copies. The two chain lengths are timed in three
alternating rounds; the table gives the median over the rounds, and the
lowest and highest round as the spread against which a ratio is to be read.

Needs a GPU; it is one GPU process. Run it under a time limit:
  timeout 600 python scripts/quantized_inception_probe.py
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simple_tensorflow_amd as tf  # noqa: E402
from simple_tensorflow_amd.python.framework.ops import apply_op  # noqa: E402
from simple_tensorflow_amd.python.ops import quantized_ops as q  # noqa: E402
from quantized_inference_probe import _per_op_seconds  # noqa: E402

BATCH = 32
MIXED = (BATCH, 35, 35)
WIDTHS = (64, 64, 96, 32)
DIFFERENT = [(-1.0, 1.0), (0.0, 6.0), (-2.0, 3.0), (-0.5, 4.0)]
EQUAL = [(-1.0, 1.0)] * 4
POOL3 = dict(ksize=[1, 3, 3, 1], strides=[1, 1, 1, 1], padding='SAME')
POOL8 = dict(ksize=[1, 8, 8, 1], strides=[1, 1, 1, 1], padding='VALID')
POOL3_SHAPE = (BATCH, 35, 35, 192)
POOL8_SHAPE = (BATCH, 8, 8, 2048)
RELU_SHAPE = (BATCH, 56, 56, 64)


def _cases():
    with tf.device('/gpu:0'):
        parts = [tf.Variable(tf.random_uniform(MIXED + (c,), -1.0, 1.0))
                 for c in WIDTHS]
        different = [q.quantize_v2(p, *r) for p, r in zip(parts, DIFFERENT)]
        equal = [q.quantize_v2(p, *r) for p, r in zip(parts, EQUAL)]
        x3 = tf.Variable(tf.random_uniform(POOL3_SHAPE, -1.0, 1.0))
        x8 = tf.Variable(tf.random_uniform(POOL8_SHAPE, -1.0, 1.0))
        xr = tf.Variable(tf.random_uniform(RELU_SHAPE, -1.0, 1.0))
        q3, q3mn, q3mx = q.quantize_v2(x3, -1.0, 1.0)
        q8, q8mn, q8mx = q.quantize_v2(x8, -1.0, 1.0)
        # 6.0 lies inside the range: both of Relu6's clamps bind
        qr, qrmn, qrmx = q.quantize_v2(xr, -1.0, 10.0)
        b3 = tf.cast(x3, tf.bfloat16)
        b8 = tf.cast(x8, tf.bfloat16)

    # the axis is a host-memory input of both concats: a Const on the CPU,
    # as the transformed graphs have it, costs no device-to-host copy
    with tf.device('/cpu:0'):
        axis = tf.constant(3)

    def concat(triples):
        return lambda: q.quantized_concat(
            axis, [t[0] for t in triples], [t[1] for t in triples],
            [t[2] for t in triples])[0]

    n_cat = int(np.prod(MIXED)) * sum(WIDTHS)
    n3 = int(np.prod(POOL3_SHAPE))
    n8, n8_out = int(np.prod(POOL8_SHAPE)), BATCH * 2048
    nr = int(np.prod(RELU_SHAPE))
    f32_concat = ('ConcatV2 f32',
                  lambda: apply_op('ConcatV2', parts, axis), 8 * n_cat)
    # (case, new op, bytes it moves, yardstick, yardstick op, its bytes)
    return [
        ('concat, 4 ranges', 'QuantizedConcat', concat(different),
         2 * n_cat) + f32_concat,
        ('concat, 1 range', 'QuantizedConcat', concat(equal),
         2 * n_cat) + f32_concat,
        ('requantize vs copy', 'QuantizedConcat, 4 ranges', concat(different),
         2 * n_cat, 'QuantizedConcat, 1 range', concat(equal), 2 * n_cat),
        ('avg pool 3x3/1', 'QuantizedAvgPool',
         lambda: q.quantized_avg_pool(q3, q3mn, q3mx, **POOL3)[0], 2 * n3,
         'AvgPool bf16', lambda: tf.nn.avg_pool(b3, **POOL3), 4 * n3),
        ('avg pool 8x8 head', 'QuantizedAvgPool',
         lambda: q.quantized_avg_pool(q8, q8mn, q8mx, **POOL8)[0],
         n8 + n8_out,
         'AvgPool bf16', lambda: tf.nn.avg_pool(b8, **POOL8),
         2 * (n8 + n8_out)),
        ('relu6', 'QuantizedRelu6',
         lambda: q.quantized_relu6(qr, qrmn, qrmx)[0], 2 * nr,
         'QuantizedRelu', lambda: q.quantized_relu(qr, qrmn, qrmx)[0],
         2 * nr),
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
        print('# %s: %s, then %s' % (case, name, yname), file=sys.stderr,
              flush=True)
        t, y = timed(make), timed(ymake)
        print('| %s | %s | %s | %s | %s | %.2f (%.2f-%.2f) |'
              % (case, name, cell(t, nbytes), yname, cell(y, ybytes),
                 t[0] / y[0], t[1] / y[2], t[2] / y[1]), flush=True)


if __name__ == '__main__':
    main()
