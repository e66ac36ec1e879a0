"""Times the int8 GPU kernels against the bf16 ones at the same shapes:
QuantizedMatMul vs bf16 MatMul at 4096^3 and at the ResNet-50 stage shape
(256*14*14, 256, 2304), and QuantizedConv2D vs bf16 Conv2D at (32,56,56,64)
with a 3x3x64x64 filter. Prints a markdown table.

Method: one graph holds `reps` copies of the op chained by control
dependencies, run as a single step that ends in a device synchronise. The
step is timed at two values of `reps`; the per-op time is the difference of
the two medians over the difference in copies, which cancels the per-step host
cost and the ops that prepare the operands. The operands are variables
filled on the device (quantized, or cast to bf16, once per step), so no step
copies anything from the host. Every step shape is warmed up first.

The quantized time includes the operand packers, which run on every call.
Their share comes from a kernel trace taken in a run of its own, e.g.
  rocprofv3 --kernel-trace --stats -d <dir> -- \
      python scripts/quantized_gemm_probe.py --profile
(--profile runs each quantized op a few times and nothing else).

Needs a GPU; run it under a time limit:
  timeout 600 python scripts/quantized_gemm_probe.py
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simple_tensorflow_amd as tf  # noqa: E402
from simple_tensorflow_amd.python.ops import quantized_ops as q  # noqa: E402

GEMM_SHAPES = [(4096, 4096, 4096), (256 * 14 * 14, 256, 2304)]
CONV_SHAPE = ((32, 56, 56, 64), (3, 3, 64, 64))


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


def _per_op_seconds(sess, make, lo, hi, warmup, iters):
    with tf.device('/gpu:0'):
        op_lo = _chained(make, lo)
        op_hi = _chained(make, hi)
    # alternate the two so drift hits both alike
    t_lo, t_hi = [], []
    for _ in range(3):
        t_lo.append(_median_step(sess, op_lo, warmup, iters))
        t_hi.append(_median_step(sess, op_hi, warmup, iters))
    print('#   step medians: %d copies %.3f ms, %d copies %.3f ms'
          % (lo, np.median(t_lo) * 1e3, hi, np.median(t_hi) * 1e3),
          file=sys.stderr, flush=True)
    return (np.median(t_hi) - np.median(t_lo)) / (hi - lo)


def _device_operand(shape):
    """An f32 variable filled on the device, so no step feeds anything."""
    return tf.Variable(tf.random_uniform(shape, -1.0, 1.0))


def _u8(v):
    return q.quantize_v2(v, -1.0, 1.0)[0]


def _gemm_ops(m, n, k):
    with tf.device('/gpu:0'):
        a, b = _device_operand((m, k)), _device_operand((k, n))
        a8, b8 = _u8(a), _u8(b)
        a16, b16 = tf.cast(a, tf.bfloat16), tf.cast(b, tf.bfloat16)
    make8 = lambda: q.quantized_matmul(a8, b8, -1.0, 1.0, -1.0, 1.0)[0]
    make16 = lambda: tf.matmul(a16, b16)
    return make8, make16


def _conv_ops(xs, ws):
    with tf.device('/gpu:0'):
        x, w = _device_operand(xs), _device_operand(ws)
        x8, w8 = _u8(x), _u8(w)
        x16, w16 = tf.cast(x, tf.bfloat16), tf.cast(w, tf.bfloat16)
    make8 = lambda: q.quantized_conv2d(x8, w8, -1.0, 1.0, -1.0, 1.0,
                                       [1, 1, 1, 1], 'SAME')[0]
    make16 = lambda: tf.nn.conv2d(x16, w16, [1, 1, 1, 1], 'SAME')
    return make8, make16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lo', type=int, default=4)
    ap.add_argument('--hi', type=int, default=44)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--profile', action='store_true',
                    help='run each quantized op a few times and exit')
    args = ap.parse_args()

    sess = tf.Session()
    assert sess.num_gpus() > 0, 'the probe needs a GPU'

    cases = []
    for m, n, k in GEMM_SHAPES:
        cases.append(('matmul %dx%dx%d' % (m, n, k), 2.0 * m * n * k,
                      _gemm_ops(m, n, k)))
    xs, ws = CONV_SHAPE
    flops = 2.0 * xs[0] * xs[1] * xs[2] * ws[0] * ws[1] * ws[2] * ws[3]
    cases.append(('conv %s * %s' % (xs, ws), flops, _conv_ops(xs, ws)))

    sess.run(tf.global_variables_initializer())
    if args.profile:
        for _, _, (make8, _) in cases:
            with tf.device('/gpu:0'):
                op = _chained(make8, 4)
            for _ in range(3):
                sess.run(op)
            sess.sync()
        return

    print('| case | int8 ms | int8 Top/s | bf16 ms | bf16 Tflop/s | '
          'int8 / bf16 time |')
    print('|---|---|---|---|---|---|')
    for name, flops, (make8, make16) in cases:
        t8 = _per_op_seconds(sess, make8, args.lo, args.hi, args.warmup,
                             args.iters)
        t16 = _per_op_seconds(sess, make16, args.lo, args.hi, args.warmup,
                              args.iters)
        print('| %s | %.3f | %.1f | %.3f | %.1f | %.2f |'
              % (name, t8 * 1e3, flops / t8 / 1e12, t16 * 1e3,
                 flops / t16 / 1e12, t8 / t16), flush=True)


if __name__ == '__main__':
    main()
