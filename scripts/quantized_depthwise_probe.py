"""Times the quantized depthwise conv at the 13 depthwise layers of
MobileNet-v1 (3x3, channel multiplier 1, SAME), batch 32, four ways:

  fused   QuantizedDepthwiseConv2DWithBiasAndRequantize (Relu6), quint8 in,
          quint8 out (hip/depthwise_q8.hip)
  i32     QuantizedDepthwiseConv2D, quint8 in, qint32 out
  f32     the f32 DepthwiseConv2dNative of the same shape (hip/depthwise_f32.hip)
  chain   what quantize_nodes made of one depthwise layer before the
          quantized op existed, timed as one: Dequantize, f32 depthwise,
          BiasAdd, Relu6, Reshape / Min / Max / QuantizeV2

Prints a markdown table: microseconds per op (median and the range over the
rounds), and each time over the op's byte floor, x read once and y written
once at `--floor-tbs` TB/s. Layers dw7 to dw11 have one shape and are timed
once. The method is that of quantized_inference_probe.py: `reps` copies of
the op chained by control dependencies run as one step that ends in a device
synchronise; the per-op time is the difference of the step medians at two
chain lengths over the difference in copies, in three alternating rounds.

Needs a GPU; it is one GPU process. Run it under a time limit:
  timeout 900 python scripts/quantized_depthwise_probe.py
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import simple_tensorflow_amd as tf  # noqa: E402
from simple_tensorflow_amd.python.framework.ops import apply_op  # noqa: E402
from simple_tensorflow_amd.python.ops import quantized_ops as q  # noqa: E402
from quantized_inference_probe import _per_op_seconds  # noqa: E402

BATCH = 32
# name: (h = w, c, stride)
LAYERS = [('dw1', 112, 32, 1), ('dw2', 112, 64, 2), ('dw3', 56, 128, 1),
          ('dw4', 56, 128, 2), ('dw5', 28, 256, 1), ('dw6', 28, 256, 2),
          ('dw7-11', 14, 512, 1), ('dw12', 14, 512, 2), ('dw13', 7, 1024, 1)]
X_RANGE, W_RANGE, OUT_RANGE = (0.0, 6.0), (-1.0, 1.0), (0.0, 6.0)


def _layer(hw, c, stride):
    """{kind: (make, bytes of one x read and one y write)}."""
    attrs = dict(strides=[1, stride, stride, 1], padding='SAME')
    n_in = BATCH * hw * hw * c
    n_out = BATCH * (-(-hw // stride)) ** 2 * c
    with tf.device('/gpu:0'):
        x = tf.Variable(tf.random_uniform((BATCH, hw, hw, c), *X_RANGE))
        w = tf.Variable(tf.random_uniform((3, 3, c, 1), *W_RANGE))
        bias = tf.Variable(tf.random_uniform((c,), -1.0, 1.0))
        x8, xmn, xmx = q.quantize_v2(x, *X_RANGE)
        w8, wmn, wmx = q.quantize_v2(w, *W_RANGE)

    def fused():
        return q.quantized_depthwise_conv2d_with_bias_and_requantize(
            x8, w8, bias, xmn, xmx, wmn, wmx, *OUT_RANGE, activation='Relu6',
            **attrs)[0]

    def i32():
        return q.quantized_depthwise_conv2d(x8, w8, xmn, xmx, wmn, wmx,
                                            **attrs)[0]

    def f32():
        return tf.nn.depthwise_conv2d(x, w, **attrs)

    def chain():
        h = q.dequantize(x8, xmn, xmx)
        h = tf.nn.relu6(tf.nn.bias_add(tf.nn.depthwise_conv2d(h, w, **attrs),
                                       bias))
        flat = tf.reshape(h, [-1])
        return apply_op('QuantizeV2', h, tf.reduce_min(flat, 0),
                        tf.reduce_max(flat, 0), mode='MIN_COMBINED')[0]

    return [('fused', fused, n_in + n_out), ('i32', i32, n_in + 4 * n_out),
            ('f32', f32, 4 * (n_in + n_out)), ('chain', chain, n_in + n_out)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lo', type=int, default=4)
    ap.add_argument('--hi', type=int, default=24)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--floor-tbs', type=float, default=5.5)
    ap.add_argument('--layers', default='')
    args = ap.parse_args()
    want = set(args.layers.split(',')) if args.layers else None

    sess = tf.Session()
    assert sess.num_gpus() > 0, 'the probe needs a GPU'
    print('| layer | h x c / stride | op | us (rounds) | byte floor us | '
          'time / floor | time / f32 |')
    print('|---|---|---|---|---|---|---|')
    for name, hw, c, stride in LAYERS:
        if want and name not in want:
            continue
        kinds = _layer(hw, c, stride)
        sess.run(tf.global_variables_initializer())
        times = {}
        for kind, make, nbytes in kinds:
            print('# %s %s' % (name, kind), file=sys.stderr, flush=True)
            times[kind] = _per_op_seconds(sess, make, args.lo, args.hi,
                                          args.warmup, args.iters)
        for kind, _, nbytes in kinds:
            t = times[kind]
            floor = nbytes / (args.floor_tbs * 1e12)
            print('| %s | %d x %d / %d | %s | %.1f (%.1f-%.1f) | %.1f | %.2f '
                  '| %.2f |' % (name, hw, c, stride, kind, t[0] * 1e6,
                                t[1] * 1e6, t[2] * 1e6, floor * 1e6,
                                t[0] / floor, t[0] / times['f32'][0]),
                  flush=True)


if __name__ == '__main__':
    main()
