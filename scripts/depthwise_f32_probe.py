"""Times float32 depthwise conv forward, dx and dW at the depthwise layers of
MobileNet-v1 (3x3, channel multiplier 1, SAME), batch 32, three ways:

  f32      the op as placed by default (the tiled kernels of
           hip/depthwise_f32.hip), operands in GPU variables
  cpu      the forward under tf.device('/cpu:0'), which is where the placer
           sent the f32 op before those kernels existed, operands fed from
           host memory (see scripts/conv_f32_probe.py for why that is the CPU
           path at its best). Forward only: before these kernels the float
           gradients had no kernel on any device, so there is nothing to time.
  bf16     the bf16 op of the same shape on the GPU (hip/depthwise.hip, one
           thread per element, R*S atomics per output in dW), operands in GPU
           variables (cast once, at initialisation)

Each row also carries the byte floor: x read once and y written once for fwd
(dy and dx for dx), x and dy read once for dW, as microseconds at
`--floor-tbs` TB/s, and the f32 time over it.

The fetch is the op itself, not its value, so nothing is copied back. Each
figure is the host clock around `--steps` runs that end in a device
synchronise, after `--warmup` runs; the best and the median of `--repeats`
windows are printed, one JSON line per layer and op. Needs a GPU. One layer
per process keeps every run under a limit of its own:

  for l in dw1 dw2 dw4 dw6 dw8 dw13; do
    timeout 240 python scripts/depthwise_f32_probe.py --layer $l || break
  done"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simple_tensorflow_amd as tf  # noqa: E402
from simple_tensorflow_amd.python.framework.ops import apply_op  # noqa: E402

# name: (h, w, c), stride; 3x3, mult 1, SAME
LAYERS = {'dw1': ((112, 112, 32), 1), 'dw2': ((112, 112, 64), 2),
          'dw4': ((56, 56, 128), 1), 'dw6': ((28, 28, 256), 1),
          'dw8': ((14, 14, 512), 1), 'dw13': ((7, 7, 1024), 1)}


def build(kind, batch, hwc, stride, feeds):
    """{'fwd' | 'dx' | 'dw': op} of one layer for one way of running it;
    the host operands of kind 'cpu' go into `feeds`."""
    h, w, c = hwc
    p, q = -(-h // stride), -(-w // stride)
    rng = np.random.RandomState(0)
    dtype = tf.bfloat16 if kind == 'bf16' else tf.float32
    attrs = dict(strides=[1, stride, stride, 1], padding='SAME')

    def operand(*shape):
        value = rng.randn(*shape).astype(np.float32)
        if kind == 'cpu':
            ph = tf.placeholder(tf.float32, list(shape))
            feeds[ph] = value
            return ph
        return tf.Variable(tf.cast(tf.constant(value), dtype)).ref()

    with tf.device('/cpu:0' if kind == 'cpu' else None):
        x, f = operand(batch, h, w, c), operand(3, 3, c, 1)
        ops = {'fwd': tf.nn.depthwise_conv2d(x, f, **attrs)}
        if kind == 'cpu':
            return ops
        dy = operand(batch, p, q, c)
        ops['dx'] = apply_op(
            'DepthwiseConv2dNativeBackpropInput',
            tf.constant([batch, h, w, c], dtype=tf.int32), f, dy, **attrs)
        ops['dw'] = apply_op(
            'DepthwiseConv2dNativeBackpropFilter', x,
            tf.constant([3, 3, c, 1], dtype=tf.int32), dy, **attrs)
        return ops


def measure(sess, op, feeds, steps, warmup, repeats):
    for _ in range(warmup):
        sess.run(op.op, feeds)
    sess.sync()
    windows = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            sess.run(op.op, feeds)
        sess.sync()
        windows.append((time.perf_counter() - t0) / steps * 1e6)
    return min(windows), float(np.median(windows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--layer', choices=sorted(LAYERS), required=True)
    ap.add_argument('--kinds', default='f32,cpu,bf16')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--bf16-steps', type=int, default=20)
    ap.add_argument('--cpu-steps', type=int, default=2)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--floor-tbs', type=float, default=5.5)
    args = ap.parse_args()
    kinds = args.kinds.split(',')
    hwc, stride = LAYERS[args.layer]
    h, w, c = hwc
    x_bytes = 4 * args.batch * h * w * c
    y_bytes = 4 * args.batch * -(-h // stride) * -(-w // stride) * c
    feeds = {}
    ops = {kind: build(kind, args.batch, hwc, stride, feeds)
           for kind in kinds}
    steps = {'f32': args.steps, 'bf16': args.bf16_steps,
             'cpu': args.cpu_steps}
    with tf.Session() as sess:
        assert sess.num_gpus() > 0, 'depthwise_f32_probe needs a GPU'
        sess.run(tf.global_variables_initializer())
        for which in ('fwd', 'dx', 'dw'):
            row = {'layer': args.layer, 'op': which, 'batch': args.batch}
            for kind in kinds:
                if which not in ops[kind]:
                    continue
                cpu = kind == 'cpu'
                best, med = measure(
                    sess, ops[kind][which], feeds if cpu else {}, steps[kind],
                    1 if cpu else min(args.warmup, steps[kind]),
                    2 if cpu else args.repeats)
                row[kind + '_us'] = round(best, 1)
                row[kind + '_median_us'] = round(med, 1)
            row['floor_us'] = round(
                (x_bytes + y_bytes) / (args.floor_tbs * 1e12) * 1e6, 1)
            if 'f32_us' in row:
                row['f32_over_floor'] = round(
                    row['f32_us'] / max(row['floor_us'], 0.1), 2)
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
