"""Times float32 Conv2D forward, dx and dW at the two conv layers of the
TF-1.0 CIFAR-10 and MNIST tutorial nets, batch 128, three ways:

  f32      the op as placed by default (the f32-MFMA kernel of conv_f32.hip),
           operands in GPU variables
  cpu      the same op under tf.device('/cpu:0'), which is where the placer
           sent every f32 conv before that kernel existed, with its operands
           fed from host memory. That is the CPU path at its best: a CPU
           kernel whose input comes from a GPU op is handed the device
           pointer (Device::CopyDeviceTensorToHost of the CPU device is an
           alias) and its direct loops then read every element over the bus,
           which takes minutes at these shapes and is not timed here.
  bf16     the bf16 op of the same shape on the GPU, operands in GPU
           variables (cast once, at initialisation)

The fetch is the op itself, not its value, so nothing is copied back. Each
figure is the host clock around `--steps` runs that end in a device
synchronise, after `--warmup` runs; the best and the median of `--repeats`
windows are printed, one JSON line per layer and op. Needs a GPU. One layer
per process keeps every run under a limit of its own:

  for l in cifar10_conv1 cifar10_conv2 mnist_conv1 mnist_conv2; do
    timeout 120 python scripts/conv_f32_probe.py --layer $l || break
  done"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simple_tensorflow_amd as tf  # noqa: E402

# name: (h, w, c), (r, s, cout); stride 1, SAME
LAYERS = {'cifar10_conv1': ((24, 24, 3), (5, 5, 64)),
          'cifar10_conv2': ((12, 12, 64), (5, 5, 64)),
          'mnist_conv1': ((28, 28, 1), (5, 5, 32)),
          'mnist_conv2': ((14, 14, 32), (5, 5, 64))}
STRIDES = [1, 1, 1, 1]


def build(kind, batch, hwc, rsk, feeds):
    """{'fwd' | 'dx' | 'dw': op} of one layer for one way of running it;
    the host operands of kind 'cpu' go into `feeds`."""
    (h, w, c), (r, s, k) = hwc, rsk
    rng = np.random.RandomState(0)
    dtype = tf.bfloat16 if kind == 'bf16' else tf.float32

    def operand(*shape):
        value = rng.randn(*shape).astype(np.float32)
        if kind == 'cpu':
            p = tf.placeholder(tf.float32, list(shape))
            feeds[p] = value
            return p
        return tf.Variable(tf.cast(tf.constant(value), dtype)).ref()

    with tf.device('/cpu:0' if kind == 'cpu' else None):
        x, f, dy = (operand(batch, h, w, c), operand(r, s, c, k),
                    operand(batch, h, w, k))
        return {
            'fwd': tf.nn.conv2d(x, f, STRIDES, 'SAME'),
            'dx': tf.nn.conv2d_backprop_input([batch, h, w, c], f, dy,
                                              STRIDES, 'SAME'),
            'dw': tf.nn.conv2d_backprop_filter(x, [r, s, c, k], dy, STRIDES,
                                               'SAME')}


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
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--cpu-steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    kinds = args.kinds.split(',')
    hwc, rsk = LAYERS[args.layer]
    feeds = {}
    ops = {kind: build(kind, args.batch, hwc, rsk, feeds) for kind in kinds}
    with tf.Session() as sess:
        assert sess.num_gpus() > 0, 'conv_f32_probe needs a GPU'
        sess.run(tf.global_variables_initializer())
        for which in ('fwd', 'dx', 'dw'):
            row = {'layer': args.layer, 'op': which, 'batch': args.batch}
            for kind in kinds:
                cpu = kind == 'cpu'
                best, med = measure(
                    sess, ops[kind][which], feeds if cpu else {},
                    args.cpu_steps if cpu else args.steps,
                    1 if cpu else args.warmup, 2 if cpu else args.repeats)
                row[kind + '_us'] = round(best, 1)
                row[kind + '_median_us'] = round(med, 1)
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
