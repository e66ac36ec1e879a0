#!/usr/bin/env python3
"""Flagship benchmark: ResNet-50 v1 bf16 training, images/sec (whole job),
batch 256/GPU, synthetic 224x224x3 data, random-init weights
(BASELINE.json metric).

Single GPU:   python bench.py --steps 20 --warmup 5
Multi-GPU:    torchrun --nnodes=1 --nproc-per-node N bench.py --gpus N ...
              (one process per GPU over RCCL; rank/env from torchrun)

A plain run sets up, warms up, times --steps training steps and prints one
JSON result line. --dump-outputs DIR additionally writes what the last timed
step computed, starting from the post-initialization state (see _Rewind
and _dump_outputs). --full is where any measurement beyond
the headline figure belongs; the benchmark has none today, so it changes
nothing yet.
"""
import argparse
import json
import os
import sys
import time

# Pin this rank's GPU BEFORE any HIP initialization.
_local_rank = int(os.environ.get('LOCAL_RANK', 0))
_world = int(os.environ.get('WORLD_SIZE', 1))
if _world > 1:
    os.environ.setdefault('HIP_VISIBLE_DEVICES', str(_local_rank))
    # RCCL collectives inside hipGraph capture are not yet validated on
    # multi-GPU nodes (replay of the communicator's internal sequencing);
    # run the distributed step eagerly until round 2 proves it out.
    os.environ.setdefault('STF_NO_HIPGRAPH', '1')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=0)  # 0 = model default
    ap.add_argument('--lr', type=float, default=0.1)
    ap.add_argument('--model', default='resnet50',
                    choices=['resnet50', 'inception3', 'ptb_lstm'])
    ap.add_argument('--seq-len', type=int, default=35)
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='rewind the variables before the last timed step '
                         'and write what it computed as DIR/<name>.npy')
    ap.add_argument('--full', action='store_true',
                    help='also run every secondary measurement (none today)')
    args = ap.parse_args()
    if args.batch == 0:
        args.batch = {'resnet50': 256, 'inception3': 128,
                      'ptb_lstm': 20}[args.model]

    import simple_tensorflow_amd as tf
    from simple_tensorflow_amd.models import resnet

    world = _world
    rank = int(os.environ.get('RANK', 0))

    comm = None
    if world > 1:
        from simple_tensorflow_amd.parallel import dist
        comm = dist.init(world, rank)

    loss_t, train_op = _build(args, world)
    rewind = _Rewind() if args.dump_outputs else None

    sess = tf.Session()
    sess.run(tf.global_variables_initializer())
    if comm is not None:
        comm.broadcast_variables(sess)
    if rewind is not None:
        rewind.save(sess)

    # warmup
    _run_steps(sess, train_op, loss_t, comm, args.warmup)

    if rewind is None:
        elapsed = _run_steps(sess, train_op, loss_t, comm, args.steps)
    else:
        # The clock stops while the state is rewound before the last step.
        elapsed = _run_steps(sess, train_op, loss_t, comm, args.steps - 1)
        rewind.restore(sess)
        elapsed += _run_steps(sess, train_op, loss_t, comm, 1)

    if comm is not None:
        elapsed = comm.max_scalar(elapsed)

    ms_per_step = elapsed / args.steps * 1000.0
    if args.model == 'ptb_lstm':
        value = args.batch * args.seq_len * world * args.steps / elapsed
        metric, unit = 'words/sec', 'words/sec'
        model_name, seq_len, vsb = 'ptb_lstm_h1500', args.seq_len, None
    else:
        value = args.batch * world * args.steps / elapsed
        metric, unit = 'images/sec', 'images/sec'
        seq_len = None
        model_name = 'resnet50_v1' if args.model == 'resnet50' \
            else 'inception_v3'
        vsb = round(value / 219.0, 3) if args.model == 'resnet50' else None
    if rank == 0:
        out = {
            'metric': metric,
            'value': round(value, 2),
            'unit': unit,
            'n_gpus': world,
            'steps': args.steps,
            'warmup': args.warmup,
            'ms_per_step': round(ms_per_step, 3),
            'higher_is_better': True,
            'scaling': 'weak',
            'vs_baseline': vsb,
            'dtype': 'bf16',
            'data': 'synthetic',
            'config': {
                'model': model_name,
                'global_batch': args.batch * world,
                'seq_len': seq_len,
                'parallelism': 'dp%d' % world,
            },
        }
        if args.dump_outputs:
            _dump_outputs(sess, loss_t, args.dump_outputs)
        print(json.dumps(out))


def _run_steps(sess, train_op, loss_t, comm, n):
    """Runs n training steps to completion; returns the seconds they took."""
    t0 = time.time()
    for _ in range(n):
        sess.run(train_op)
    _sync(sess, loss_t)
    if comm is not None:
        comm.barrier()
    return time.time() - t0


class _Rewind(object):
    """Puts every variable (weights and optimizer slots) back to its value
    right after initialization.

    Steps are not bit-reproducible (split-K partial sums are accumulated
    with f32 atomics), and training from random init at the benchmark's
    learning rate amplifies that rounding noise: after a few dozen steps two
    runs of the same build no longer agree in any digit. One step from a
    fixed state stays within rounding noise, so --dump-outputs rewinds
    before the last timed step and two builds can be compared on what that
    step computes."""

    def __init__(self):
        import simple_tensorflow_amd as tf
        self._vars = tf.global_variables()
        self._feeds = [tf.placeholder(v.value().dtype, v.value()._shape)
                       for v in self._vars]
        self._op = tf.group(*[v.assign(p)
                              for v, p in zip(self._vars, self._feeds)])
        self._saved = None

    def save(self, sess):
        self._saved = sess.run([v.value() for v in self._vars])

    def restore(self, sess):
        sess.run(self._op, feed_dict=dict(zip(self._feeds, self._saved)))
        sess.sync()


# Elements written per variable by --dump-outputs; larger ones are sampled.
_DUMP_MAX_ELEMS = 1 << 16
# Upper bound on variables.npy, well inside the 64 MB a dump may take.
_DUMP_BUDGET_BYTES = 48 << 20


def _dump_outputs(sess, loss_t, out_dir):
    """Writes what a caller of the last timed train step is left with, as
    float32 .npy files:

    variables.npy  every trainable variable as that step updated it, in
                   graph order, each flattened; a variable with more than
                   _DUMP_MAX_ELEMS elements contributes a fixed, seeded
                   sample of them (same indices in every run).
    loss.npy       the loss the model gives with those variables.

    The variables are fetched, not recomputed. Graph construction, the
    initializer seeds, the synthetic batches and the state the last step
    starts from (see _Rewind) are fixed, so runs with the same arguments
    start from identical inputs."""
    import numpy as np
    import simple_tensorflow_amd as tf

    os.makedirs(out_dir, exist_ok=True)
    tvars = tf.trainable_variables()
    values = sess.run([v.value() for v in tvars])
    cap = min(_DUMP_MAX_ELEMS, _DUMP_BUDGET_BYTES // (4 * max(len(tvars), 1)))
    rng = np.random.RandomState(20240229)
    parts = []
    for val in values:
        flat = np.asarray(val, dtype=np.float32).reshape(-1)
        if flat.size > cap:
            flat = flat[np.sort(rng.randint(0, flat.size, cap))]
        parts.append(flat)
    np.save(os.path.join(out_dir, 'variables.npy'), np.concatenate(parts))
    loss = np.asarray(sess.run(loss_t), dtype=np.float32)
    np.save(os.path.join(out_dir, 'loss.npy'), loss)


def _build(args, world):
    import simple_tensorflow_amd as tf
    if args.model == 'inception3':
        from simple_tensorflow_amd.models import inception
        loss, train_op = inception.build_train_graph(batch=args.batch,
                                                     lr=args.lr)
        if world > 1:
            raise SystemExit('inception bench is single-GPU in round 1')
        return loss, train_op
    if args.model == 'ptb_lstm':
        from simple_tensorflow_amd.models import ptb_lstm
        loss, train_op = ptb_lstm.build_ptb_graph(
            batch=args.batch, seq_len=args.seq_len, hidden=1500,
            vocab=10000, lr=args.lr)
        if world > 1:
            raise SystemExit('use the resnet50 model for multi-GPU scaling')
        return loss, train_op
    from simple_tensorflow_amd.models import resnet
    images, labels = resnet.synthetic_inputs(args.batch)
    loss = resnet.resnet50_loss(images, labels)
    opt = tf.train.MomentumOptimizer(args.lr, 0.9)
    if world > 1:
        from simple_tensorflow_amd.parallel import dist
        opt = dist.DistributedOptimizer(opt, world)
    train_op = opt.minimize(loss)
    return loss, train_op


def _sync(sess, loss_t):
    sess.sync()


if __name__ == '__main__':
    main()
