"""bench.py command line: --steps, ms_per_step, --full and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import simple_tensorflow_amd as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _tiny_train_graph():
    tf.reset_default_graph()
    w = tf.Variable(tf.truncated_normal([4, 3], stddev=0.1, seed=3), name='w')
    b = tf.Variable(tf.zeros([3]), name='b')
    x = tf.constant(np.arange(8, dtype=np.float32).reshape(2, 4))
    loss = tf.reduce_mean(tf.square(tf.matmul(x, w.value()) + b.value()))
    train_op = tf.train.MomentumOptimizer(0.01, 0.9).minimize(loss)
    return w, b, loss, train_op


def test_rewind_restores_weights_and_slots():
    w, b, loss, train_op = _tiny_train_graph()
    rewind = bench._Rewind()
    gvars = tf.global_variables()
    assert len(gvars) == 4  # w, b and their momentum slots
    with tf.Session() as sess:
        sess.run(tf.global_variables_initializer())
        rewind.save(sess)
        start = sess.run([v.value() for v in gvars])
        bench._run_steps(sess, train_op, loss, None, 1)
        once = sess.run([v.value() for v in gvars])
        bench._run_steps(sess, train_op, loss, None, 2)
        rewind.restore(sess)
        back = sess.run([v.value() for v in gvars])
        for s, r in zip(start, back):
            np.testing.assert_array_equal(s, r)
        # the step after a rewind repeats the first step exactly (CPU)
        bench._run_steps(sess, train_op, loss, None, 1)
        again = sess.run([v.value() for v in gvars])
        for o, a in zip(once, again):
            np.testing.assert_array_equal(o, a)
        assert any(np.abs(o - s).max() > 0 for o, s in zip(once, start))


def test_dump_outputs_files(tmp_path, monkeypatch):
    w, b, loss, train_op = _tiny_train_graph()
    monkeypatch.setattr(bench, '_DUMP_MAX_ELEMS', 8)  # w (12) gets sampled
    out = tmp_path / 'dump'
    with tf.Session() as sess:
        sess.run(tf.global_variables_initializer())
        bench._run_steps(sess, train_op, loss, None, 1)
        bench._dump_outputs(sess, loss, str(out))
        bench._dump_outputs(sess, loss, str(tmp_path / 'dump2'))
        wv, bv, lv = sess.run([w.value(), b.value(), loss])
    assert sorted(os.listdir(str(out))) == ['loss.npy', 'variables.npy']
    got = np.load(str(out / 'variables.npy'))
    assert got.dtype == np.float32 and got.shape == (8 + 3,)
    assert set(got[:8]) <= set(wv.reshape(-1))
    np.testing.assert_array_equal(got[8:], bv)
    got_loss = np.load(str(out / 'loss.npy'))
    assert got_loss.dtype == np.float32 and float(got_loss) == float(lv)
    # the sample is fixed: a second dump of the same state is identical
    np.testing.assert_array_equal(
        got, np.load(str(tmp_path / 'dump2' / 'variables.npy')))


@pytest.mark.gpu
def test_bench_cli_steps_full_and_dump(tmp_path):
    out = tmp_path / 'outputs'
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1',
         '--steps', '3', '--warmup', '1', '--batch', '8', '--full',
         '--dump-outputs', str(out)],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res['steps'] == 3 and res['warmup'] == 1
    assert res['metric'] == res['unit'] == 'images/sec'
    assert res['higher_is_better'] is True and res['dtype'] == 'bf16'
    assert res['ms_per_step'] > 0
    # value and ms_per_step describe the same timed steps
    assert res['value'] == pytest.approx(8 * 1000.0 / res['ms_per_step'],
                                         rel=1e-3)
    files = sorted(os.listdir(str(out)))
    assert files == ['loss.npy', 'variables.npy']
    total = 0
    for f in files:
        a = np.load(str(out / f))
        assert a.dtype == np.float32 and np.isfinite(a).all()
        total += os.path.getsize(str(out / f))
    assert total <= 64 << 20
    assert float(np.load(str(out / 'loss.npy'))) > 0.0  # a cross-entropy
