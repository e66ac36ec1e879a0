"""Multi-tensor ApplyMomentum: the FuseApplyMomentum pass and its kernel.

Every comparison is the fused graph against the same graph built with
STF_NO_MULTI_APPLY set, in which each variable is updated by its own
ApplyMomentum node and the per-variable kernel. Both kernels run the one
per-element update function and no other value in these graphs comes from a
kernel that sums in a varying order, so var and accum must agree bit for bit:
they are compared as uint32 after one step and after three.

Gradients are f32 (the variable is used in an f32 loss) or bf16 (the variable
is cast to bf16 and used in bf16 arithmetic or a bf16 matmul, so its gradient
reaches the update through a bf16 -> f32 Cast, which the pass looks through).
Every loss term is quadratic in its variable, so later steps see gradients
that depend on the earlier updates."""
import os
import re

import numpy as np
import pytest

import simple_tensorflow_amd as tf
from simple_tensorflow_amd.python.ops import variables

pytestmark = pytest.mark.gpu


def _pack_constant(name):
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.path.join(here, '..', 'simple_tensorflow_amd', 'csrc', 'kernels',
                        'hip', 'multi_apply_pack.h')
    with open(path) as f:
        m = re.search(r'constexpr \w+ %s = (\d+);' % name, f.read())
    return int(m.group(1))


CHUNK = _pack_constant('kMultiApplyChunk')
CAPACITY = _pack_constant('kMultiApplyMaxTensors')

# 1 .. 1024: below, at and above the vector width; 3*3*8*16: a filter shape;
# 2 * CHUNK + 13: three chunks, the last one ragged with an odd tail.
SHAPES = [(1,), (7,), (8,), (255,), (1024,), (3, 3, 8, 16), (2 * CHUNK + 13,)]


@pytest.fixture(autouse=True)
def fresh_graph():
    tf.reset_default_graph()
    yield


def _sess():
    s = tf.Session()
    assert s.num_gpus() > 0
    return s


def _with_env(name, fn):
    """fn() in a fresh graph with the switch `name` set."""
    os.environ[name] = '1'
    try:
        tf.reset_default_graph()
        return fn()
    finally:
        del os.environ[name]


class _Model(object):
    """Variables and loss terms, with seeded values."""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.vars = []
        self.terms = []

    def _var(self, shape):
        v = variables.Variable(
            tf.constant(self.rng.randn(*shape).astype(np.float32)),
            name='v%d' % len(self.vars))
        self.vars.append(v)
        return v

    def _coeff(self, shape):
        return (self.rng.rand(*shape) + 0.5).astype(np.float32)

    def f32(self, shape, coeff=None):
        """sum(c v^2) in f32, or sum(c v) for a given c: grad is f32"""
        v = self._var(shape)
        if coeff is None:
            term = v.value() * v.value() * tf.constant(self._coeff(shape))
        else:
            term = v.value() * tf.constant(coeff)
        self.terms.append(tf.reduce_sum(term))
        return v

    def bf16(self, shape, coeff=None):
        """the same in bf16 arithmetic on cast(v): grad is bf16"""
        v = self._var(shape)
        v16 = tf.cast(v.ref(), tf.bfloat16)
        if coeff is None:
            term = v16 * v16 * tf.constant(self._coeff(shape),
                                           dtype=tf.bfloat16)
        else:
            term = v16 * tf.constant(coeff, dtype=tf.bfloat16)
        self.terms.append(tf.reduce_sum(tf.cast(term, tf.float32)))
        return v

    def matmul_bf16(self, k, n):
        """sum(c (x w16)^2) with a bf16 matmul: grad is the bf16 dW"""
        v = self._var((k, n))
        x = tf.constant(self.rng.randn(8, k).astype(np.float32),
                        dtype=tf.bfloat16)
        y = tf.cast(tf.matmul(x, tf.cast(v.ref(), tf.bfloat16)), tf.float32)
        self.terms.append(tf.reduce_sum(y * y * tf.constant(
            self._coeff((8, n)))))
        return v

    def loss(self):
        return tf.add_n(self.terms)


def _grad_casts():
    """names of the bf16 -> f32 Cast nodes that feed an ApplyMomentum and
    nothing else"""
    names = []
    for op in tf.get_default_graph().get_operations():
        if op.type != 'ApplyMomentum':
            continue
        g = op.inputs[3]
        if (g.op.type == 'Cast' and g.op.inputs[0].dtype == tf.bfloat16 and
                g.consumers() == [op]):
            names.append(g.op.name)
    return names


def _u32(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def _train(build, steps=3, with_init=False):
    """build() -> (fetches to run each step, optimizers, variables). Returns
    the uint32 views of every var and slot after step 1 and after the last
    step (with_init: also, first, after initialization), the (node name, op)
    pairs the first step ran, and the Cast names of _grad_casts. The state
    list goes variable by variable: var, then its slot of each optimizer that
    has one."""
    fetches, opts, vs = build()
    state = []
    for v in vs:
        state.append(v.value())
        for opt in opts:
            slot = opt.get_slot(v, 'momentum')
            if slot is not None:
                state.append(slot.value())
    casts = _grad_casts()
    run_opts = tf.RunOptions(trace_level=tf.RunOptions.FULL_TRACE)
    md = tf.RunMetadata()
    snaps = []
    with _sess() as s:
        s.run(tf.global_variables_initializer())
        if with_init:
            snaps.append([_u32(a) for a in s.run(state)])
        for step in range(steps):
            if step == 0:
                s.run(fetches, options=run_opts, run_metadata=md)
            else:
                s.run(fetches)
            if step in (0, steps - 1):
                snaps.append([_u32(a) for a in s.run(state)])
    # a set: a GPU node is listed under its device and under its stream
    ran = sorted({(ns.node_name, ns.op) for ds in md.step_stats.dev_stats
                  for ns in ds.node_stats})
    return snaps, ran, casts


def _count(ran, op):
    return sum(1 for _, o in ran if o == op)


def _assert_bit_equal(on, off):
    assert len(on) == len(off) >= 2
    for step, (a, b) in enumerate(zip(on, off)):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), (
                'snapshot %d, state tensor %d of %d elements: %d differ'
                % (step, i, x.size, int((x != y).sum())))
    # the variables moved, so the comparison is of updates and not of inits
    assert any(not np.array_equal(x, y) for x, y in zip(on[-2], on[-1]))


def _both(build):
    on, on_ran, casts = _train(build)
    off, off_ran, off_casts = _with_env('STF_NO_MULTI_APPLY',
                                        lambda: _train(build))
    assert casts == off_casts
    _assert_bit_equal(on, off)
    return on_ran, off_ran, casts


# ---------------------------------------------------------------------------
@pytest.mark.parametrize('nesterov', [False, True], ids=['plain', 'nesterov'])
def test_sizes_and_gradient_types(nesterov):
    def build():
        m = _Model(seed=1)
        for shape in SHAPES:
            m.f32(shape)
        for shape in SHAPES:
            m.bf16(shape)
        m.matmul_bf16(16, 64)
        opt = tf.train.MomentumOptimizer(0.1, 0.9, use_nesterov=nesterov)
        return opt.minimize(m.loss()), [opt], m.vars

    on_ran, off_ran, casts = _both(build)
    n = 2 * len(SHAPES) + 1
    assert len(casts) == len(SHAPES) + 1
    # one fused node per gradient type, nothing left of the members
    assert _count(on_ran, '_MultiApplyMomentum') == 2
    assert _count(on_ran, 'ApplyMomentum') == 0
    on_names = {name for name, _ in on_ran}
    assert not on_names & set(casts)
    assert _count(off_ran, 'ApplyMomentum') == n
    assert _count(off_ran, '_MultiApplyMomentum') == 0
    assert set(casts) <= {name for name, _ in off_ran}


def test_more_variables_than_one_table():
    def build():
        m = _Model(seed=2)
        for i in range(CAPACITY + 5):
            m.f32((1 + i % 9,))
        opt = tf.train.MomentumOptimizer(0.1, 0.9)
        return opt.minimize(m.loss()), [opt], m.vars

    on_ran, off_ran, _ = _both(build)
    assert _count(on_ran, '_MultiApplyMomentum') == 1
    assert _count(on_ran, 'ApplyMomentum') == 0
    assert _count(off_ran, 'ApplyMomentum') == CAPACITY + 5


@pytest.mark.parametrize('nesterov', [False, True], ids=['plain', 'nesterov'])
def test_two_learning_rates_two_groups(nesterov):
    def build():
        m = _Model(seed=3)
        a = [m.f32((7,)), m.f32((1024,)), m.bf16((255,)), m.bf16((8,))]
        b = [m.f32((255,)), m.f32((8,)), m.bf16((7,)), m.bf16((1024,))]
        loss = m.loss()
        opt_a = tf.train.MomentumOptimizer(tf.constant(0.1), 0.9,
                                           use_nesterov=nesterov)
        opt_b = tf.train.MomentumOptimizer(tf.constant(0.05), 0.9,
                                           use_nesterov=nesterov,
                                           name='MomentumB')
        train = tf.group(opt_a.minimize(loss, var_list=a),
                         opt_b.minimize(loss, var_list=b))
        return train, [opt_a, opt_b], m.vars

    on_ran, off_ran, casts = _both(build)
    assert len(casts) == 4
    # (two learning rates) x (two gradient types)
    assert _count(on_ran, '_MultiApplyMomentum') == 4
    assert _count(on_ran, 'ApplyMomentum') == 0
    assert _count(off_ran, 'ApplyMomentum') == 8


@pytest.mark.parametrize('optimizers', [1, 2], ids=['one_optimizer',
                                                    'two_equal_lr'])
def test_other_train_op_is_left_alone(optimizers):
    """Two minimize calls over disjoint variables, with equal lr and momentum
    (their constants are merged by CSE), and only the first train op is run:
    the second list's variables and slots keep their initial bits, and its
    loss, which needs a placeholder nobody feeds, is never asked for."""
    n_a = 4

    def build():
        m = _Model(seed=7)
        a = [m.f32((7,)), m.f32((1024,)), m.bf16((255,)), m.bf16((8,))]
        loss_a = m.loss()
        m.terms = []
        b = [m.f32((255,)), m.f32((8,)), m.bf16((7,)), m.bf16((1024,))]
        loss_b = m.loss() * tf.placeholder(tf.float32, [])
        assert len(a) == n_a
        opt_a = tf.train.MomentumOptimizer(0.1, 0.9)
        opt_b = opt_a if optimizers == 1 else tf.train.MomentumOptimizer(
            0.1, 0.9, name='MomentumB')
        train_a = opt_a.minimize(loss_a, var_list=a)
        opt_b.minimize(loss_b, var_list=b)
        return train_a, [opt_a] if optimizers == 1 else [opt_a, opt_b], m.vars

    on, on_ran, casts = _train(build, with_init=True)
    off, off_ran, _ = _with_env('STF_NO_MULTI_APPLY',
                                lambda: _train(build, with_init=True))
    _assert_bit_equal(on, off)
    assert len(casts) == 4
    # only the first train op's updates ran: one fused node per gradient type
    assert _count(on_ran, '_MultiApplyMomentum') == 2
    assert _count(on_ran, 'ApplyMomentum') == 0
    assert _count(off_ran, 'ApplyMomentum') == n_a
    # state: (var, slot) per variable; the second list is as initialized
    assert len(on[0]) == 4 * n_a
    for snap in on[1:]:
        for i in range(2 * n_a, 4 * n_a):
            assert np.array_equal(snap[i], on[0][i])
        assert all(not np.array_equal(snap[i], on[0][i])
                   for i in range(2 * n_a))


def test_fetched_update_stays():
    def build():
        m = _Model(seed=4)
        for shape in [(7,), (255,), (1024,)]:
            m.f32(shape)
        opt = tf.train.MomentumOptimizer(0.1, 0.9)
        train = opt.minimize(m.loss())
        fetched = [op for op in tf.get_default_graph().get_operations()
                   if op.type == 'ApplyMomentum' and
                   op.inputs[0] is m.vars[1].ref()]
        assert len(fetched) == 1
        return [train, fetched[0].outputs[0]], [opt], m.vars

    on_ran, off_ran, _ = _both(build)
    assert _count(on_ran, '_MultiApplyMomentum') == 1
    assert _count(on_ran, 'ApplyMomentum') == 1
    assert _count(off_ran, 'ApplyMomentum') == 3


def test_variable_with_two_updates_stays():
    def build():
        m = _Model(seed=5)
        vs = [m.f32((7,)), m.f32((255,)), m.f32((1024,)), m.f32((8,)),
              m.f32((1,))]
        loss = m.loss()
        opt_a = tf.train.MomentumOptimizer(tf.constant(0.1), 0.9)
        opt_b = tf.train.MomentumOptimizer(tf.constant(0.05), 0.9,
                                           name='MomentumB')
        train_a = opt_a.minimize(loss, var_list=vs[:3])
        # the second update of vs[0] is ordered after the first
        with tf.control_dependencies([train_a]):
            train_b = opt_b.minimize(loss, var_list=[vs[0]] + vs[3:])
        return train_b, [opt_a, opt_b], m.vars

    on_ran, off_ran, _ = _both(build)
    assert _count(on_ran, '_MultiApplyMomentum') == 2
    assert _count(on_ran, 'ApplyMomentum') == 2
    assert _count(off_ran, 'ApplyMomentum') == 6


def test_non_finite_gradients():
    def coeff(n):
        c = np.linspace(-2.0, 2.0, n).astype(np.float32)
        c[1::7] = np.nan
        c[2::7] = np.inf
        c[3::7] = -np.inf
        return c

    def build():
        m = _Model(seed=6)
        m.f32((255,), coeff(255))
        m.f32((1024,))
        m.bf16((255,), coeff(255))
        m.bf16((1024,))
        opt = tf.train.MomentumOptimizer(0.1, 0.9)
        return opt.minimize(m.loss()), [opt], m.vars

    on, on_ran, _ = _train(build)
    off, _, _ = _with_env('STF_NO_MULTI_APPLY', lambda: _train(build))
    assert _count(on_ran, '_MultiApplyMomentum') == 2
    _assert_bit_equal(on, off)
    # NaN and both infinities did reach var and accum
    got = np.concatenate([x.view(np.float32) for x in on[0]])
    assert np.isnan(got).any()
    assert np.isposinf(got).any() and np.isneginf(got).any()
