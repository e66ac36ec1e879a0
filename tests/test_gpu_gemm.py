"""Bit-exact pinning tests for the GEMM kernels behind MatMul and BatchMatMul
(csrc/kernels/hip/gemm_bf16.hip, gemm_bf16_8ph.hip and gemm_f32.hip, dispatched
from csrc/kernels/gpu_matmul.cc and GemmBf16AutoEx in gpu_common.cc).

Why the results can be compared bit for bit. A product of two bf16 values is
exact in f32. When every input is a multiple of 2^-q and every partial sum
stays below 2^(24-q), f32 accumulation is exact in any order: the MFMA adder
tree, single or double buffering, the split-K atomics and the split-K arena
all give the same f32 sum. The kernel then rounds once to bf16 (round to
nearest even), so the expected output is _bf16(exact), `exact` computed in
float64 (itself exact here: every sum is far below 2^53).

Two input families, each with a seed fixed per case:
  int    one operand holds integers in [-2, 2], the other {-1, 0, 1} with a
         non-zero share of min(2/3, 1000/K). The test asserts on the
         reference that max|exact| <= 256 (a condition on the inputs, not on
         the kernel); every output is then an integer bf16 holds exactly, and
         an error of 1 in any sum shows.
  mant   one operand is n/16, n an integer in [-255, 255] (8 significant
         bits, exact in bf16), the other the sparse {-1, 0, 1} set; run once
         with A rich ('mantA') and once with B rich ('mantB'). |sum| <=
         1000 * 16 and a multiple of 1/16, so below 2^20 and exact in f32. The
         outputs are rounded, ties included: every mantissa bit of the loads
         and the one rounding of each epilogue is checked.

The f32 kernel is exact on integer inputs in [-64, 64] (|sum| <= 64*64*K <
2^24 for K <= 4096); its one randn case carries the standard dot-product
bound gamma_K * (|A| @ |B|), gamma_K = K*u / (1 - K*u), u = 2^-24, on every
element.

Every input goes through a placeholder (bf16 is fed as f32 and cast on the
device), the op under test is fetched directly, and the tests of a module
share one session (renewed every 64 tests, see `sess`). The three families of a case are fetched in one step, so they
are independent ops that the executor enqueues from different threads. The
case table's reach is checked on the CPU by
test_case_table_reaches_every_variant against Python mirrors of the dispatch
predicates, so a retune of the dispatch cannot silently stop a case from
reaching its variant.

BatchMatMul at m=50, n=36, k=45: the K-major row strides (50, 36) and the NT
row stride (45) are no multiples of 8, and the per-batch offsets m*k = 2250
and k*n = 1620 elements are no multiples of 8 either (the bases are 4- and
8-byte aligned, the rows inside them 2-byte). Every block is an
edge block at this size, so the loads are StageSafe's / StageKMajorSafe's
16-byte `*(const ulong2*)` global loads at 2-byte-aligned addresses, plus the
per-element branch of StageKMajorSafe. That is the same unaligned 16-byte
global access the long-standing (100, 60, 147) NT case performs (row stride
147 elements = 294 bytes, through both StageFast and StageSafe); global
memory on gfx950 has no alignment requirement beyond the element, only LDS
does, and every LDS address here is slot-aligned regardless of the source.
So BatchMatMul keeps handing K-major operands to the GEMM as they are.
m=99, n=75, k=77 (all odd, so every batch base is 2-byte aligned too) adds
interior blocks with a full K tile: the unguarded StageKMajor and StageFast
then load from such rows as well."""
import itertools
import zlib

import numpy as np
import pytest

import simple_tensorflow_amd as tf

from test_gpu_kernels import _bf16, _sess

FAMILIES = ('int', 'mantA', 'mantB')
FLAGS = list(itertools.product((False, True), repeat=2))   # (ta, tb)


# ---------------------------------------------------------------------------
# Python mirrors of the dispatch, each beside the name of its C++ source
# ---------------------------------------------------------------------------
def _8ph_ok(M, N, K):
    # stf_gemm_bf16_8ph_ok, csrc/kernels/hip/gemm_bf16_8ph.hip
    return M % 256 == 0 and N % 64 == 0 and K % 64 == 0 and K > 0


def _8ph_nr(N):
    # Launch8Ph, csrc/kernels/hip/gemm_bf16_8ph.hip
    return 4 if N % 256 == 0 else 2 if N % 128 == 0 else 1


def _pick_splitk(M, N, K):
    # PickSplitK, csrc/kernels/gpu_common.cc (STF_SPLITK_TARGET unset)
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if tiles >= 256 or K < 1024:
        return 1
    want = 512 // (tiles or 1)
    kt = K // 64
    if tiles <= 6 and kt // (tiles * want) > 96:
        want = 2048 // tiles
        want = min(want, kt // 48)
        if tiles * want > 4096:
            want = 4096 // tiles
    maxk = max(K // 512, 1)
    return max(min(want, maxk), 1)


def _pick_tile(M, N, skinny=True):
    # PickTile<SKINNY>, csrc/kernels/hip/gemm_bf16.hip; returns (BM, BN)
    if skinny and M <= 32 and N >= 128:
        return (32, 128)
    if N >= 128 and M >= 128:
        return (128, 128)
    if N >= 128:
        return (64, 128)
    if M >= 128:
        return (128, 64)
    return (64, 64)


def _matmul_layout(m, n, ta, tb):
    # GpuMatMulOp::Compute, csrc/kernels/gpu_matmul.cc: a transposed side is
    # staged K-major unless its row stride (m or n) is not a multiple of 8,
    # in which case it is transposed to NT form first
    a_km = ta and m % 8 == 0
    b_km = (not tb) and n % 8 == 0
    return (int(a_km), int(b_km))


def _route(m, n, k, ta, tb):
    """What GemmBf16AutoEx + stf_gemm_bf16 launch for a bf16 MatMul."""
    layout = _matmul_layout(m, n, ta, tb)
    sk = _pick_splitk(m, n, k)
    r = dict(layout=layout, tile=_pick_tile(m, n), sk=sk, nr=None,
             empty_slice=False)
    if sk > 1:
        # GemmBf16NT<SPLITK>: per = ceil(kt / sk); slice s starts at s * per
        kt = (k + 63) // 64
        per = (kt + sk - 1) // sk
        r['mode'] = 'splitk'
        r['empty_slice'] = (sk - 1) * per >= kt
    elif layout == (0, 0) and _8ph_ok(m, n, k):
        r['mode'] = '8ph'
        r['tile'] = (256, 64 * _8ph_nr(n))
        r['nr'] = _8ph_nr(n)
    else:
        # stf_gemm_bf16: short_k = K <= 4 * 64 (STF_GEMM_NO_SB unset)
        r['mode'] = 'single' if k <= 256 else 'double'
    return r


# ---------------------------------------------------------------------------
# case tables: (m, n, k, ta, tb)
# ---------------------------------------------------------------------------
# One interior block plus an edge block along every tile dimension that can
# have one (the skinny tile holds all of M in one block), and a K tail.
TILE_SHAPES = {
    (32, 128): (24, 136),
    (128, 128): (136, 136),
    (64, 128): (72, 136),
    (128, 64): (136, 72),
    (64, 64): (72, 72),
}
MODE_K = {'single': 200, 'double': 328, 'splitk': 1096}
LAYOUTS = list(itertools.product((0, 1), repeat=2))
TILES = list(TILE_SHAPES)
MODES = list(MODE_K)

NT_CASES = [(m, n, k, ta, tb)
            for (m, n) in TILE_SHAPES.values()
            for k in MODE_K.values()
            for ta, tb in FLAGS]
# 81 K-tiles over 10 slices of 9: slice 9 is empty and must leave C alone
NT_CASES += [(136, 136, 5184, False, True), (136, 136, 5184, True, False)]
# NT only: scalar K tail of StageSafe (kbase < K < kbase + 8), and row bases
# that are not 16-byte aligned in StageFast
NT_CASES += [(m, n, k, False, True)
             for (m, n) in ((136, 136), (24, 136), (72, 72))
             for k in (147, 333)]
# M or N not a multiple of 8: GpuMatMulOp's pre-transpose fallback
NT_CASES += [(m, n, k, ta, tb)
             for (m, n, k) in ((100, 60, 200), (130, 60, 328),
                               (60, 130, 1096))
             for ta, tb in FLAGS]

# 8-phase kernel: the A and the B ring each hold 2 K-tiles (a_slot/b_slot
# take slot u & 1; the prologue stages B(0) and B(1)), so K/64 = 1, 2, 3 and
# 15 run the loop below, at, one past and far past the ring depth.
PH8_N = (64, 192, 128, 384, 256, 512)      # NR 1, 1, 2, 2, 4, 4
PH8_K = (64, 128, 192, 960)
PH8_CASES = [(256, n, k, False, True) for n in PH8_N for k in PH8_K]
PH8_CASES += [(512, n, 192, False, True) for n in PH8_N]

# BatchMatMul bf16 goes to stf_gemm_bf16 directly (no split-K), batch of 3
# (99, 75, 77) adds interior blocks with a full first K tile, so StageKMajor
# and StageFast themselves (not only their guarded forms) load 16 bytes from
# rows whose strides (99, 75, 77) and batch offsets (odd) are 2-byte aligned
BMM_SHAPES = ((72, 136, 328), (50, 36, 45), (99, 75, 77))

F32_SHAPES = ((200, 300, 150), (64, 64, 16), (65, 63, 17), (1, 1, 1))


def _cid(case):
    m, n, k, ta, tb = case
    return '%dx%dx%d-%s%s' % (m, n, k, 'T' if ta else 'N', 'T' if tb else 'N')


# ---------------------------------------------------------------------------
# inputs and references
# ---------------------------------------------------------------------------
def _sparse(rng, shape, kc):
    """{-1, 0, 1} with a non-zero share of min(2/3, 1000/kc)."""
    share = min(2.0 / 3.0, 1000.0 / kc)
    keep = rng.random_sample(shape) < share
    return (rng.choice([-1.0, 1.0], shape) * keep).astype(np.float32)


def _rich(rng, shape, family):
    if family == 'int':
        return rng.randint(-2, 3, shape).astype(np.float32)
    return (rng.randint(-255, 256, shape) / 16.0).astype(np.float32)


def _operands(label, family, a_shape, b_shape, kc):
    """A and B of one family; the seed is a function of the label alone."""
    seed = zlib.crc32(('%s/%s' % (label, family)).encode())
    rng = np.random.RandomState(seed % 2**31)
    if family == 'mantB':
        return _sparse(rng, a_shape, kc), _rich(rng, b_shape, family)
    return _rich(rng, a_shape, family), _sparse(rng, b_shape, kc)


def _exact(a, b, ta, tb):
    """float64 product of the stored operands under the transpose flags,
    over the last two axes."""
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    if ta:
        a = np.swapaxes(a, -1, -2)
    if tb:
        b = np.swapaxes(b, -1, -2)
    return a @ b


def _round_exact(exact):
    """bf16 rounding of float64 values that f32 holds exactly. A sum that
    starts from +0, as every accumulator here does, is never -0: `+ 0.0`
    gives the reference the same sign of zero."""
    v32 = (exact + 0.0).astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), exact)
    return _bf16(v32)


def _expected_bf16(label, family, exact):
    if family == 'int':
        # a condition on the inputs: see the module docstring
        assert np.abs(exact).max() <= 256, (label, np.abs(exact).max())
    else:
        assert np.abs(exact).max() < 2.0 ** 20, label
    return _round_exact(exact)


def _stored_shapes(m, n, k, ta, tb, batch=()):
    return (tuple(batch) + ((k, m) if ta else (m, k)),
            tuple(batch) + ((n, k) if tb else (k, n)))


def _bf16_case(label, m, n, k, ta, tb, batch=()):
    """[(family, a, b, expected)] for one bf16 case."""
    a_shape, b_shape = _stored_shapes(m, n, k, ta, tb, batch)
    out = []
    for fam in FAMILIES:
        a, b = _operands(label, fam, a_shape, b_shape, k)
        assert np.array_equal(_bf16(a), a) and np.array_equal(_bf16(b), b)
        out.append((fam, a, b, _expected_bf16(label, fam,
                                              _exact(a, b, ta, tb))))
    return out


def _feed(feeds, x, dtype):
    """Placeholder fed with x; bf16 goes in as f32 and is cast on the device
    (exact: x is bf16-representable)."""
    p = tf.placeholder(tf.float32, list(x.shape))
    feeds[p] = x
    return tf.cast(p, tf.bfloat16) if dtype == tf.bfloat16 else p


def _assert_equal(label, out, want):
    """Equal in every bit of every element (so -0.0 is not +0.0)."""
    assert out.dtype == want.dtype == np.float32 and \
        out.shape == want.shape, (label, out.dtype, out.shape, want.shape)
    bad = np.argwhere(np.ascontiguousarray(out).view(np.uint32) !=
                      np.ascontiguousarray(want).view(np.uint32))
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(
            '%s: %d of %d not equal; first at %s: got %r want %r; rows %s '
            'cols %s' % (label, len(bad), out.size, i, out[i], want[i],
                         sorted(set(bad[:, -2]))[:8],
                         sorted(set(bad[:, -1]))[:8]))


@pytest.fixture(scope='module')
def _sessions():
    state = {'sess': None, 'tests': 0}
    yield state
    if state['sess'] is not None:
        state['sess'].__exit__(None, None, None)


@pytest.fixture
def sess(_sessions):
    """One graph and one session shared by the tests of a module, which only
    add nodes; renewed every 64 tests, since a step's set-up time grows with
    the graph while opening a session costs more than any case here."""
    st = _sessions
    if st['sess'] is None or st['tests'] >= 64:
        if st['sess'] is not None:
            st['sess'].__exit__(None, None, None)
        tf.reset_default_graph()
        st['sess'] = _sess().__enter__()
        st['tests'] = 0
    st['tests'] += 1
    return st['sess']


def _run_bf16(sess, label, m, n, k, ta, tb, batch=()):
    feeds, ops = {}, []
    fams = _bf16_case(label, m, n, k, ta, tb, batch)
    for fam, a, b, _ in fams:
        ops.append(tf.matmul(_feed(feeds, a, tf.bfloat16),
                             _feed(feeds, b, tf.bfloat16),
                             transpose_a=ta, transpose_b=tb))
        assert ops[-1].op.type == ('BatchMatMul' if batch else 'MatMul')
    outs = sess.run(ops, feeds)
    for (fam, _, _, want), out in zip(fams, outs):
        _assert_equal('%s %s' % (label, fam), out, want)


# ---------------------------------------------------------------------------
# coverage self-check and input conditions (CPU)
# ---------------------------------------------------------------------------
def test_case_table_reaches_every_variant():
    routes = {c: _route(*c) for c in NT_CASES + PH8_CASES}
    # the mirrors agree with the numbers the case table was built on
    assert _pick_splitk(136, 136, 1096) == 2
    assert _pick_splitk(136, 136, 5184) == 10
    assert _pick_splitk(512, 1000, 2048) == 4
    for c in NT_CASES:
        assert routes[c]['mode'] != '8ph', c
    # every (tile, layout, mode) of the general template
    reached = {(r['tile'], r['layout'], r['mode']) for r in routes.values()}
    for combo in itertools.product(TILES, LAYOUTS, MODES):
        assert combo in reached, combo
    # split-K with the K tail in the second of two slices
    for (m, n) in TILE_SHAPES.values():
        r = routes[(m, n, 1096, False, True)]
        assert r['sk'] == 2 and not r['empty_slice'] and 1096 % 64, r
    # the empty last slice
    assert [c for c, r in routes.items() if r['empty_slice']] == [
        (136, 136, 5184, False, True), (136, 136, 5184, True, False)]
    # scalar K tail on NT, single and double buffered, on three tiles
    for k, mode in ((147, 'single'), (333, 'double')):
        assert 0 < k % 8 and k % 64
        tiles = {routes[c]['tile'] for c in NT_CASES
                 if c[2] == k and routes[c]['layout'] == (0, 0)
                 and routes[c]['mode'] == mode}
        assert tiles == {(128, 128), (32, 128), (64, 64)}, (k, tiles)
    # pre-transpose fallback: a stride that is no multiple of 8 is never
    # handed over K-major, and each such case runs under all four flags
    for c in NT_CASES:
        m, n, _, ta, tb = c
        a_km, b_km = routes[c]['layout']
        assert not (a_km and m % 8) and not (b_km and n % 8), c
    fallback = [c for c in NT_CASES
                if (c[3] and c[0] % 8) or (not c[4] and c[1] % 8)]
    assert {c[:3] for c in fallback} == {(100, 60, 200), (130, 60, 328),
                                         (60, 130, 1096)}
    assert {routes[c]['mode'] for c in fallback} == {'single', 'double',
                                                     'splitk'}
    # the NT interior fast path keeps a case the 8-phase kernel cannot take:
    # an interior block (m, n >= tile) with a full first K tile
    r = routes[(136, 136, 328, False, True)]
    assert (r['layout'], r['mode'], r['tile']) == ((0, 0), 'double',
                                                   (128, 128))
    # 8-phase: every NR with one and with several column tiles, both M, and
    # K loops below, at, one past and far past the ring depth of 2
    seen = set()
    for c in PH8_CASES:
        r = routes[c]
        assert r['mode'] == '8ph' and r['layout'] == (0, 0), c
        seen.add((c[0] // 256, r['nr'], c[1] // (64 * r['nr']) > 1,
                  c[2] // 64))
    for nr, several in itertools.product((1, 2, 4), (False, True)):
        for kt in (1, 2, 3, 15):
            assert (1, nr, several, kt) in seen, (nr, several, kt)
        assert (2, nr, several, 3) in seen, (nr, several)
    # BatchMatMul (stf_gemm_bf16, no split-K): an aligned shape, and one
    # whose K-major strides and batch offsets are no multiples of 8
    m, n, k = BMM_SHAPES[1]
    assert m % 8 and n % 8 and k % 8 and (m * k) % 8 and (k * n) % 8
    assert _pick_tile(m, n) == (64, 64) and m < 64 and n < 64
    m, n, k = BMM_SHAPES[2]
    assert (m * k) % 2 and (k * n) % 2 and m % 2 and n % 2 and k % 2
    assert _pick_tile(m, n) == (64, 64) and m > 64 and n > 64 and k > 64
    m, n, k = BMM_SHAPES[0]
    assert m % 8 == 0 and n % 8 == 0 and k % 8 == 0 and not _8ph_ok(m, n, k)


@pytest.mark.parametrize('case', NT_CASES + PH8_CASES, ids=_cid)
def test_reference_conditions(case):
    """The inputs satisfy the exactness conditions (max|exact| <= 256 for the
    small-integer family): the reference side alone, no GPU."""
    _bf16_case(_cid(case), *case)


@pytest.mark.parametrize('m,n,k', BMM_SHAPES)
@pytest.mark.parametrize('ta,tb', FLAGS)
def test_reference_conditions_batch(m, n, k, ta, tb):
    _bf16_case('bmm-' + _cid((m, n, k, ta, tb)), m, n, k, ta, tb, (3,))


# ---------------------------------------------------------------------------
# GPU: bf16
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('case', NT_CASES, ids=_cid)
def test_matmul_bf16_nt_template(sess, case):
    _run_bf16(sess, _cid(case), *case)


@pytest.mark.gpu
def test_splitk_ops_of_one_step_share_the_arena(sess):
    """Independent split-K ops of one step are enqueued from different
    executor threads and all accumulate into the one pre-zeroed arena: each
    op's accumulation and its cast-and-rezero must reach the stream as a
    pair (SplitKInto). When they interleaved, one op returned the sum of two
    results and the other zeros."""
    feeds, ops, wants = {}, [], []
    for i in range(12):
        m, n, k = ((72, 72, 1096), (24, 136, 1096), (136, 72, 1096))[i % 3]
        assert _route(m, n, k, False, False)['mode'] == 'splitk'
        label = 'arena-%d' % i
        for fam, a, b, want in _bf16_case(label, m, n, k, False, False)[:2]:
            ops.append(tf.matmul(_feed(feeds, a, tf.bfloat16),
                                 _feed(feeds, b, tf.bfloat16)))
            wants.append(('%s %s' % (label, fam), want))
    for (label, want), out in zip(wants, sess.run(ops, feeds)):
        _assert_equal(label, out, want)


@pytest.mark.gpu
@pytest.mark.parametrize('case', PH8_CASES, ids=_cid)
def test_matmul_bf16_8phase(sess, case):
    _run_bf16(sess, _cid(case), *case)


@pytest.mark.gpu
@pytest.mark.parametrize('m,n,k', BMM_SHAPES)
@pytest.mark.parametrize('ta,tb', FLAGS)
def test_batch_matmul_bf16(sess, m, n, k, ta, tb):
    _run_bf16(sess, 'bmm-' + _cid((m, n, k, ta, tb)), m, n, k, ta, tb, (3,))


# ---------------------------------------------------------------------------
# GPU: f32
# ---------------------------------------------------------------------------
def _f32_ints(label, m, n, k, ta, tb, batch):
    rng = np.random.RandomState(zlib.crc32(label.encode()) % 2**31)
    a_shape, b_shape = _stored_shapes(m, n, k, ta, tb, batch)
    a = rng.randint(-64, 65, a_shape).astype(np.float32)
    b = rng.randint(-64, 65, b_shape).astype(np.float32)
    exact = _exact(a, b, ta, tb)
    assert np.abs(exact).max() < 2.0 ** 24, label
    return a, b, (exact + 0.0).astype(np.float32)   # +0, as an f32 sum from 0


@pytest.mark.gpu
@pytest.mark.parametrize('batch', [(), (3,)], ids=['matmul', 'batch3'])
@pytest.mark.parametrize('m,n,k', F32_SHAPES)
def test_matmul_f32_integers_exact(sess, m, n, k, batch):
    feeds, ops, wants = {}, [], []
    for ta, tb in FLAGS:
        label = 'f32-%s%s' % ('b3-' if batch else '', _cid((m, n, k, ta, tb)))
        a, b, want = _f32_ints(label, m, n, k, ta, tb, batch)
        ops.append(tf.matmul(_feed(feeds, a, tf.float32),
                             _feed(feeds, b, tf.float32),
                             transpose_a=ta, transpose_b=tb))
        assert ops[-1].op.type == ('BatchMatMul' if batch else 'MatMul')
        wants.append((label, want))
    for (label, want), out in zip(wants, sess.run(ops, feeds)):
        _assert_equal(label, out, want)


@pytest.mark.gpu
@pytest.mark.parametrize('batch', [(), (3,)], ids=['matmul', 'batch3'])
def test_matmul_f32_randn_dot_product_bound(sess, batch):
    """|fl(a.b) - a.b| <= gamma_K * |a|.|b| for a length-K f32 dot product
    summed in any order, fused or not (Higham, Accuracy and Stability of
    Numerical Algorithms, 2nd ed., eq. 3.5), on every element."""
    m, n, k = 200, 300, 150
    rng = np.random.RandomState(3)
    a = rng.randn(*(batch + (m, k))).astype(np.float32)
    b = rng.randn(*(batch + (k, n))).astype(np.float32)
    feeds = {}
    out = sess.run(tf.matmul(_feed(feeds, a, tf.float32),
                             _feed(feeds, b, tf.float32)), feeds)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    u = 2.0 ** -24
    gamma = k * u / (1 - k * u)
    err = np.abs(out.astype(np.float64) - a64 @ b64)
    bound = gamma * (np.abs(a64) @ np.abs(b64))
    print('f32 randn: max err/bound %.3g' % (err / bound).max())
    assert out.shape == bound.shape and np.all(err <= bound)
