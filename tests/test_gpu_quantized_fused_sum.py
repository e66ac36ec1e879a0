"""QuantizedConv2DWithBiasSumAndRequantize on the GPU (GemmI8FusedSum in
csrc/kernels/hip/gemm_i8_fused.hip) against the numpy reference and the cases
of tests/test_quantized_fused_sum.py; every input comes through a placeholder,
so nothing is folded onto the CPU. All tests need a gfx950 GPU."""
import numpy as np
import pytest

from test_gpu_quantized import _trace_run
from test_gpu_quantized_fused import sess  # noqa: F401 - the fixture
from test_quantized_fused_sum import CASES, PARAMS, check_sum_case, param_id

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('param', PARAMS, ids=param_id)
def test_fused_sum_op(sess, param):
    check_sum_case(sess, '/gpu:0', *param)


def test_fused_sum_node_runs_on_the_gpu(sess):
    """In a trace, and again past the point where the step is captured and
    replayed."""
    outs, feeds, want = check_sum_case(sess, '/gpu:0', CASES[1], 'Relu',
                                       'random', 1)
    got, on_gpu = _trace_run(sess, outs, feeds)
    assert outs[0].op.name in on_gpu, sorted(on_gpu)
    for _ in range(5):
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        got = sess.run(outs, feeds)
