"""Exact, guarded GPU tests of the kernels that reduce or select (csrc/elementwise.hip: the six max-pooling entry points, colsum, sgd_momentum, sum_f32, loss_total,
l2norm_fwd / _bwd; csrc/centernet_net.hip: adam) through odtk.ops, on the cases and float64 references of tests/reduce_exact.py (proved on the kernel source by
tests/test_reduce_exact_cpu.py): pitched operands, maps smaller than their window, ties, every tail and block edge of the optimisers, the second grid trip of the
L2-norm kernels, guard rows around every operand (inputs and workspaces included).  Bit for bit wherever the kernel neither divides nor takes a root; the L2-norm
and Adam within  |ref32 - ref64| + K ulp_f32(ref64)  of float64, K = reduce_exact.K_ULP = 4.  Largest K needed on an MI355X: l2norm_fwd y 1.59, l2norm_bwd dx 2.00,
adam p 2.00, m 0.00, v 0.00, cast copy 2.00; dgamma used 0.17 of its bound (on the CPU emulation: 0, 0, 1.00, 0, 0, 1.00 and 0.17)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reduce_exact as RX  # noqa: E402

pytestmark = pytest.mark.gpu
DTS = ['f32', 'bf16']


def _ops():
    import odtk  # noqa: F401
    from odtk import ops
    return ops


def _cases(cases):
    return pytest.mark.parametrize('case', cases, ids=[RX.case_id(c) for c in cases])


@pytest.mark.parametrize('dt', DTS)
@_cases(RX.POOL_CASES)
def test_max_pooling(case, dt, dev):
    RX.run_pool(_ops(), dev, case, dt)


@pytest.mark.parametrize('dt', DTS)
@_cases(RX.COLSUM_CASES)
def test_colsum(case, dt, dev):
    RX.run_colsum(_ops(), dev, case, dt)


@pytest.mark.parametrize('n', RX.OPT_NS)
def test_sgd_momentum(n, dev):
    RX.run_sgd(_ops(), dev, n)


@pytest.mark.parametrize('n', RX.SUM_NS)
def test_sum_f32_and_loss_total(n, dev):
    RX.run_sums(_ops(), dev, n)


@pytest.mark.parametrize('dt', DTS)
@_cases(RX.L2_CASES)
def test_l2norm(case, dt, dev):
    print('largest K needed (bound: %d):' % RX.K_ULP, RX.run_l2norm(_ops(), dev, case, dt))


@pytest.mark.parametrize('n', RX.OPT_NS)
def test_adam(n, dev):
    print('largest K needed (bound: %d):' % RX.K_ULP, RX.run_adam(_ops(), dev, n))
