"""CPU tier of tests/reduce_exact.py: every case against the float64 reference on the kernel SOURCE of csrc/elementwise.hip / centernet_net.hip through
tests/hip_cpu_backend.py, which proves the cases, the references and the bounds before a GPU sees them (the emulation's rsqrtf is 1 / sqrtf, two roundings; its
products are not contracted).  No case is GPU-only: the two long L2-norm cases take five to seven seconds each here (the backward one with one variant
per reduction mode instead of all eight)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hip_cpu_backend as HC  # noqa: E402
import reduce_exact as RX  # noqa: E402

CPU = torch.device('cpu')
DTS = ['f32', 'bf16']


def _ops():
    import odtk  # noqa: F401
    from odtk import ops
    return ops


def _cases(cases):
    return pytest.mark.parametrize('case', cases, ids=[RX.case_id(c) for c in cases])


def test_the_tie_rule_of_the_pooling_reference_is_pinned():
    RX.reference_tie_rule_is_pinned(_ops())


@pytest.mark.parametrize('dt', DTS)
@_cases(RX.POOL_CASES)
def test_max_pooling(case, dt):
    with HC.installed():
        RX.run_pool(_ops(), CPU, case, dt)


@pytest.mark.parametrize('dt', DTS)
@_cases(RX.COLSUM_CASES)
def test_colsum(case, dt):
    with HC.installed():
        RX.run_colsum(_ops(), CPU, case, dt)


@pytest.mark.parametrize('n', RX.OPT_NS)
def test_sgd_momentum(n):
    with HC.installed():
        RX.run_sgd(_ops(), CPU, n)


@pytest.mark.parametrize('n', RX.SUM_NS)
def test_sum_f32_and_loss_total(n):
    with HC.installed():
        RX.run_sums(_ops(), CPU, n)


@pytest.mark.parametrize('dt', DTS)
@_cases(RX.L2_CASES)
def test_l2norm(case, dt):
    with HC.installed():
        print('largest K needed (bound: %d):' % RX.K_ULP, RX.run_l2norm(_ops(), CPU, case, dt))


@pytest.mark.parametrize('n', RX.OPT_NS)
def test_adam(n):
    with HC.installed():
        print('largest K needed (bound: %d):' % RX.K_ULP, RX.run_adam(_ops(), CPU, n))
