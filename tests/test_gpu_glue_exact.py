"""Bit-exact, guarded GPU tests of the data-moving kernels between the layers (csrc/elementwise.hip: add2d, upsample2x_*, copy_channels, rows_to_f32 /
rows_from_f32, exp_rows_*, the casts; csrc/centernet_net.hip: add_relu_fwd, relu_bwd, avgpool2x2_*, preprocess_norm) through odtk.ops, on the cases and float64
references of tests/glue_exact.py (proved on the CPU by tests/test_glue_exact_cpu.py): pitched operands and channel slices of wider buffers, sentinel pad columns,
guard rows around every operand (inputs included), in-place calls as the models make them, every dispatch route of the casts, and one launch per kernel family
whose grid-stride loop runs a second time.  Plus the GPU twin of test_hip_cpu.py::test_global_batch_norm_entry_points_from_source."""
import contextlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_exact as GX  # noqa: E402

pytestmark = pytest.mark.gpu
DTS = ['f32', 'bf16']


def _ops():
    import odtk  # noqa: F401
    from odtk import ops
    return ops


def _cases(cases):
    return pytest.mark.parametrize('case', cases, ids=[GX.case_id(c) for c in cases])


@pytest.mark.parametrize('dt', DTS)
@_cases(GX.ADD_CASES)
def test_copies_and_adds(case, dt, dev):
    GX.run_add(_ops(), dev, case, dt)


@pytest.mark.parametrize('dt', DTS)
@_cases(GX.RELU_CASES)
def test_relu_pair(case, dt, dev):
    GX.run_relu(_ops(), dev, case, dt)


@pytest.mark.parametrize('dt', DTS)
@_cases(GX.UP_CASES)
def test_upsampling(case, dt, dev):
    GX.run_upsample(_ops(), dev, case, dt)


@pytest.mark.parametrize('dt', DTS)
@_cases(GX.AVG_CASES + GX.PRE_CASES)
def test_average_pooling_and_preprocess_norm(case, dt, dev):
    (GX.run_avgpool if case in GX.AVG_CASES else GX.run_preprocess_norm)(_ops(), dev, case, dt)


@pytest.mark.parametrize('dt', DTS)
@_cases(GX.ROWS_CASES)
def test_rows_to_and_from_f32(case, dt, dev):
    GX.run_rows(_ops(), dev, case, dt)


@pytest.mark.parametrize('dt', DTS)
@_cases(GX.EXP_CASES)
def test_exp_rows(case, dt, dev):
    # exp_rows_to_f32 is allowed what torch.exp in f32 loses on the same device and inputs against float64 exp, + 1 ulp (it may use a different expf); both
    # figures are measured in the test.  Measured on an MI355X over these 32 cases: kernel and torch.exp agree case by case, 0.803 ulp at worst (M=257, C=72, f32),
    # so the bound in force is 1.803 ulp; exp(-88), a subnormal f32, is not flushed by either.
    GX.run_exp(_ops(), dev, case, dt)


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('n', GX.CAST_NS)
def test_casts(n, dt, dev):
    GX.run_cast(_ops(), dev, n, dt)


@pytest.mark.parametrize('name,dt', GX.OVERCAP, ids=[f'{n}-{d}' for n, d in GX.OVERCAP])
def test_over_the_cap(name, dt, dev):
    """total > cap * 256 by one partial workgroup, per launch (sizes and caps: tests/glue_exact.py); the operands of one case are freed before the next"""
    try:
        GX.run_overcap(_ops(), dev, name, dt)
    finally:
        torch.cuda.empty_cache()


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('shape', GX.BN_GLOBAL_SHAPES)
def test_global_batch_norm_entry_points(shape, dt, dev):
    """odtk_bn_moments / _fwd_given / _bwd_sums / _bwd_given on the GPU: the body and the bounds of test_hip_cpu.py::test_global_batch_norm_entry_points_from_source"""
    GX.global_batch_norm_case(_ops(), dev, shape, dt, contextlib.nullcontext())
