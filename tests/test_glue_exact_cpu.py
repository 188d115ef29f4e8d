"""CPU tier of tests/glue_exact.py: every small case (not the over-the-cap group) against the float64 reference, two ways -- 'source': the kernel SOURCE of
csrc/elementwise.hip / centernet_net.hip through tests/hip_cpu_backend.py, which proves the cases and the reference before a GPU sees them; 'mock': the
restatements of tests/mock_ops.py, which the in-situ shadows (tests/insitu.py) compare the kernels with at model shapes and Frobenius tolerances -- here they are
pinned, bit for bit, pad columns and in-place calls included, to a reference that is independent of both."""
import contextlib
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import glue_exact as GX  # noqa: E402
import hip_cpu_backend as HC  # noqa: E402
import mock_ops  # noqa: E402

CPU = torch.device('cpu')
BACKENDS = ['source', 'mock']
DTS = ['f32', 'bf16']


@contextlib.contextmanager
def _ops(backend):
    import odtk  # noqa: F401
    from odtk import ops
    with (HC.installed() if backend == 'source' else mock_ops.installed()):
        yield ops


def _cases(cases):
    return pytest.mark.parametrize('case', cases, ids=[GX.case_id(c) for c in cases])


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('dt', DTS)
@_cases(GX.ADD_CASES)
def test_copies_and_adds(case, dt, backend):
    with _ops(backend) as ops:
        GX.run_add(ops, CPU, case, dt)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('dt', DTS)
@_cases(GX.RELU_CASES)
def test_relu_pair(case, dt, backend):
    with _ops(backend) as ops:
        GX.run_relu(ops, CPU, case, dt)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('dt', DTS)
@_cases(GX.UP_CASES)
def test_upsampling(case, dt, backend):
    with _ops(backend) as ops:
        GX.run_upsample(ops, CPU, case, dt)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('dt', DTS)
@_cases(GX.AVG_CASES)
def test_average_pooling(case, dt, backend):
    with _ops(backend) as ops:
        GX.run_avgpool(ops, CPU, case, dt)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('dt', DTS)
@_cases(GX.ROWS_CASES)
def test_rows_to_and_from_f32(case, dt, backend):
    with _ops(backend) as ops:
        GX.run_rows(ops, CPU, case, dt)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('dt', DTS)
@_cases(GX.EXP_CASES)
def test_exp_rows(case, dt, backend):
    """(bound: torch.exp in f32 on the CPU + 1 ulp; the emulated kernel calls glibc's expf)"""
    with _ops(backend) as ops:
        GX.run_exp(ops, CPU, case, dt)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('dt', DTS)
@_cases(GX.PRE_CASES)
def test_preprocess_norm(case, dt, backend):
    with _ops(backend) as ops:
        GX.run_preprocess_norm(ops, CPU, case, dt)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('n', GX.CAST_NS)
def test_casts(n, dt, backend):
    with _ops(backend) as ops:
        GX.run_cast(ops, CPU, n, dt)


def test_over_the_cap_sizes_exceed_the_caps_in_the_source():
    """the caps the over-the-cap group of the GPU tier is sized from are the ones the sources launch with"""
    import re
    csrc = os.path.join(os.path.dirname(HERE), 'object-detection-tensorflow_amd', 'csrc')
    ew = open(os.path.join(csrc, 'elementwise.hip')).read()
    cn = open(os.path.join(csrc, 'centernet_net.hip')).read()
    assert re.search(r'grid_for\(long long total, int threads, int cap = (\d+)\)', ew).group(1) == str(GX.CAP_SMALL)
    assert re.search(r'grid_for\(long long total, int threads, int cap = (\d+)\)', cn).group(1) == str(GX.CAP_LARGE)
    for kernel, src, cap in [('cast_f32_to_bf16_x8_kernel', ew, None), ('cast_bf16_to_f32_x8_kernel', ew, None), ('cast_kernel<T>', ew, None),
                             ('cast_to_f32_kernel<T>', ew, None), ('add2d_kernel<T>', ew, GX.CAP_LARGE), ('upsample2x_fwd_kernel<T>', ew, GX.CAP_LARGE),
                             ('upsample2x_bwd_kernel<T>', ew, GX.CAP_LARGE), ('copy_channels_kernel<T>', ew, GX.CAP_LARGE), ('rows_to_f32_kernel<T>', ew, GX.CAP_LARGE),
                             ('rows_from_f32_kernel<T>', ew, GX.CAP_LARGE), ('exp_rows_to_f32_kernel<T>', ew, GX.CAP_LARGE), ('exp_rows_bwd_kernel<T>', ew, GX.CAP_LARGE),
                             ('add_relu_kernel<T>', cn, None), ('relu_bwd_kernel<T>', cn, None), ('(avgpool2x2_kernel<T, false>)', cn, None),
                             ('(avgpool2x2_kernel<T, true>)', cn, None), ('preprocess_norm_kernel<T>', cn, GX.CAP_SMALL)]:
        m = re.search(r'hipLaunchKernelGGL\(' + re.escape(kernel) + r', dim3\(grid_for\((.*?), 256(?:, (\d+))?\)\), dim3\(256\)', src)
        assert m, kernel
        assert m.group(2) == (None if cap is None else str(cap)), (kernel, m.group(2))
