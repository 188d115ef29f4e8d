"""CPU tier of the bit-exact convolution tests: proves the TESTS (tests/conv_exact.py, tests/test_gpu_conv_exact.py) without a GPU.
 * the generators' bounds and coverage properties on every case of every list the GPU module walks;
 * the f32 reference equals the f64 reference;
 * the GPU test bodies, unchanged, on tests/mock_ops.py (device 'cpu'): descriptors, layouts, guard bands and pad handling of the test code;
 * four mutants of the mock (one dropped term, one dropped pixel of the filter gradient, a guard row read unmasked, a write into an output guard): each must
   fail the exact comparison; the first two also go through the Gaussian data and 2e-2 bound of test_gpu_kernels._conv_case, reported, not asserted."""
import contextlib
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conv_exact as CE  # noqa: E402
import mock_ops  # noqa: E402
import test_gpu_conv_exact as G  # noqa: E402
import test_gpu_kernels as GK  # noqa: E402

BATCH32 = [(32,) + c[1:] for c in GK.SSD300_LAYER_CASES]
ALL_CASES = sorted(set(GK.CONV_CASES + GK.V3_EXTRA_CASES + GK.V9_EXTRA_CASES + GK.HALO128_CASES + GK.SSD300_LAYER_CASES + BATCH32 + GK.BACKBONE_CASES + GK.X3_CASES))
# every case is generated here (the generators assert their bounds themselves); only the f64 repeat of the reference is limited, to cases of at most F64_MACS
# multiply-adds per pass
F64_MACS = 2e9


def _macs(case):
    N, H, W, C, K, k, s, d = case
    return N * CE.same_out(H, s) * CE.same_out(W, s) * K * k * k * C


# ------------------------------------------------------------------------------------------------------------ generators
@pytest.mark.parametrize("case", ALL_CASES)
def test_coverage_of_the_sparsity_patterns(case):
    N, H, W, C, K, k, s, d = case
    Mo = N * CE.same_out(H, s) * CE.same_out(W, s)
    hit = torch.zeros(k, k, C, dtype=torch.bool)
    for r in range(CE.rounds_fwd(case, 'A')):
        w = CE.filter_fwd_A(case, r)
        assert set(w.unique().tolist()) <= {-1.0, 0.0, 1.0} and int((w != 0).reshape(K, -1).sum(1).max()) <= CE.CAP
        hit |= (w != 0).any(0)
    assert bool(hit.all()), 'forward A: a (tap, channel) position that no output channel reads'
    hit = torch.zeros(K, k, k, dtype=torch.bool)
    for r in range(CE.rounds_dgrad(case, 'A')):
        w = CE.filter_dgrad_A(case, r)
        assert int((w != 0).permute(3, 0, 1, 2).reshape(C, -1).sum(1).max()) <= CE.CAP
        hit |= (w != 0).any(3)
    assert bool(hit.all()), 'input gradient A: a (k, tap) position that no input channel reads'
    m = CE.per_pixel(k)
    for M, Cn, rounds in ((N * H * W, C, CE.rounds_fwd(case, 'B')), (Mo, K, CE.rounds_dgrad(case, 'B'))):
        hit = torch.zeros(Cn, dtype=torch.bool)
        for r in range(rounds):
            mask = CE.rotating_mask(M, Cn, m, r)
            assert int(mask.sum(1).max()) <= m and m * k * k <= CE.CAP
            hit |= mask.any(0)
        assert bool(hit.all()), 'B: a channel that no pixel carries'


@pytest.mark.parametrize("case", ALL_CASES)
def test_bounds_hold_and_f32_reference_equals_f64(case):
    torch.set_num_threads(16)
    f64 = _macs(case) <= F64_MACS
    for arr in ('A', 'B'):
        for r in range(CE.rounds_fwd(case, arr)):
            z = CE.forward_operands(case, arr, r)[3]                       # (asserts |z| <= 256 itself)
            assert torch.equal(z, z.round()) and torch.equal(z.bfloat16().float(), z)
            if f64 and r == 0:
                assert torch.equal(CE.forward_operands(case, arr, r, torch.float64)[3].float(), z)
            del z
        for r in range(CE.rounds_dgrad(case, arr)):
            o = None                                                       # (the largest cases hold several GB per pass)
            o = CE.dgrad_operands(case, arr, r)
            assert torch.equal(o[4].bfloat16().float(), o[4]) and torch.equal(o[5].bfloat16().float(), o[5])
            if f64 and r == 0:
                o64 = CE.dgrad_operands(case, arr, r, torch.float64)
                assert torch.equal(o64[4].float(), o[4]) and torch.equal(o64[5].float(), o[5])
    for bounded in (False, True):
        x, dy, dw, db = CE.wgrad_operands(case, bounded)
        if f64:
            _, _, dw64, db64 = CE.wgrad_operands(case, bounded, torch.float64)
            assert torch.equal(dw64.float(), dw) and torch.equal(db64.float(), db)


# ------------------------------------------------------------------------------------------------------------ the GPU bodies on the mock
def _filter_prepare(w, K, R, S, C_, Kp, dtype, w_c, w_t):
    wf = w.float().reshape(K, R * S, C_)
    if w_c is not None:
        w_c.copy_(wf.reshape(-1).to(w_c.dtype))
    if w_t is not None:
        full = torch.zeros(C_, R * S, Kp)
        full[:, :, :K] = wf.permute(2, 1, 0).flip(1)
        w_t.copy_(full.reshape(-1).to(w_t.dtype))


@contextlib.contextmanager
def cpu_ops(**mutants):
    """tests/mock_ops.installed() + what the conv tests need besides the launches (filter layouts, debug keys, the name of the last kernel); `mutants` replace
    launches of the mock by wrong ones"""
    from odtk import ops
    last = {'name': ''}
    with mock_ops.installed():
        names = ('filter_prepare', 'debug_set', 'conv_last_kernel', 'conv2d_fwd', 'conv2d_dgrad', 'conv2d_wgrad')
        old = {n: getattr(ops, n) for n in names}
        sync = torch.cuda.synchronize

        def named(fn, tag):
            def f(d, *a, **k):
                last['name'] = f'conv_{tag}_kernel(mock)' + ('+x3' if d.dtype == ops.F32X3 else '')
                return fn(d, *a, **k)
            return f
        try:
            ops.filter_prepare = _filter_prepare
            ops.debug_set = lambda key, value: None
            ops.conv_last_kernel = lambda: last['name']
            for n, tag in (('conv2d_fwd', 'fwd'), ('conv2d_dgrad', 'dgrad'), ('conv2d_wgrad', 'wgrad')):
                setattr(ops, n, named(mutants.get(n, old[n]), tag))
            torch.cuda.synchronize = lambda *a, **k: None
            yield
        finally:
            torch.cuda.synchronize = sync
            for n, v in old.items():
                setattr(ops, n, v)


CPU_SUBSET = [GK.CONV_CASES[0], GK.CONV_CASES[1], GK.CONV_CASES[2], GK.CONV_CASES[5], GK.CONV_CASES[6], GK.BACKBONE_CASES[0], GK.BACKBONE_CASES[5],
              GK.BACKBONE_CASES[16], GK.BACKBONE_CASES[20], GK.V9_EXTRA_CASES[0], GK.V9_EXTRA_CASES[4]]


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("case", CPU_SUBSET)
def test_gpu_bodies_pass_exactly_on_the_mock(case, dt):
    with cpu_ops():
        ran = G.exact_case(case, dt, 'cpu')
    assert ran == {'fwd': {'conv_fwd_kernel(mock)'}, 'wgrad': {'conv_wgrad_kernel(mock)'}, 'dgrad': {'conv_dgrad_kernel(mock)'}}


def test_gpu_test_functions_run_unchanged_on_the_mock():
    with cpu_ops():
        G.test_exact_legacy_engine(GK.CONV_CASES[3], 'cpu')
        G.test_exact_v9_engine(GK.V9_EXTRA_CASES[2], 'cpu', None)
        G.test_exact_halo_kernel_on_128x128_tiles((1, 6, 7, 64, 72, 3, 1, 1), 16384, 'cpu')
        G.test_exact_ssd300_layer_geometries(GK.SSD300_LAYER_CASES[-1], 'cpu')
        G.test_exact_filter_gradient_split_reduce_with_rsc_not_a_multiple_of_8('cpu')
        G.test_exact_x3_operand_splitting(GK.X3_CASES[5], 'cpu')
        G.test_exact_x3_operand_splitting(GK.X3_CASES[8], 'cpu')


# ------------------------------------------------------------------------------------------------------------ mutants
MUT_CASE = GK.CONV_CASES[0]


def _fwd_with(edit):
    """the mock's forward pass with `edit(pre-activation rows [M][K] f32, d, x, w)` applied before the ReLU and the store"""
    def fwd(d, x, w, bias, y, relu):
        z = torch.zeros(y.shape[0], d.K)
        mock_ops.conv2d_fwd(d, x, w, bias, z, False)
        edit(z, d, x, w, bias)
        y[:, :d.K] = (torch.relu(z) if relu else z).to(y.dtype)
    return fwd


def _drop_one_term(z, d, x, w, bias):
    """output pixel (0, 5, 7): the centre tap's product with ONE input channel is missing (from every output channel that reads it: one term per output element)"""
    row = 5 * d.Wo + 7
    wv = w.float().reshape(d.K, d.R, d.S, d.C)[:, d.R // 2, d.S // 2, :]
    for c in range(d.C):
        term = wv[:, c] * float(x[5 * d.stride * d.W + 7 * d.stride, c])
        if bool(((term != 0) & (z[row] > 1)).any()):           # (visible through the ReLU)
            z[row] -= term
            return
    raise RuntimeError('no droppable term')


def _leak_guard_row(z, d, x, w, bias):
    """output pixel (0, 0, 0) reads the pixel above it -- outside the image, in memory the guard band in front of x -- as if the halo mask were missing"""
    flat, off = mock_ops._storage(x)
    above = flat[off - d.W * d.ldx: off - d.W * d.ldx + d.C].float()
    z[0] += (w.float().reshape(d.K, d.R, d.S, d.C)[:, 0, 1, :] * above).sum(-1)


def _wgrad_drops_last_pixel(d, x, dy, lddy, dw, dbias=None):
    short = dy.clone()
    short[-1] = 0
    mock_ops.conv2d_wgrad(d, x, short, lddy, dw, None)
    if dbias is not None:
        dbias[: d.K] += dy[:, :d.K].float().sum(0)


def _fwd_writes_into_guard(d, x, w, bias, y, relu):
    mock_ops.conv2d_fwd(d, x, w, bias, y, relu)
    flat, off = mock_ops._storage(y)
    flat[off - 1] = 1.0


def _gaussian_bound_sees(**mutants):
    with cpu_ops(**mutants):
        try:
            GK._conv_case(MUT_CASE, 'bf16', 'cpu')
        except AssertionError as e:
            return f'yes ({str(e)[:40]})'
    return 'NO'


@pytest.mark.parametrize("name,mutants,expect,gaussian", [
    ('one (pixel, tap, channel) term dropped', dict(conv2d_fwd=_fwd_with(_drop_one_term)), 'forward A', True),
    ('last pixel missing from the filter-gradient sum', dict(conv2d_wgrad=_wgrad_drops_last_pixel), 'filter gradient x1', True),
    ('a guard row read as if a mask were missing', dict(conv2d_fwd=_fwd_with(_leak_guard_row)), 'forward A', False),
    ('one element written into an output guard', dict(conv2d_fwd=_fwd_writes_into_guard), 'wrote outside its output', False)],
    ids=['dropped-term', 'dropped-pixel', 'guard-leak', 'guard-write'])
def test_mutants_fail_the_exact_comparison(name, mutants, expect, gaussian):
    with cpu_ops():
        G.exact_case(MUT_CASE, 'bf16', 'cpu')                       # the unmutated mock passes
    seen = _gaussian_bound_sees(**mutants) if gaussian else 'not run'
    note = f'{name}: does the Gaussian data with the 2e-2 bound of test_gpu_kernels._conv_case see it: {seen}'
    print(note)
    with cpu_ops(**mutants):
        with pytest.raises(AssertionError) as e:
            G.exact_case(MUT_CASE, 'bf16', 'cpu')
    assert expect in str(e.value), f'{note}; the exact comparison failed elsewhere: {e.value}'
