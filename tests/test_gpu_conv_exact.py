"""Bit-exact tests of every convolution kernel and pass (csrc/conv.hip, conv_v3.hip, conv_v9.hip) through the C-ABI, on the integer operands of
tests/conv_exact.py: forward + bias + ReLU, input gradient (plain, ReLU-masked + accumulated, wider dy pitch), filter + bias gradient (deterministic and atomic
flush, second call = twice the first), the fused / two-launch 2 x 2 pooling epilogue and the sign-bit pair -- all with torch.equal against the f32 CPU reference,
over the case lists and engine fixtures of tests/test_gpu_kernels.py (imported, not copied).  Every operand and result sits between guard bands inside one
allocation; output guards and pad columns must come back untouched.

The Gaussian tests of test_gpu_kernels.py stay what checks the rounding of non-representable values; these check that every term is there exactly once.

Run time, one MI355X box, back to back: tests/test_gpu_kernels.py 65 s (862 cases), this module 128 s (625 cases, 2.0 x; the references are cached across the
engine fixtures, tests/conv_exact.py).  No case was cut.  One repeat was: under the forced-engine fixtures (v3 / legacy / v9 / 128 x 128 tiles) the pooling
entry point is checked only where it runs as ONE launch; its two-launch form -- the convolution just checked, then the engine-independent pool kernel -- is
checked by the auto-dispatch tests (SSD300 layers at both batches, CONV_CASES, backbone).  With it repeated there as well the module took 131 - 138 s."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_exact as CE  # noqa: E402
from test_gpu_kernels import (BACKBONE_CASES, CONV_CASES, HALO128_CASES, SSD300_LAYER_CASES, V3_EXTRA_CASES, V9_EXTRA_CASES, X3_CASES,  # noqa: E402,F401
                              v3_engine, v9_engine)

pytestmark = pytest.mark.gpu


def _ops():
    import odtk  # noqa: F401
    from odtk import ops
    return ops


def _sync(dev):
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()


def _check(buf, exp_rows, shape, what, ops, kern=None):
    """buf: CE.Guarded result; exp_rows: [M][ld] CPU reference (pad columns zero).  Bit equality, guards untouched."""
    kern = ops.conv_last_kernel() if kern is None else kern
    got = buf.view.reshape(exp_rows.shape).float().cpu()
    exp = exp_rows.float()
    if not torch.equal(got, exp):
        raise AssertionError(f'{what} [{kern}]: {CE.describe_mismatch(got, exp, shape)}')
    if not buf.guards_intact():
        raise AssertionError(f'{what} [{kern}]: wrote outside its output: (row relative to the tensor, column, value) {buf.first_guard_damage()}')


def _prefilled(exp_rows, K, value=7.0):
    """an output buffer's content before the launch: `value` where the kernel must write, zero in the pad columns (which stay zero, as in to_rows)"""
    t = torch.zeros_like(exp_rows)
    t[:, :K] = value
    return t


def _filters(ops, w_pad, K, k, ldx, Kp, DT, dtype, dev):
    """both filter layouts between guards"""
    wm = CE.Guarded(w_pad.reshape(-1), torch.float32, dev, CE.GUARD_IN)
    w_c = CE.Guarded(torch.zeros(K * k * k * ldx), dtype, dev, CE.GUARD_IN)
    w_t = CE.Guarded(torch.zeros(ldx * k * k * Kp), dtype, dev, CE.GUARD_IN)
    ops.filter_prepare(wm.view, K, k, k, ldx, Kp, DT, w_c.view, w_t.view)
    return w_c, w_t


def exact_case(case, dt, dev, arrangements=('A', 'B'), kpad=None, forced=False):
    """dt: 'bf16' | 'f32' | 'x3'; forced: under an engine fixture (see _pool_case).  Returns the names of ALL kernels that ran, per pass (for the callers that assert on the dispatch)."""
    ops = _ops()
    N, H, W, C, K, k, stride, dil = case
    dtype = torch.bfloat16 if dt == 'bf16' else torch.float32
    DT = {'bf16': ops.BF16, 'f32': ops.F32, 'x3': ops.F32X3}[dt]
    FDT = ops.BF16 if dt == 'bf16' else ops.F32                      # filter_prepare's type: F32X3 tensors are f32 tensors
    ldx = ops.pad_to(C, ops.chunk(FDT))
    Kp = ops.pad_to(K, kpad or (4 if dt == 'x3' else 8))
    d = ops.conv_desc(N, H, W, ldx, ldx, K, Kp, k, stride, dil, DT, DT)
    ran = {'fwd': set(), 'wgrad': set(), 'dgrad': set()}
    for arr in arrangements:
        # ---------------- forward + bias + ReLU
        for rnd in range(CE.rounds_fwd(case, arr)):
            E = CE.forward_case(case, arr, rnd, ldx, Kp)
            x = CE.Guarded(E['x'], dtype, dev, CE.GUARD_IN)
            w_c, _ = _filters(ops, E['w'], K, k, ldx, Kp, FDT, dtype, dev)
            b = CE.Guarded(E['b'], torch.float32, dev, CE.GUARD_IN)
            y = CE.Guarded(_prefilled(E['y'], K), dtype, dev, CE.GUARD_OUT)
            ops.conv2d_fwd(d, x.view, w_c.view, b.view, y.view, True)
            _sync(dev)
            ran['fwd'].add(ops.conv_last_kernel())
            _check(y, E['y'], E['shape_out'], f'forward {arr} round {rnd} {case} {dt}', ops)
            if rnd == 0 and dt != 'x3':                          # (the pool and sign-bit entry points refuse F32X3 descriptors)
                _pool_case(ops, d, case, E, x, w_c, b, dtype, dev, arr, forced)
                if arr == 'A' and dt == 'bf16':
                    _bits_case(ops, d, case, E, x, w_c, b, dev)
            # ---------------- filter + bias gradient: deterministic flush (the default) and float atomics, each called twice
            if 'dw' in E:
                dy = CE.Guarded(E['dy'], dtype, dev, CE.GUARD_IN)
                try:
                    for det in (1, 0):
                        ops.debug_set(5, det)
                        dw = CE.Guarded(torch.zeros_like(E['dw']), torch.float32, dev, CE.GUARD_OUT)
                        db = CE.Guarded(torch.zeros(K), torch.float32, dev, CE.GUARD_OUT)
                        for times in (1, 2):
                            ops.conv2d_wgrad(d, x.view, dy.view, Kp, dw.view, db.view)
                            _sync(dev)
                            what = f'filter gradient x{times} ({"deterministic" if det else "atomics"}) {case} {dt}'
                            ran['wgrad'].add(ops.conv_last_kernel())
                            _check(dw, times * E['dw'].reshape(K, -1), (1, 1, K), what + ' [index = (0, 0, k, (r s c))]', ops)
                            _check(db, times * E['db'].reshape(K, 1), (1, 1, K), what + ': bias gradient', ops)
                finally:
                    ops.debug_set(5, 1)
        # ---------------- input gradient: plain into 7.0, ReLU-masked + accumulated, wider dy pitch
        for rnd in range(CE.rounds_dgrad(case, arr)):
            D = CE.dgrad_case(case, arr, rnd, ldx, Kp)
            _, w_t = _filters(ops, D['w'], K, k, ldx, Kp, FDT, dtype, dev)
            dy = CE.Guarded(D['dy'], dtype, dev, CE.GUARD_IN)
            dx = CE.Guarded(torch.full_like(D['dx'], 7.0), dtype, dev, CE.GUARD_OUT)
            ops.conv2d_dgrad(d, dy.view, Kp, w_t.view, None, dx.view, False)
            _sync(dev)
            ran['dgrad'].add(ops.conv_last_kernel())
            _check(dx, D['dx'], D['shape_in'], f'input gradient {arr} round {rnd} {case} {dt}', ops)
            src = CE.Guarded(D['src'], dtype, dev, CE.GUARD_IN)
            dx2 = CE.Guarded(D['prev'], dtype, dev, CE.GUARD_OUT)
            ops.conv2d_dgrad(d, dy.view, Kp, w_t.view, src.view, dx2.view, True)
            _sync(dev)
            _check(dx2, D['dx2'], D['shape_in'], f'masked, accumulated input gradient {arr} round {rnd} {case} {dt}', ops)
            if arr == 'A' and rnd == 0:
                lddy = Kp + 8
                _, w_t2 = _filters(ops, D['w'], K, k, ldx, lddy, FDT, dtype, dev)
                wide = torch.zeros(D['dy'].shape[0], lddy, dtype=D['dy'].dtype)
                wide[:, :Kp] = D['dy']
                dyw = CE.Guarded(wide, dtype, dev, CE.GUARD_IN)
                dx3 = CE.Guarded(torch.full_like(D['dx'], 7.0), dtype, dev, CE.GUARD_OUT)
                ops.conv2d_dgrad(d, dyw.view, lddy, w_t2.view, None, dx3.view, False)
                _sync(dev)
                _check(dx3, D['dx'], D['shape_in'], f'input gradient, lddy = {lddy} > Kp = {Kp}, {case} {dt}', ops)
    return ran


def _pool_case(ops, d, case, E, x, w_c, b, dtype, dev, arr, forced):
    """odtk_conv2d_fwd_pool2x2: in one launch where the library says so (with and without the un-pooled output), else as conv + pool.  The pooled map equals the
    pool of the exact un-pooled map, and the recorded arg-max routes a gradient of ones to exactly one element per window whose exact value IS the maximum."""
    N, H, W, C, K, k, stride, dil = case
    fused = ops.conv2d_fwd_pool2x2_fused(d)
    Kp = E['y'].shape[1]
    kch = 8 if dtype == torch.bfloat16 else 4
    if K % kch or Kp % 8:          # what the entry points accept: one arg-max code per whole 16-byte chunk of channels, pooled pitch a multiple of 8
        return
    if forced and not fused:       # conv + pool as two launches under a forced engine: the convolution just checked, then the pool kernel the auto dispatch checks
        return
    if 'pool' not in E:
        E['pool'], E['pool_shape'] = CE.pool2x2_ref(E['y'], E['shape_out'], K)
    p_ref, pshape = E['pool'], E['pool_shape']
    n, Ho, Wo = E['shape_out']
    nchunk = p_ref.shape[0] * (Kp // kch)
    for keep in ((True, False) if fused else (True,)):
        y = CE.Guarded(_prefilled(E['y'], K), dtype, dev, CE.GUARD_OUT) if keep else None
        p = CE.Guarded(_prefilled(p_ref, K, -3.0), dtype, dev, CE.GUARD_OUT)
        idx = CE.Guarded(torch.zeros(nchunk), torch.int16, dev, -1)
        ops.conv2d_fwd_pool2x2(d, x.view, w_c.view, b.view, y.view if keep else None, True, p.view, idx.view)
        _sync(dev)
        kern = ops.conv_last_kernel()
        what = f'conv + 2x2 pool ({"one launch" if fused else "two launches"}, keep={keep}) {arr} {case}'
        _check(p, p_ref, pshape, what + ': pooled map', ops, kern)
        if keep:
            _check(y, E['y'], E['shape_out'], what + ': un-pooled map', ops, kern)
        assert idx.guards_intact(), what + ': wrote outside the arg-max record'
        # the recorded routing, whatever its encoding: a gradient of ones lands once per window and channel, on an element that holds the window's maximum
        ones = torch.zeros_like(p_ref)
        ones[:, :K] = 1
        g1 = CE.Guarded(ones, dtype, dev, CE.GUARD_IN)
        dxp = CE.Guarded(torch.full_like(E['y'], 5.0), dtype, dev, CE.GUARD_OUT)
        ops.maxpool2x2_bwd_idx(idx.view, g1.view, dxp.view, n, Ho, Wo, K, Kp, pshape[1], pshape[2])
        _sync(dev)
        assert dxp.guards_intact(), what + ': the routed gradient left its buffer'
        r = dxp.view.float().cpu()[:, :K].reshape(n, Ho, Wo, K)
        cnt, _ = CE.pool2x2_ref(CE.rows(r, Kp), E['shape_out'], K)               # max over each window of a 0 / 1 map ...
        assert float(r.sum()) == float(p_ref.shape[0] * K) and torch.equal(cnt[:, :K].float(), torch.ones(p_ref.shape[0], K)), what + ': not one routed element per window'
        yv = E['y'][:, :K].float().reshape(n, Ho, Wo, K)
        up = p_ref[:, :K].float().reshape(n, pshape[1], pshape[2], K).repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :Ho, :Wo]
        assert torch.equal(yv[r > 0], up[r > 0]), what + f' [{kern}]: the recorded arg-max points at an element that is not the maximum'


def _bits_case(ops, d1, case, E, x, w_c, b, dev):
    """odtk_conv2d_fwd_bits / odtk_conv2d_dgrad_bits where the library says the pair applies (a <= 8 -> 64 first layer in front of a 64 -> 64 3 x 3 layer)"""
    N, H, W, C, K, k, stride, dil = case
    if not (C <= 8 and K == 64 and k == 3 and stride == 1 and dil == 1):
        return
    d2 = ops.conv_desc(N, H, W, 64, 64, 64, 64, 3, 1, 1)
    if not ops.conv2d_relu_bits_supported(d1, d2, 64):
        return
    y = CE.Guarded(torch.full_like(E['y'], 3.0), torch.bfloat16, dev, CE.GUARD_OUT)
    want = ((E['y'].float() > 0).reshape(-1, 8).to(torch.int32) * (2 ** torch.arange(8, dtype=torch.int32))).sum(-1).to(torch.uint8)
    bits = CE.Guarded(torch.full_like(want, 255), torch.uint8, dev, 0x55)
    ops.conv2d_fwd_bits(d1, x.view, w_c.view, b.view, y.view, True, bits.view)
    _sync(dev)
    kern = ops.conv_last_kernel()
    _check(y, E['y'], E['shape_out'], f'forward with sign bits {case}', ops, kern)
    assert torch.equal(bits.view.cpu(), want) and bits.guards_intact(), f'sign bits {case} [{kern}]'
    case2 = (N, H, W, 64, 64, 3, 1, 1)
    D = CE.dgrad_case(case2, 'A', 0, 64, 64)
    _, w_t = _filters(ops, D['w'], 64, 3, 64, 64, ops.BF16, torch.bfloat16, dev)
    dy = CE.Guarded(D['dy'], torch.bfloat16, dev, CE.GUARD_IN)
    dx = CE.Guarded(torch.full_like(D['dx'], 5.0), torch.bfloat16, dev, CE.GUARD_OUT)
    ops.conv2d_dgrad_bits(d2, dy.view, 64, w_t.view, bits.view, dx.view, False)
    _sync(dev)
    _check(dx, D['dx'] * (E['y'] > 0), D['shape_in'], f'input gradient masked by sign bits {case2}', ops)


# ------------------------------------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("case", CONV_CASES + V3_EXTRA_CASES)
def test_exact_v3_engine(case, dev, v3_engine):
    exact_case(case, "bf16", dev, forced=True)


@pytest.mark.parametrize("case", CONV_CASES + V3_EXTRA_CASES)
def test_exact_legacy_engine(case, dev):
    ops = _ops()
    ops.debug_set(1, 1)
    try:
        exact_case(case, "bf16", dev, forced=True)
    finally:
        ops.debug_set(1, 0)


@pytest.mark.parametrize("case", V9_EXTRA_CASES + V3_EXTRA_CASES[:12])
def test_exact_v9_engine(case, dev, v9_engine):
    assert "" not in exact_case(case, "bf16", dev, forced=True)['fwd']


@pytest.mark.parametrize("off", [0, 16384], ids=["tiles128", "tiles128-off"])
@pytest.mark.parametrize("case", HALO128_CASES)
def test_exact_halo_kernel_on_128x128_tiles(case, off, dev):
    ops = _ops()
    ops.debug_set(6, off)
    try:
        exact_case(case, "bf16", dev, forced=True)
    finally:
        ops.debug_set(6, 0)


@pytest.mark.parametrize("case", SSD300_LAYER_CASES)
def test_exact_ssd300_layer_geometries(case, dev):
    exact_case(case, "bf16", dev)


@pytest.mark.parametrize("case", [(32,) + c[1:] for c in SSD300_LAYER_CASES])
def test_exact_ssd300_layer_geometries_batch32(case, dev):
    torch.set_num_threads(16)
    exact_case(case, "bf16", dev)


@pytest.mark.parametrize("case", CONV_CASES)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_exact_auto_dispatch(case, dt, dev):
    exact_case(case, dt, dev)


@pytest.mark.parametrize("case", BACKBONE_CASES)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_exact_backbone_geometries(case, dt, dev):
    exact_case(case, dt, dev)


def test_exact_filter_gradient_split_reduce_with_rsc_not_a_multiple_of_8(dev):
    """the fixed-order reduction of the filter-gradient partials moves 16-byte rows of K R S C floats: R S C = 9 x 28 = 252 (f32, two pixel splits)"""
    ran = exact_case((2, 32, 32, 28, 56, 3, 2, 1), "f32", dev, arrangements=('A',))
    # the generic kernel is the one that splits 16 slabs of 32 pixels in two (512 output pixels, 2 tiles) and reduces them in the deterministic mode
    assert all(n.startswith('conv_wgrad_kernel') for n in ran['wgrad']), ran


@pytest.mark.parametrize("case", X3_CASES)
def test_exact_x3_operand_splitting(case, dev):
    """F32X3 descriptors through the split path (odtk_debug_set(6, 8)): exact, hence equal to the plain f32 engine, which is held to the same reference"""
    ops = _ops()
    ops.debug_set(6, 8)
    try:
        ran = exact_case(case, "x3", dev)
        assert all('x3' in n for n in ran['fwd'] | ran['dgrad']), ran           # every arrangement and round
        ran = exact_case(case, "f32", dev, kpad=4)
        assert not any('x3' in n for n in ran['fwd'] | ran['dgrad']), ran
    finally:
        ops.debug_set(6, 0)
