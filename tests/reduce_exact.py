"""Cases and float64 references for the kernels of csrc/elementwise.hip / centernet_net.hip that reduce or select (plain module, no tests and no GPU imports; used by
tests/test_gpu_reduce_exact.py on the GPU and by tests/test_reduce_exact_cpu.py on the kernel source without one): max pooling (maxpool_fwd / _bwd -- the gather
kernel and its 2 x 2 specialisation --, maxpool_fwd_argmax / _bwd_argmax, maxpool2x2_fwd_idx / _bwd_idx), colsum, sgd_momentum, sum_f32, loss_total, and, bounded
against float64 instead of exact, l2norm_fwd / _bwd and adam.

Operands are chosen so that there is ONE right answer, bit for bit, wherever the kernel has no rsqrtf, sqrtf or division:
  max pooling     integers that are exact in bf16 ('random' in [-100, 100], 'ties' from {-1, -0.0, +0.0, 1}, 'constant', 'negative': all < 0), dy integers in [-8, 8]: at
                  most nine windows overlap a pixel, every sum is exact.  y and dx as raw bits, the 2-bit / 4-bit position codes decoded and compared with the
                  reference arg-max position.  Reference: float64 F.max_pool2d(return_indices=True) over the map padded with -inf, scatter-add of dy at its indices;
                  its tie rule -- the FIRST maximum in row-major window scan order, TF's MaxPoolGrad routing -- is pinned by a pure-Python loop (pool_reference_loop,
                  reference_tie_rule_is_pinned).  Every backward path gets the REFERENCE's y / codes as input and is compared with the reference, never with a kernel.
                  Non-finite activations through the pools are out of scope.
  colsum          integers in [-8, 8] (|partial sum| <= 40 000 < 2^24) against an int64 sum; the guarded workspace may only be written in whole rows of C partials
  sgd_momentum    integers in [-16, 16], lr 2^-3, momentum 0.5, wd 2^-4, grad_scale 1 or 0.5: every product and sum is representable, fused or not
  sum_f32 / loss_total   integers, power-of-two scales
The two bounded families, per element:  |got - ref64| <= |ref32 - ref64| + K ulp_f32(ref64)  (+ one bf16 ulp for a bf16 output), ref32 being the same expression
step by step in float32 (torch, CPU), K = 4 (K_ULP).  So that this holds for a CORRECT kernel the operands keep the expressions well conditioned -- that is a choice
of inputs, not of tolerance:
  l2norm   x in +-{8..16}/16, dy in +-{8..16}/8: sum x^2 and sum x dy are exact in f32 in any order (<= 18 bits), so rsqrtf and the products are all that rounds.  dx =
           g inv dy - k x cancels where the two terms meet (dx is orthogonal to x); the signs of dy are drawn until |k x| <= |g inv dy| / 4 everywhere, and the
           accumulated-onto dx has dy's sign.  Then |dx| >= 3/4 |g inv dy| and the kernel's roundings (rsqrtf 1 ulp, two products for the first term, five for the
           second at a quarter of the weight, one subtraction) stay below K ulp of dx.  One all-zero row (the clamp: y = 0, dx = g 1e6 dy, no second term) and one row
           with a single non-zero element, a power of two (there the two terms cancel EXACTLY: dx = 0 at that element), each once in the middle and once last.
           From four rows on, one row of 2^-25 x: its sum of squares is positive and below the clamp while sum x dy is not zero, which is where the clamp branch
           differs from the unclamped expression (tf.maximum passes no gradient to the sum of squares there: dx = g 1e6 dy, no second term).
           dgamma: |got - ref64| <= 8 eps_f32 (sum_m |sd_m inv_m| + |dgamma before|), a condition-number bound.
  adam     p, m, g integers in [-16, 16] (p = 0 included), v integers in [1, 16], lr_t 2^-10, wd 2^-4: g' = g gs + wd p and g'^2 are exact, v' >= 0.99, the update
           |u| <= 2^-6 never cancels against a non-zero p, and where p = 0 the result IS -u.  l2_partial is exact (p integers).
The two long l2norm cases (M = 4 101: second grid trip of the backward kernel, M = 16 389: of the forward kernel) run in both tiers.

Every operand -- inputs included -- lives in a conv_exact.Guarded allocation, pad columns of inputs hold GUARD_IN, outputs are pre-filled with a sentinel; after
every launch: guards intact, inputs unchanged, the WHOLE [M][ld] output == what was there before with the window replaced by the reference (pad columns of y / dx keep
what they held: include/odtk.h).  The runners take `ops` (odtk.ops or the CPU emulation of the kernel source installed over it) and the device; the bounded ones
return {family: largest K needed}."""
import torch
import torch.nn.functional as F

import conv_exact as CE
import glue_exact as GX
from glue_exact import FRESH, IN_PAD, PAD, Operand, _gen, _rnd, _sync, check_input, check_output, ints, kc, tdt  # noqa: F401

K_ULP = 4
EPS32 = 2.0 ** -24
case_id = GX.case_id


# ------------------------------------------------------------------------------------------------------------ flat operands
class Flat:
    """1-D operand: `off` sentinels, the n elements the launch sees, 8 sentinels -- between guard bands"""

    def __init__(self, window, off, dtype, dev, pad, guard):
        n = window.numel()
        self.n, self.off = n, off
        if not dtype.is_floating_point:
            pad, guard = int(pad), int(guard)
        self.before = torch.full((off + n + 8,), pad, dtype=dtype)
        self.before[off: off + n] = window if window.dtype == dtype else _rnd(window, dtype)
        self.G = CE.Guarded(self.before, dtype, dev, guard)
        self.t = self.G.view[off: off + n]

    def got(self):
        return self.G.view.cpu()

    def check(self, ref, what):
        """the whole buffer, raw bits: the window == ref, everything around it as before; guards intact"""
        exp = self.before.clone()
        exp[self.off: self.off + self.n] = ref
        got = self.got()
        if not torch.equal(_bits(got), _bits(exp)):
            bad = (_bits(got) != _bits(exp)).nonzero().flatten()
            first = [(int(i) - self.off, got[i].item(), exp[i].item()) for i in bad[:8]]
            raise AssertionError(f'{what}: {bad.numel()} of {exp.numel()} elements differ [raw bits]; first (index in the view, got, expected): {first}')
        assert self.G.guards_intact(), f'{what}: wrote outside its operand {self.G.first_guard_damage()}'

    def unchanged(self, what):
        self.check(self.before[self.off: self.off + self.n], what + ': an INPUT changed')


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def ulp32(r64):
    """spacing of f32 at |r| (the subnormal spacing at 0)"""
    r = r64.float().abs()
    return torch.nextafter(r, torch.full_like(r, float('inf'))).double() - r.double()


def k_needed(got, ref64, ref32, dtype):
    """per element: (|got - ref64| - |ref32 - ref64| - [one bf16 ulp]) / ulp_f32(ref64); the bound is K_ULP"""
    u = ulp32(ref64)
    excess = (got.double() - ref64).abs() - (ref32.double() - ref64).abs() - (u * 65536. if dtype == torch.bfloat16 else 0.)
    return excess / u


def check_bounded(got, ref64, ref32, dtype, what, tol_of_max):
    assert bool(torch.isfinite(got.double()).all()), what + ': non-finite output'
    need = k_needed(got, ref64, ref32, dtype)
    worst = float(need.max()) if need.numel() else 0.
    u = ulp32(ref64)
    bound = (ref32.double() - ref64).abs() + K_ULP * u + (u * 65536. if dtype == torch.bfloat16 else 0.)
    if need.numel() and float(ref64.abs().max()) > 0.:         # the bound stays inside what tests/test_gpu_kernels.py allows of the largest output
        assert float(bound.max()) <= tol_of_max * float(ref64.abs().max()), (what, float(bound.max()), float(ref64.abs().max()))
    if worst > K_ULP:
        i = int(need.reshape(-1).argmax())
        raise AssertionError(f'{what}: element {i}: got {float(got.reshape(-1)[i])!r}, float64 {float(ref64.reshape(-1)[i])!r}, float32 reference '
                             f'{float(ref32.reshape(-1)[i])!r}: needs K = {worst:.2f} > {K_ULP}')
    return max(worst, 0.)


def check_bounded_rows(o, ref64, ref32, what, tol_of_max):
    """output Operand `o`: pad columns and guards exactly, the window within the bound; returns the K needed"""
    got = o.G.view.reshape(o.before.shape).cpu()
    keep = o.before.clone()
    win = got[:, o.c0: o.c0 + o.C].clone()
    got[:, o.c0: o.c0 + o.C] = keep[:, o.c0: o.c0 + o.C]
    GX._fail(what + ' [pad columns, raw bits]', o.G, GX._ibits(got), GX._ibits(keep), None)
    return check_bounded(win, ref64, ref32, o.before.dtype, what, tol_of_max)


# ------------------------------------------------------------------------------------------------------------ max pooling
POOL_WINDOWS = [('k2s2', 2, 2, [(1, 1, 1), (2, 2, 2), (2, 5, 7), (3, 4, 9), (1, 1, 6), (1, 6, 1)]),
                ('k3s1', 3, 1, [(1, 1, 1), (2, 3, 3), (2, 5, 7), (1, 1, 5)]),
                ('k3s2', 3, 2, [(2, 5, 7), (2, 6, 6)]),                                   # pad-before 1 and 0
                ('k2s1', 2, 1, [(2, 4, 5)])]
POOL_CASES = [((name, k, s), geo, nch, lay) for name, k, s, geos in POOL_WINDOWS for geo in geos for nch in (1, 3) for lay in ('tight', 'pitched')]
POOL_REGIMES = ('random', 'ties', 'constant', 'negative')


def pool_input(regime, shape, g):
    if regime == 'random':
        return ints(shape, -100, 100, g)
    if regime == 'ties':
        return torch.tensor([-1., -0., 0., 1.], dtype=torch.float64)[torch.randint(0, 4, shape, generator=g)]
    if regime == 'constant':
        return torch.full(shape, -3., dtype=torch.float64)
    return ints(shape, -100, -1, g)


def pool_geometry(ops, H, W, k, s):
    Ho, pt, pb = ops.same_pad(H, k, s)
    Wo, pl, pr = ops.same_pad(W, k, s)
    return Ho, Wo, (pt, pb, pl, pr)


def pool_reference(xv, N, H, W, k, s, Ho, Wo, pads):
    """rows [N H W][C] float64 -> (y rows [N Ho Wo][C], window position r * k + s of the maximum, input row it sits in); torch on the CPU in float64 over the map
    padded with -inf the way oracle/ssd300_ref.maxpool_same pads"""
    pt, pb, pl, pr = pads
    C = xv.shape[1]
    xp = F.pad(xv.reshape(N, H, W, C).permute(0, 3, 1, 2), (pl, pr, pt, pb), value=float('-inf'))
    y, ind = F.max_pool2d(xp, k, s, return_indices=True)
    assert y.shape[2:] == (Ho, Wo)
    Wp = W + pl + pr
    hp, wp = ind // Wp, ind % Wp
    ho, wo = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Wo).view(1, 1, 1, Wo)
    pos = (hp - ho * s) * k + (wp - wo * s)
    src = (torch.arange(N).view(N, 1, 1, 1) * H + (hp - pt)) * W + (wp - pl)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(N * Ho * Wo, C)      # noqa: E731
    return rows(y), rows(pos), rows(src)


def pool_reference_loop(xv, N, H, W, k, s, Ho, Wo, pads):
    """the same in plain Python: the FIRST maximum in row-major window scan order keeps the window (strict >), cells outside the map never win"""
    pt, _, pl, _ = pads
    C = xv.shape[1]
    y, pos, src = torch.zeros(N * Ho * Wo, C, dtype=torch.float64), torch.zeros(N * Ho * Wo, C, dtype=torch.int64), torch.zeros(N * Ho * Wo, C, dtype=torch.int64)
    for n in range(N):
        for ho in range(Ho):
            for wo in range(Wo):
                for c in range(C):
                    best = None
                    for r in range(k):
                        for q in range(k):
                            h, w = ho * s - pt + r, wo * s - pl + q
                            if 0 <= h < H and 0 <= w < W and (best is None or float(xv[(n * H + h) * W + w, c]) > float(best[0])):
                                best = (xv[(n * H + h) * W + w, c], r * k + q, (n * H + h) * W + w)
                    o = (n * Ho + ho) * Wo + wo
                    y[o, c], pos[o, c], src[o, c] = best
    return y, pos, src


def reference_tie_rule_is_pinned(ops):
    """torch's arg-max (the reference of every pooling case) == the loop above on inputs that are nothing but ties; both windows that overlap and that do not"""
    for (k, s, (N, H, W)) in [(3, 1, (2, 3, 3)), (2, 2, (2, 5, 7)), (3, 2, (2, 5, 7))]:
        Ho, Wo, pads = pool_geometry(ops, H, W, k, s)
        for regime in ('ties', 'constant'):
            xv = pool_input(regime, (N * H * W, 4), _gen('pin', k, s, regime))
            a, b = pool_reference(xv, N, H, W, k, s, Ho, Wo, pads), pool_reference_loop(xv, N, H, W, k, s, Ho, Wo, pads)
            assert torch.equal(a[0].float().view(torch.int32), b[0].float().view(torch.int32)), (k, s, regime, 'y (raw bits)')
            assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (k, s, regime, 'arg-max')


def _pack_codes(pos, k_c, bits, dtype):
    """[rows][C] positions -> one word per 16-byte chunk, `bits` per channel, channel e of the chunk at bit e * bits"""
    rows, C = pos.shape
    v = (pos.reshape(rows, C // k_c, k_c) << (torch.arange(k_c) * bits)).sum(-1).reshape(-1)
    top = 1 << (8 * {torch.int32: 4, torch.int16: 2}[dtype])
    return torch.where(v >= top // 2, v - top, v).to(dtype)


def _check_codes(o, pos, k_c, bits, what):
    got = o.got()[o.off: o.off + o.n].to(torch.int64)
    dec = (got.view(-1, 1) >> (torch.arange(k_c) * bits)) & ((1 << bits) - 1)
    want = pos.reshape(-1, k_c)
    if not torch.equal(dec, want):
        bad = (dec != want).nonzero()
        first = [((int(r), int(e)), int(dec[r, e]), int(want[r, e])) for r, e in bad[:8]]
        raise AssertionError(f'{what}: {bad.shape[0]} position codes differ; first ((chunk, channel in it), got, reference arg-max position): {first}')
    o.check(_pack_codes(pos, k_c, bits, o.before.dtype), what + ' [code words]')


def run_pool(ops, dev, case, dt):
    (name, k, s), (N, H, W), nch, layout = case
    dtype, k_c = tdt(dt), kc(dt)
    C = nch * k_c
    ld = C if layout == 'tight' else C + 2 * k_c
    Ho, Wo, pads = pool_geometry(ops, H, W, k, s)
    pt, _, pl, _ = pads
    Mi, Mo = N * H * W, N * Ho * Wo
    for regime in POOL_REGIMES:
        g = _gen('pool', case, dt, regime)
        what = f'{name} N,H,W={N},{H},{W} C={C} ld={ld} {regime} {dt}'
        xv = pool_input(regime, (Mi, C), g)
        dyv = ints((Mo, C), -8, 8, g)
        y_ref, pos, src = pool_reference(xv, N, H, W, k, s, Ho, Wo, pads)
        dx_ref = torch.zeros(Mi, C, dtype=torch.float64)
        dx_ref.index_put_((src.reshape(-1), torch.arange(C).repeat(Mo)), dyv.reshape(-1), accumulate=True)
        y_ref, dx_ref = _rnd(y_ref, dtype), _rnd(dx_ref, dtype)
        x = Operand(xv, ld, dtype, dev, IN_PAD, CE.GUARD_IN)
        dy = Operand(dyv, ld, dtype, dev, IN_PAD, CE.GUARD_IN)
        yin = Operand(y_ref, ld, dtype, dev, IN_PAD, CE.GUARD_IN)                       # the reference's y: what the gather kernel is handed
        fresh_y = lambda: Operand(torch.full((Mo, C), FRESH, dtype=dtype), ld, dtype, dev, PAD, CE.GUARD_OUT)      # noqa: E731
        fresh_dx = lambda: Operand(torch.full((Mi, C), FRESH, dtype=dtype), ld, dtype, dev, PAD, CE.GUARD_OUT)     # noqa: E731

        def inputs_unchanged(w, *more):
            for o in (x, dy, yin):
                check_input(o, w)
            for o in more:
                o.unchanged(w)

        y = fresh_y()
        ops.maxpool_fwd(x.t, y.t, N, H, W, C, ld, Ho, Wo, k, s, pt, pl)
        _sync(dev)
        check_output(y, y_ref, 'maxpool_fwd ' + what, bits=True, shape=(N, Ho, Wo))
        inputs_unchanged('maxpool_fwd ' + what)
        dx = fresh_dx()
        ops.maxpool_bwd(x.t, yin.t, dy.t, dx.t, N, H, W, C, ld, Ho, Wo, k, s, pt, pl)         # k2s2: the 2 x 2 specialisation, else the gather kernel
        _sync(dev)
        check_output(dx, dx_ref, 'maxpool_bwd ' + what, bits=True, shape=(N, H, W))
        inputs_unchanged('maxpool_bwd ' + what)
        # recorded arg-max, 4 bits per channel in a 32-bit word per chunk
        y = fresh_y()
        arg = Flat(torch.full((Mo * nch,), 0x5a5a, dtype=torch.int32), 1, torch.int32, dev, PAD, CE.GUARD_OUT)
        ops.maxpool_fwd_argmax(x.t, y.t, arg.t, N, H, W, C, ld, Ho, Wo, k, s, pt, pl)
        _sync(dev)
        check_output(y, y_ref, 'maxpool_fwd_argmax ' + what, bits=True, shape=(N, Ho, Wo))
        _check_codes(arg, pos, k_c, 4, 'maxpool_fwd_argmax ' + what)
        inputs_unchanged('maxpool_fwd_argmax ' + what)
        argin = Flat(_pack_codes(pos, k_c, 4, torch.int32), 1, torch.int32, dev, IN_PAD, CE.GUARD_IN)
        dx = fresh_dx()
        ops.maxpool_bwd_argmax(argin.t, dy.t, dx.t, N, H, W, C, ld, Ho, Wo, k, s, pt, pl)
        _sync(dev)
        check_output(dx, dx_ref, 'maxpool_bwd_argmax ' + what, bits=True, shape=(N, H, W))
        inputs_unchanged('maxpool_bwd_argmax ' + what, argin)
        if name != 'k2s2':
            continue
        # 2 x 2 / stride 2: 2 bits per channel (t = 2 dr + dc) in a 16-bit word per chunk
        y = fresh_y()
        idx = Flat(torch.full((Mo * nch,), 0x5a5a, dtype=torch.int16), 1, torch.int16, dev, PAD, CE.GUARD_OUT)
        ops.maxpool2x2_fwd_idx(x.t, y.t, idx.t, N, H, W, C, ld, Ho, Wo)
        _sync(dev)
        check_output(y, y_ref, 'maxpool2x2_fwd_idx ' + what, bits=True, shape=(N, Ho, Wo))
        _check_codes(idx, pos, k_c, 2, 'maxpool2x2_fwd_idx ' + what)
        inputs_unchanged('maxpool2x2_fwd_idx ' + what)
        idxin = Flat(_pack_codes(pos, k_c, 2, torch.int16), 1, torch.int16, dev, IN_PAD, CE.GUARD_IN)
        dx = fresh_dx()
        ops.maxpool2x2_bwd_idx(idxin.t, dy.t, dx.t, N, H, W, C, ld, Ho, Wo)
        _sync(dev)
        check_output(dx, dx_ref, 'maxpool2x2_bwd_idx ' + what, bits=True, shape=(N, H, W))
        inputs_unchanged('maxpool2x2_bwd_idx ' + what, idxin)


# ------------------------------------------------------------------------------------------------------------ colsum
COLSUM_CASES = [(M, C) for M in (1, 31, 33, 129, 5000) for C in (3, 8, 40, 100, 264)]
WS_FRESH = -8192.5                  # no sum of integers: what the workspace holds where nothing was written


def run_colsum(ops, dev, case, dt):
    M, C = case
    dtype = tdt(dt)
    ld = CE.pad_to(C, kc(dt))
    g = _gen('colsum', case, dt)
    xv, prev = ints((M, C), -8, 8, g), ints((C,), -50, 50, g)
    total = xv.to(torch.int64).sum(0).double()
    x = Operand(xv, ld, dtype, dev, IN_PAD, CE.GUARD_IN)
    nws = ops.bn_workspace_bytes(M, C) // 4
    for acc in (False, True):
        what = f'colsum M={M} C={C} ld={ld} accumulate={acc} {dt}'
        out = Flat(prev, 1, torch.float32, dev, PAD, CE.GUARD_OUT)
        ws = Flat(torch.full((nws,), WS_FRESH), 0, torch.float32, dev, WS_FRESH, CE.GUARD_OUT)
        ops.colsum(x.t, M, C, ld, out.t, acc, ws.t)
        _sync(dev)
        out.check(_rnd(total + (prev if acc else 0.), torch.float32), what)
        check_input(x, what)
        # the workspace: partials in whole rows of C floats from its start, nothing else, nothing outside
        w = ws.got()
        written = (w != WS_FRESH).nonzero().flatten()
        last = int(written.max()) + 1 if written.numel() else 0
        assert last % C == 0 and last >= C and last <= nws, f'{what}: the workspace was written up to float {last}, which is not a whole number of rows of C = {C} partials'
        assert ws.G.guards_intact(), f'{what}: wrote outside its workspace {ws.G.first_guard_damage()}'


# ------------------------------------------------------------------------------------------------------------ the optimisers
OPT_NS = [1, 2, 3, 4, 5, 8191, 8192, 8193, 16387]
OPT_VARIANTS = [(l2, cast, gs) for l2 in (True, False) for cast in (None, 'f32', 'bf16') for gs in (1.0, 0.5)]


def _opt_buffers(ops, dev, n, l2, cast, pv):
    nb = ops.sgd_blocks(n)
    part = Flat(torch.full((nb,), FRESH), 1, torch.float32, dev, PAD, CE.GUARD_OUT) if l2 else None
    pc = None if cast is None else Flat(torch.full((n,), FRESH, dtype=tdt(cast)), 0, tdt(cast), dev, PAD, CE.GUARD_OUT)
    blocks = torch.arange(n) // (256 * 4 * 8)
    l2_ref = torch.zeros(nb, dtype=torch.float64).index_add_(0, blocks, pv * pv) * 0.5
    assert nb == int(blocks.max()) + 1 and float(l2_ref.max()) <= 2. ** 21
    return nb, part, pc, l2_ref


def _check_l2(ops, dev, part, l2_ref, what):
    """the per-block sums, exact; then odtk_sum_f32 over them, exact too"""
    part.check(_rnd(l2_ref, torch.float32), what + ' l2_partial')
    tot = Flat(torch.full((1,), FRESH), 1, torch.float32, dev, PAD, CE.GUARD_OUT)
    ops.sum_f32(part.t, tot.t)
    _sync(dev)
    tot.check(_rnd(l2_ref.sum().reshape(1), torch.float32), what + ' sum_f32(l2_partial)')
    part.check(_rnd(l2_ref, torch.float32), what + ' sum_f32(l2_partial): an INPUT changed')


def run_sgd(ops, dev, n, dt=None):
    lr, mom, wd = 2. ** -3, 0.5, 2. ** -4
    for l2, cast, gs in OPT_VARIANTS:
        g = _gen('sgd', n, l2, cast, gs)
        what = f'sgd_momentum n={n} l2_partial={l2} cast={cast} grad_scale={gs}'
        pv, mv, gv = ints((n,), -16, 16, g), ints((n,), -16, 16, g), ints((n,), -16, 16, g)
        m_ref = mom * mv + (gv * gs + wd * pv)
        p_ref = pv - lr * m_ref
        p = Flat(pv, 0, torch.float32, dev, PAD, CE.GUARD_OUT)
        m = Flat(mv, 0, torch.float32, dev, PAD, CE.GUARD_OUT)
        gr = Flat(gv, 0, torch.float32, dev, IN_PAD, CE.GUARD_IN)
        nb, part, pc, l2_ref = _opt_buffers(ops, dev, n, l2, cast, pv)
        ops.sgd_momentum(p.t, m.t, gr.t, lr, mom, wd, gs, part.t if l2 else None, pc.t if pc else None)
        _sync(dev)
        p.check(_rnd(p_ref, torch.float32), what + ' p')                     # (_rnd asserts that float64 -> f32 loses nothing)
        m.check(_rnd(m_ref, torch.float32), what + ' m')
        gr.unchanged(what)
        if pc:
            pc.check(_rnd(p_ref, tdt(cast), exact=False), what + ' cast copy (round to nearest even of the exact value)')
        if l2:
            _check_l2(ops, dev, part, l2_ref, what)


def run_adam(ops, dev, n, dt=None):
    """tf.train.AdamOptimizer as csrc/centernet_net.hip quotes ApplyAdam: g' = g gs + wd p; m += (g' - m)(1 - b1); v += (g' g' - v)(1 - b2);
    p -= (m lr_t) / (sqrt(v) + eps), with the f32 values of the parameters the kernel is handed"""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))      # noqa: E731
    lr_t, b1, b2, eps, wd = 2. ** -10, f32(0.9), f32(0.999), f32(1e-8), 2. ** -4
    worst = {}
    for l2, cast, gs in OPT_VARIANTS:
        g = _gen('adam', n, l2, cast, gs)
        what = f'adam n={n} l2_partial={l2} cast={cast} grad_scale={gs}'
        pv, mv, vv, gv = ints((n,), -16, 16, g), ints((n,), -16, 16, g), ints((n,), 1, 16, g), ints((n,), -16, 16, g)
        pv[::3] = 0.                                                            # where p = 0 the result is the update itself
        ge = gv * gs + wd * pv
        m64 = mv + (ge - mv) * (1. - b1)
        v64 = vv + (ge * ge - vv) * (1. - b2)
        p64 = pv - (m64 * lr_t) / (torch.sqrt(v64) + eps)
        t = lambda v: torch.tensor(v, dtype=torch.float32)            # noqa: E731
        pf, mf, vf, gf = pv.float(), mv.float(), vv.float(), gv.float()
        ge32 = gf * t(gs) + t(wd) * pf
        m32 = mf + (ge32 - mf) * (t(1.) - t(b1))
        v32 = vf + (ge32 * ge32 - vf) * (t(1.) - t(b2))
        p32 = pf - (m32 * t(lr_t)) / (torch.sqrt(v32) + t(eps))
        assert torch.equal(ge32.double(), ge) and torch.equal((ge32 * ge32).double(), ge * ge)
        p = Flat(pv, 0, torch.float32, dev, PAD, CE.GUARD_OUT)
        m = Flat(mv, 0, torch.float32, dev, PAD, CE.GUARD_OUT)
        v = Flat(vv, 0, torch.float32, dev, PAD, CE.GUARD_OUT)
        gr = Flat(gv, 0, torch.float32, dev, IN_PAD, CE.GUARD_IN)
        nb, part, pc, l2_ref = _opt_buffers(ops, dev, n, l2, cast, pv)
        ops.adam(p.t, m.t, v.t, gr.t, lr_t, b1, b2, eps, wd, gs, part.t if l2 else None, pc.t if pc else None)
        _sync(dev)
        for o, r64, r32, nm in ((p, p64, p32, 'p'), (m, m64, m32, 'm'), (v, v64, v32, 'v')) + (((pc, p64, p32, 'cast copy'),) if pc else ()):
            got = o.got()
            worst[nm] = max(worst.get(nm, 0.), check_bounded(got[:n], r64, r32, got.dtype, f'{what} {nm}', 1.0))
            o.check(got[:n], f'{what} {nm}: past its n elements')              # the sentinels behind element n - 1 and the guards
        gr.unchanged(what)
        if l2:
            _check_l2(ops, dev, part, l2_ref, what)
    return {'adam ' + k: v for k, v in worst.items()}


# ------------------------------------------------------------------------------------------------------------ sum_f32 / loss_total
SUM_NS = [0, 1, 63, 64, 65, 1023, 1024, 1025]


def run_sums(ops, dev, n, dt=None):
    g = _gen('sums', n)
    bv = ints((n,), -100, 100, g)
    b = Flat(bv, 1, torch.float32, dev, IN_PAD, CE.GUARD_IN)
    bp = b.G.view[1:]                                                            # (an empty view has no address: the pointer is taken from a longer one)
    out = Flat(torch.full((1,), FRESH), 1, torch.float32, dev, PAD, CE.GUARD_OUT)
    if n:
        ops.sum_f32(b.t, out.t)
    else:
        ops.call('odtk_sum_f32', ops._p(bp), 0, ops._p(out.t), ops._stream())
    _sync(dev)
    out.check(_rnd(bv.sum().reshape(1), torch.float32), f'sum_f32 n={n}')
    b.unchanged(f'sum_f32 n={n}')
    sa_, sb_ = 2. ** -2, 2. ** 3
    for stride in (1, 3):
        for na in (0, 1, 5, 1030):
            av = ints((na,), -100, 100, g)
            spread = torch.full((max(na * stride, 1),), IN_PAD, dtype=torch.float64)
            spread[: na * stride: stride] = av
            a = Flat(spread, 1, torch.float32, dev, IN_PAD, CE.GUARD_IN)
            for sums in (True, False):
                what = f'loss_total nb={n} na={na} stride_a={stride} sums={sums}'
                o = [Flat(torch.full((1,), FRESH), 1, torch.float32, dev, PAD, CE.GUARD_OUT) for _ in range(3)]
                sa, sb = (o[0].t, o[1].t) if sums else (None, None)
                if n:
                    ops.loss_total(a.t, na, stride, b.t, sa_, sb_, sa, sb, o[2].t)
                else:
                    ops.call('odtk_loss_total', ops._p(a.t), na, stride, ops._p(bp), 0, sa_, sb_, ops._p(sa), ops._p(sb), ops._p(o[2].t), ops._stream())
                _sync(dev)
                ta, tb = av.sum().reshape(1), bv.sum().reshape(1)
                o[0].check(_rnd(ta, torch.float32) if sums else o[0].before[1:2], what + ' sum_a')
                o[1].check(_rnd(tb, torch.float32) if sums else o[1].before[1:2], what + ' sum_b')
                o[2].check(_rnd(sa_ * ta + sb_ * tb, torch.float32), what + ' total')
                a.unchanged(what)
                b.unchanged(what)


# ------------------------------------------------------------------------------------------------------------ L2 normalise
L2_CASES = ([(M, C, lay, 'both') for M in (1, 3, 4, 5) for C in ('k', 40, 520) for lay in ('tight', 'pitched')]
            + [(4101, 'k', 'pitched', 'bwd'), (16389, 'k', 'pitched', 'fwd')])
L2_PLACEMENTS = ('middle', 'zero_last', 'single_last')
CLAMP = float(torch.tensor(1e-12, dtype=torch.float32))
GAMMA = 20.0


def l2_operands(M, C, placement, g):
    """x in +-{8..16}/16, dy in +-{8..16}/8, drawn until, row by row, |x_e| |sd| / ss <= |dy_e| / 4 and sd != 0; then the two special rows.  Returns float64
    (x, dy, prev with dy's sign, relu source)"""
    def draw(rows):
        sg = lambda: torch.randint(0, 2, (rows, C), generator=g).double() * 2 - 1          # noqa: E731
        return ints((rows, C), 8, 16, g) / 16. * sg(), ints((rows, C), 8, 16, g) / 8. * sg()
    x, dy = draw(M)
    for _ in range(2000):
        sd, ss = (x * dy).sum(1), (x * x).sum(1)
        bad = ((x.abs() / dy.abs()).max(1).values * sd.abs() / ss > 0.25) | (sd == 0)
        if not bool(bad.any()):
            break
        x[bad], dy[bad] = draw(int(bad.sum()))
    assert not bool(bad.any()), 'no well-conditioned draw'
    zero_row = single_row = None
    if placement == 'middle' and M >= 3:
        zero_row, single_row = 0, 1
    elif placement == 'zero_last':
        zero_row, single_row = M - 1, (0 if M >= 2 else None)
    elif placement == 'single_last':
        single_row, zero_row = M - 1, (0 if M >= 2 else None)
    if zero_row is not None:
        x[zero_row] = 0.
    if single_row is not None:
        x[single_row] = 0.
        x[single_row, C // 2] = -2.
    if M >= 4:                                      # row 2, never one of the two above: 0 < ss <= C 2^-50 < 1e-12, clamped with a NON-zero sum x dy
        x[2] *= 2. ** -25
    prev = ints((M, C), 8, 16, g) / 8. * torch.sign(dy)
    relu = torch.tensor([-1., -0., 0., 1., 2.], dtype=torch.float64)[torch.randint(0, 5, (M, C), generator=g)]
    return x, dy, prev, relu


def l2_reference(x, dy, prev, relu, gamma, dt64):
    """float64 (dt64 = torch.float64) or the same expression step by step in float32"""
    x, dy, gm = x.to(dt64), dy.to(dt64), torch.tensor(gamma, dtype=dt64)
    ss, sd = (x * x).sum(1, keepdim=True), (x * dy).sum(1, keepdim=True)
    clamped = ~(ss > CLAMP)
    inv = torch.rsqrt(torch.clamp(ss, min=CLAMP)) if dt64 == torch.float32 else 1. / torch.sqrt(torch.clamp(ss, min=CLAMP))
    y = x * inv * gm
    k = torch.where(clamped, torch.zeros((), dtype=dt64), gm * inv * inv * inv * sd)
    dx = gm * inv * dy - k * x
    if prev is not None:
        dx = dx + prev.to(dt64)
    if relu is not None:
        dx = torch.where(relu.to(dt64) > 0, dx, torch.zeros((), dtype=dt64))
    return y, dx, sd * inv


def run_l2norm(ops, dev, case, dt):
    M, C, layout, which = case
    dtype, k_c = tdt(dt), kc(dt)
    C = k_c if C == 'k' else C
    ld = C if layout == 'tight' else C + 2 * k_c
    tol = 1e-5 if dt == 'f32' else 1e-2
    worst = {'l2norm_fwd y': 0., 'l2norm_bwd dx': 0., 'l2norm_bwd dgamma (of its bound)': 0.}
    gm = Flat(torch.tensor([GAMMA], dtype=torch.float64), 1, torch.float32, dev, IN_PAD, CE.GUARD_IN)
    for placement in (L2_PLACEMENTS if which == 'both' else ('middle',)):
        g = _gen('l2', case, dt, placement)
        xv, dyv, prevv, reluv = l2_operands(M, C, placement, g)
        what = f'M={M} C={C} ld={ld} {placement} {dt}'
        x = Operand(xv, ld, dtype, dev, IN_PAD, CE.GUARD_IN)
        if which != 'bwd':
            y = Operand(torch.full((M, C), FRESH, dtype=dtype), ld, dtype, dev, PAD, CE.GUARD_OUT)
            ops.l2norm_fwd(x.t, y.t, M, C, ld, gm.t)
            _sync(dev)
            y64, y32 = l2_reference(xv, dyv, None, None, GAMMA, torch.float64)[0], l2_reference(xv, dyv, None, None, GAMMA, torch.float32)[0]
            worst['l2norm_fwd y'] = max(worst['l2norm_fwd y'], check_bounded_rows(y, y64, y32, 'l2norm_fwd ' + what, tol))
            check_input(x, 'l2norm_fwd ' + what)
            gm.unchanged('l2norm_fwd ' + what)
        if which == 'fwd':
            continue
        dy = Operand(dyv, ld, dtype, dev, IN_PAD, CE.GUARD_IN)
        rl = Operand(reluv, ld, dtype, dev, IN_PAD, CE.GUARD_IN)
        # odtk_debug_set key 5: 1 = block sums added in block order (the default), 0 = float atomics; the long case (its point is the second grid trip) takes one
        # variant of each mode, the small ones all eight
        variants = [(1, True, True), (0, False, False)] if which == 'bwd' else [(md, a, r) for md in (1, 0) for a in (False, True) for r in (False, True)]
        for mode, acc, relu in variants:
            w = f'l2norm_bwd {"deterministic" if mode else "atomic"} accumulate={acc} relu_src={relu} ' + what
            _, dx64, dg64 = l2_reference(xv, dyv, prevv if acc else None, reluv if relu else None, GAMMA, torch.float64)
            _, dx32, _ = l2_reference(xv, dyv, prevv if acc else None, reluv if relu else None, GAMMA, torch.float32)
            dg_bound = 8. * EPS32 * (float(dg64.abs().sum()) + 0.5)
            runs = []
            for _ in range(2 if mode else 1):
                dx = Operand(prevv if acc else torch.full((M, C), FRESH, dtype=dtype), ld, dtype, dev, PAD, CE.GUARD_OUT)
                dg = Flat(torch.tensor([0.5]), 1, torch.float32, dev, PAD, CE.GUARD_OUT)
                ops.debug_set(5, mode)
                try:
                    ops.l2norm_bwd(x.t, dy.t, dx.t, M, C, ld, gm.t, dg.t, acc, rl.t if relu else None)
                    _sync(dev)
                finally:
                    ops.debug_set(5, 1)
                worst['l2norm_bwd dx'] = max(worst['l2norm_bwd dx'], check_bounded_rows(dx, dx64, dx32, w, tol))
                got = dg.got()
                dg.check(got[1:2], w + ' dgamma: around the scalar')
                err = abs(float(got[1]) - (0.5 + float(dg64.sum())))
                assert err <= dg_bound, f'{w}: dgamma {float(got[1])!r}, float64 {0.5 + float(dg64.sum())!r}: off by {err:.3e} > 8 eps sum|sd inv| = {dg_bound:.3e}'
                worst['l2norm_bwd dgamma (of its bound)'] = max(worst['l2norm_bwd dgamma (of its bound)'], err / dg_bound)
                for o in (x, dy, rl):
                    check_input(o, w)
                gm.unchanged(w)
                runs.append((_bits(got).clone(), GX._ibits(dx.G.view.cpu()).clone()))
            if mode:
                assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), w + ': two deterministic runs differ'
    return worst
