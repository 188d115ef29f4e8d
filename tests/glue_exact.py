"""Cases and float64 references for the data-moving kernels between the layers (plain module, no tests and no GPU imports; used by tests/test_gpu_glue_exact.py on
the GPU and by tests/test_glue_exact_cpu.py without one): add2d, copy_channels, add_relu_fwd / relu_bwd, upsample2x_*, avgpool2x2_*, rows_to_f32 / rows_from_f32,
exp_rows_*, cast_from_f32 / cast_to_f32, preprocess_norm.

These kernels do a copy, an add, a max, a mean of four or one rounding, so for well-chosen inputs there is ONE right answer, bit for bit:
  copies                      arbitrary finite bit patterns, +-0, subnormals, +-inf; compared as raw bits
  sums (up to 5 terms)        integers in [-25, 25]: every partial sum |s| <= 128 is exact in bf16 (and f32)
  avgpool2x2_fwd / _bwd       integers in [-32, 32] / [-64, 64]: sum <= 128, / 4 leaves 2 fractional bits -> 7 significant bits
  ReLU                        compared by value (fmaxf(-0.f, 0.f) may return either zero); y of relu_bwd holds +0.0 and -0.0, the gradient there is 0
  exp_rows_bwd                one f32 multiply, one rounding: (dy * y).to(dtype)
  preprocess_norm             the f32 expression (img / div - mean) / std, bit for bit
  exp_rows_to_f32             the only inexact one: float64 exp of the loaded value; bound = what torch.exp in f32 on the same device loses against it + 1 ulp
The reference is the plain expression in float64 on the CPU, rounded once to the output dtype (`_rnd` asserts that float64 -> f32 loses nothing, so that
torch's float64 -> f32 -> bf16 is one rounding; torch.Tensor.to(torch.bfloat16) is round-to-nearest-even, the rule of f32_to_bf16 in csrc/common.h).

Every operand -- inputs included -- lives in a conv_exact.Guarded allocation: guard rows in front of and behind it, sentinels in its pad columns.  A case compares
the WHOLE [M][ld] output with `what was there before, with the [:, :C] window replaced by the reference` (pad columns zero instead where the contract of
include/odtk.h says the kernel zeroes them), demands untouched guards on every operand and unchanged inputs.

The runners take `ops` (odtk.ops: the real launches, the CPU emulation of the kernel source or tests/mock_ops.py installed over it) and the device."""
import zlib

import torch

import conv_exact as CE
from oracle.centernet_net_ref import MEAN, STD              # CenterNet.py:51-65's constants, as tests/test_gpu_centernet_model.py uses them

PAD = CE.GUARD_OUT            # pad columns / not-yet-written elements of an output
IN_PAD = CE.GUARD_IN          # pad columns of an input: read by mistake, an error of >= 16384
FRESH = 7.0                   # the [:, :C] window of an output that is overwritten
T = 256                       # threads per workgroup of every launch here


def tdt(dt):
    return torch.float32 if dt == 'f32' else torch.bfloat16


def kc(dt):
    """elements per 16-byte chunk"""
    return 4 if dt == 'f32' else 8


def case_id(case):
    return '-'.join('x'.join(str(v) for v in c) if isinstance(c, tuple) else str(c) for c in case) if isinstance(case, tuple) else str(case)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _sync(dev):
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()


def _ibits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _rnd(v64, dtype, exact=True):
    """float64 -> output dtype in one rounding; exact: the case promises a representable result, so assert it"""
    f = v64.to(torch.float32)
    assert torch.equal(f.double(), v64), 'reference not representable in f32: float64 -> f32 -> bf16 would round twice'
    r = f.to(dtype)
    if exact:
        assert torch.equal(r.double(), v64), 'case is not exact in ' + str(dtype)
    return r


def ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


_SPECIAL_BITS = {torch.float32: [0, -2 ** 31, 1, 0x007fffff, -2 ** 31 + 1, 0x7f800000, 0xff800000 - 2 ** 32, 0x00800000, 0x7f7fffff],
                 torch.bfloat16: [0, -2 ** 15, 1, 0x007f, -2 ** 15 + 1, 0x7f80, 0xff80 - 2 ** 16, 0x0080, 0x7f7f]}


def bit_patterns(shape, dtype, g):
    """arbitrary bit patterns that are not NaN; the first elements are +0, -0, the smallest / largest / a negative subnormal, +-inf, the smallest and the largest
    normal number"""
    if dtype == torch.float32:
        b = torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, dtype=torch.int64)
        nan = ((b & 0x7f800000) == 0x7f800000) & ((b & 0x007fffff) != 0)
        b = torch.where(nan, b & ~0x007fffff, b).to(torch.int32)
    else:
        b = torch.randint(-2 ** 15, 2 ** 15, shape, generator=g, dtype=torch.int64)
        nan = ((b & 0x7f80) == 0x7f80) & ((b & 0x007f) != 0)
        b = torch.where(nan, b & ~0x007f, b).to(torch.int16)
    sp = torch.tensor(_SPECIAL_BITS[dtype], dtype=b.dtype)
    flat = b.reshape(-1)
    k = min(flat.numel(), sp.numel())
    flat[:k] = sp[:k]
    t = flat.reshape(shape).view(dtype)
    assert not bool(torch.isnan(t).any())
    return t


class Operand:
    """[M][ld] rows between guard rows on `dev`; the launch sees the column window [c0, c0 + C) (c0 > 0: a channel slice of a wider concat buffer).  `inner`
    ([M][C], already of `dtype`, or a float64 tensor of exactly representable values) fills the window, `pad` every other column."""

    def __init__(self, inner, ld, dtype, dev, pad, guard, c0=0):
        M, C = inner.shape
        assert c0 + C <= ld
        self.C, self.ld, self.c0 = C, ld, c0
        self.before = torch.full((M, ld), pad, dtype=dtype)
        self.before[:, c0: c0 + C] = inner if inner.dtype == dtype else _rnd(inner, dtype)
        self.G = CE.Guarded(self.before, dtype, dev, guard)
        self.t = self.G.view[:, c0:] if c0 else self.G.view            # what the launch is handed: pointer at column c0, pitch ld

    def window(self):
        return self.before[:, self.c0: self.c0 + self.C]


def _fail(what, G, got, exp, shape):
    if not torch.equal(got, exp):
        raise AssertionError(f'{what}: {CE.describe_mismatch(got, exp, shape or (1, 1, got.shape[0]))} (column = index into the pitched row)')
    if not G.guards_intact():
        raise AssertionError(f'{what}: wrote outside its operand: (row relative to the tensor, column, value) {G.first_guard_damage()}')


def check_output(o, ref, what, bits=False, pads='keep', shape=None):
    """the whole [M][ld] allocation of output `o` against: its content before the launch with the window replaced by `ref` [M][C] (pads='zero': and every other
    column zeroed, for the kernels that write whole rows); bits: raw bit patterns (copies), else values (torch.equal: -0.0 == 0.0)"""
    exp = torch.zeros_like(o.before) if pads == 'zero' else o.before.clone()
    exp[:, o.c0: o.c0 + o.C] = ref
    got = o.G.view.reshape(exp.shape).cpu()
    if bits:
        _fail(what + ' [raw bit patterns]', o.G, _ibits(got), _ibits(exp), shape)
    else:
        assert not bool(torch.isnan(exp).any())
        _fail(what, o.G, got.float(), exp.float(), shape)


def check_input(o, what):
    got = o.G.view.reshape(o.before.shape).cpu()
    _fail(what + ': an INPUT changed', o.G, _ibits(got), _ibits(o.before), None)


def _pitches(layout, C, k):
    """(ld, c0) of the three operands a, b, y: all pitches differ; 'tight': ld == C; 'slice': windows of wider rows, 16-byte aligned where k is the chunk"""
    if layout == 'tight':
        return (C, 0), (C, 0), (C, 0)
    if layout == 'slice':
        return (C + 3 * k, k), (C + 2 * k, 2 * k), (C + 4 * k, k)
    return (C + k, 0), (C, 0), (C + 2 * k, 0)


# ------------------------------------------------------------------------------------------------------------ add2d / copy_channels
ADD_CASES = ([(op, M, C, 'pitched') for op in ('copy', 'add') for M in (1, 105, 257) for C in ('k', 40, 72)]
             + [(op, 105, 40, lay) for op in ('copy', 'add') for lay in ('tight', 'slice')]
             + [('add_inplace_a', 257, 40, 'pitched'), ('add_inplace_a', 105, 'k', 'slice'), ('add_inplace_b', 105, 72, 'pitched'),
                ('copy_channels', 105, 40, 'slice'), ('copy_channels', 257, 5, 'slice')])


def run_add(ops, dev, case, dt):
    """odtk_add2d: pitched copy (b = None), a + b, in place onto a (retinanet.py / centernet.py: add2d(gx, .., dx, .., gx, ..)) and onto b (refinedet.py:
    add2d(y.g, .., t.g, .., t.g, ..)); odtk_copy_channels as the element-granular channel-slice copy"""
    op, M, C, layout = case
    dtype, k = tdt(dt), kc(dt)
    C = k if C == 'k' else C
    g = _gen('add', case, dt)
    what = f'{op} M={M} C={C} {layout} {dt}'
    if op == 'copy_channels':
        src = Operand(bit_patterns((M, C), dtype, g), C + 4, dtype, dev, IN_PAD, CE.GUARD_IN, c0=3)
        dst = Operand(torch.full((M, C), FRESH, dtype=dtype), C + 9, dtype, dev, PAD, CE.GUARD_OUT, c0=5)
        ops.copy_channels(src.G.view, src.ld, 3, dst.G.view, dst.ld, 5, M, C)
        _sync(dev)
        check_output(dst, src.window(), what, bits=True)
        check_input(src, what)
        return
    (lda, ca), (ldb, cb), (ldy, cy) = _pitches(layout, C, k)
    if op == 'copy':
        a = Operand(bit_patterns((M, C), dtype, g), lda, dtype, dev, IN_PAD, CE.GUARD_IN, ca)
        y = Operand(torch.full((M, C), FRESH, dtype=dtype), ldy, dtype, dev, PAD, CE.GUARD_OUT, cy)
        ops.add2d(a.t, lda, None, 0, y.t, ldy, M, C)
        _sync(dev)
        check_output(y, a.window(), what, bits=True)
        check_input(a, what)
        return
    av, bv = ints((M, C), -25, 25, g), ints((M, C), -25, 25, g)
    ref = _rnd(av + bv, dtype)
    if op == 'add':
        a = Operand(av, lda, dtype, dev, IN_PAD, CE.GUARD_IN, ca)
        b = Operand(bv, ldb, dtype, dev, IN_PAD, CE.GUARD_IN, cb)
        y = Operand(torch.full((M, C), FRESH, dtype=dtype), ldy, dtype, dev, PAD, CE.GUARD_OUT, cy)
        ops.add2d(a.t, lda, b.t, ldb, y.t, ldy, M, C)
        _sync(dev)
        check_output(y, ref, what)
        check_input(a, what)
        check_input(b, what)
    elif op == 'add_inplace_a':
        a = Operand(av, lda, dtype, dev, PAD, CE.GUARD_OUT, ca)
        b = Operand(bv, ldb, dtype, dev, IN_PAD, CE.GUARD_IN, cb)
        ops.add2d(a.t, lda, b.t, ldb, a.t, lda, M, C)
        _sync(dev)
        check_output(a, ref, what)
        check_input(b, what)
    else:
        a = Operand(av, lda, dtype, dev, IN_PAD, CE.GUARD_IN, ca)
        b = Operand(bv, ldb, dtype, dev, PAD, CE.GUARD_OUT, cb)
        ops.add2d(a.t, lda, b.t, ldb, b.t, ldb, M, C)
        _sync(dev)
        check_output(b, ref, what)
        check_input(a, what)


# ------------------------------------------------------------------------------------------------------------ relu(a + b) and the ReLU gradient from the output
RELU_CASES = [(M, C, 'pitched') for M in (1, 105, 257) for C in ('k', 40, 72, 3, 5)] + [(105, 40, 'tight'), (105, 40, 'slice'), (105, 5, 'slice')]


def run_relu(ops, dev, case, dt):
    """odtk_add_relu_fwd (y never aliases an input: refinedet.py:467 is its only call site and hands it three different nodes) and odtk_relu_bwd, overwriting
    and accumulating onto a non-zero dx (refinedet.py:539-540)"""
    M, C, layout = case
    dtype, k = tdt(dt), kc(dt)
    C = k if C == 'k' else C
    g = _gen('relu', case, dt)
    (lda, ca), (ldb, cb), (ldy, cy) = _pitches(layout, C, k)
    what = f'M={M} C={C} {layout} {dt}'
    av, bv = ints((M, C), -25, 25, g), ints((M, C), -25, 25, g)
    a = Operand(av, lda, dtype, dev, IN_PAD, CE.GUARD_IN, ca)
    b = Operand(bv, ldb, dtype, dev, IN_PAD, CE.GUARD_IN, cb)
    y = Operand(torch.full((M, C), FRESH, dtype=dtype), ldy, dtype, dev, PAD, CE.GUARD_OUT, cy)
    ops.add_relu_fwd(a.t, lda, b.t, ldb, y.t, ldy, M, C)
    _sync(dev)
    check_output(y, _rnd(torch.clamp(av + bv, min=0.), dtype), 'add_relu_fwd ' + what)
    check_input(a, 'add_relu_fwd ' + what)
    check_input(b, 'add_relu_fwd ' + what)
    # the gradient: y holds exact zeros of both signs, dy is never zero (so a zero in dx is the mask's doing), dy shares y's pitch
    yv = _rnd(ints((M, C), -25, 25, g), dtype)
    yv.reshape(-1)[::7] = 0.0
    yv.reshape(-1)[3::11] = -0.0
    dyv = ints((M, C), 1, 25, g) * (ints((M, C), 0, 1, g) * 2 - 1)
    prev = ints((M, C), -25, 25, g)
    yo = Operand(yv, ldy, dtype, dev, IN_PAD, CE.GUARD_IN, cy)
    dyo = Operand(dyv, ldy, dtype, dev, IN_PAD, CE.GUARD_IN, cy)
    for acc in (False, True):
        dx = Operand(prev if acc else torch.full((M, C), FRESH, dtype=dtype), lda, dtype, dev, PAD, CE.GUARD_OUT, ca)
        ops.relu_bwd(yo.t, dyo.t, ldy, dx.t, lda, M, C, acc)
        _sync(dev)
        ref = torch.where(yv.double() > 0, dyv, torch.zeros(())) + (prev if acc else 0.)
        w = f'relu_bwd accumulate={acc} ' + what
        check_output(dx, _rnd(ref, dtype), w)
        check_input(yo, w)
        check_input(dyo, w)


# ------------------------------------------------------------------------------------------------------------ nearest-neighbour up-sampling by two
GEOMS = [(1, 1, 1), (2, 5, 7), (3, 2, 4)]          # the SMALL map (N, H, W); the large one is 2H x 2W
UP_CASES = ([(geo, C, 'pitched') for geo in GEOMS for C in ('k', 40)] + [((2, 5, 7), 72, 'pitched'), ((2, 5, 7), 40, 'tight'), ((2, 5, 7), 40, 'slice'),
                                                                         ((3, 2, 4), 'k', 'slice')])


def _small_rows_of(N, H, W):
    """for every row of the [N][2H][2W] map, in order, the row of the [N][H][W] map underneath it -- one pixel at a time"""
    return torch.tensor([(n * H + ho // 2) * W + wo // 2 for n in range(N) for ho in range(2 * H) for wo in range(2 * W)])


def run_upsample(ops, dev, case, dt):
    """odtk_upsample2x_fwd (a copy: bit patterns) and odtk_upsample2x_bwd, overwriting and accumulating onto a non-zero dx; 'slice': yolov3.py hands the gradient
    of the route's concat buffer as dcat[:, bottom.C:]"""
    (N, H, W), C, layout = case
    dtype, k = tdt(dt), kc(dt)
    C = k if C == 'k' else C
    g = _gen('up', case, dt)
    (ldx, cx), _, (ldy, cy) = _pitches(layout, C, k)
    Ms, Ml = N * H * W, N * 4 * H * W
    src = _small_rows_of(N, H, W)
    what = f'N,H,W={N},{H},{W} C={C} {layout} {dt}'
    x = Operand(bit_patterns((Ms, C), dtype, g), ldx, dtype, dev, IN_PAD, CE.GUARD_IN, cx)
    y = Operand(torch.full((Ml, C), FRESH, dtype=dtype), ldy, dtype, dev, PAD, CE.GUARD_OUT, cy)
    ops.upsample2x_fwd(x.t, ldx, y.t, ldy, N, H, W, C)
    _sync(dev)
    check_output(y, x.window()[src], 'upsample2x_fwd ' + what, bits=True, shape=(N, 2 * H, 2 * W))
    check_input(x, 'upsample2x_fwd ' + what)
    dyv, prev = ints((Ml, C), -25, 25, g), ints((Ms, C), -25, 25, g)
    summed = torch.zeros(Ms, C, dtype=torch.float64)
    for r in range(Ml):                                         # each large-map pixel's gradient goes to the pixel it was copied from
        summed[src[r]] += dyv[r]
    dy = Operand(dyv, ldy, dtype, dev, IN_PAD, CE.GUARD_IN, cy)
    for acc in (False, True):
        dx = Operand(prev if acc else torch.full((Ms, C), FRESH, dtype=dtype), ldx, dtype, dev, PAD, CE.GUARD_OUT, cx)
        ops.upsample2x_bwd(dy.t, ldy, dx.t, ldx, N, H, W, C, acc)
        _sync(dev)
        w = f'upsample2x_bwd accumulate={acc} ' + what
        check_output(dx, _rnd(summed + (prev if acc else 0.), dtype), w, shape=(N, H, W))
        check_input(dy, w)


# ------------------------------------------------------------------------------------------------------------ 2 x 2 average pooling
AVG_CASES = [(geo, ld) for geo in GEOMS for ld in ('k', 40, 72, 3, 5)]


def run_avgpool(ops, dev, case, dt):
    """odtk_avgpool2x2_fwd / _bwd: all ld columns are processed, so there are no pad columns -- the guards are what is left to damage"""
    (N, H, W), ld = case
    dtype = tdt(dt)
    ld = kc(dt) if ld == 'k' else ld
    g = _gen('avg', case, dt)
    Ms, Ml = N * H * W, N * 4 * H * W
    src = _small_rows_of(N, H, W)
    what = f'N,H,W={N},{2 * H},{2 * W} ld={ld} {dt}'
    xv = ints((Ml, ld), -32, 32, g)
    mean = torch.zeros(Ms, ld, dtype=torch.float64)
    for r in range(Ml):
        mean[src[r]] += xv[r]
    mean /= 4.
    x = Operand(xv, ld, dtype, dev, IN_PAD, CE.GUARD_IN)
    y = Operand(torch.full((Ms, ld), FRESH, dtype=dtype), ld, dtype, dev, PAD, CE.GUARD_OUT)
    ops.avgpool2x2_fwd(x.t, y.t, N, 2 * H, 2 * W, ld)
    _sync(dev)
    check_output(y, _rnd(mean, dtype), 'avgpool2x2_fwd ' + what, shape=(N, H, W))
    check_input(x, 'avgpool2x2_fwd ' + what)
    dyv = ints((Ms, ld), -64, 64, g)
    dy = Operand(dyv, ld, dtype, dev, IN_PAD, CE.GUARD_IN)
    dx = Operand(torch.full((Ml, ld), FRESH, dtype=dtype), ld, dtype, dev, PAD, CE.GUARD_OUT)
    ops.avgpool2x2_bwd(dy.t, dx.t, N, 2 * H, 2 * W, ld)
    _sync(dev)
    check_output(dx, _rnd((dyv / 4.)[src], dtype), 'avgpool2x2_bwd ' + what, shape=(N, 2 * H, 2 * W))
    check_input(dy, 'avgpool2x2_bwd ' + what)


# ------------------------------------------------------------------------------------------------------------ conv rows <-> f32 prediction tensors
# 'window': three images of 35 rows (35 does not divide a workgroup of 256) into a prediction tensor [3][100][ldy] entered at row 20 (retinanet.py:342 / :370);
# 'window_pitched': ldy > C; 'stride0': one "image" of M rows, y_img_stride = 0 (fcos.py:296 / :317); 'tight': ldx == C
ROWS_CASES = ([(105, C, 'window') for C in ('k', 40, 72, 3, 5)] + [(105, 'k', 'window_pitched'), (105, 5, 'window_pitched'), (105, 40, 'window_tight')]
              + [(M, C, 'stride0') for M in (1, 257) for C in ('k', 40, 72, 3, 5)] + [(105, 'k', 'stride0')])
_A, _ROW0, _RPI = 100, 20, 35


def run_rows(ops, dev, case, dt):
    M, C, mode = case
    dtype, k = tdt(dt), kc(dt)
    C = k if C == 'k' else C
    g = _gen('rows', case, dt)
    ldx = C if mode == 'window_tight' else C + k
    ldy = C + 2 if mode == 'window_pitched' else C
    if mode == 'stride0':
        rpi, stride, rows_y, row0 = M, 0, M, 0
        dest = torch.arange(M)
    else:
        assert M == 3 * _RPI
        rpi, stride, rows_y, row0 = _RPI, _A * ldy, 3 * _A, _ROW0
        dest = torch.tensor([n * _A + _ROW0 + j for n in range(3) for j in range(_RPI)])      # row of the prediction tensor that row m of x lands in
    what = f'M={M} C={C} ldx={ldx} ldy={ldy} rows_per_img={rpi} y_img_stride={stride} {dt}'
    # rows -> f32: a widening copy; every row outside the windows keeps the sentinel
    x = Operand(bit_patterns((M, C), dtype, g), ldx, dtype, dev, IN_PAD, CE.GUARD_IN)
    y = Operand(torch.full((rows_y, C), PAD, dtype=torch.float32), ldy, torch.float32, dev, PAD, CE.GUARD_OUT)
    ops.rows_to_f32(x.t, ldx, y.t[row0:], ldy, rpi, stride, M, C)
    _sync(dev)
    ref = y.window().clone()
    ref[dest] = x.window().float()
    check_output(y, ref, 'rows_to_f32 ' + what, bits=True)
    check_input(x, 'rows_to_f32 ' + what)
    # f32 -> rows: one rounding; the rows outside the windows hold other numbers, the pad columns of x come back zero
    yv = Operand(bit_patterns((rows_y, C), torch.float32, g), ldy, torch.float32, dev, IN_PAD, CE.GUARD_IN)
    xo = Operand(torch.full((M, C), FRESH, dtype=dtype), ldx, dtype, dev, PAD, CE.GUARD_OUT)
    ops.rows_from_f32(yv.t[row0:], ldy, rpi, stride, xo.t, ldx, M, C)
    _sync(dev)
    check_output(xo, yv.window()[dest].to(dtype), 'rows_from_f32 ' + what, bits=True, pads='zero')
    check_input(yv, 'rows_from_f32 ' + what)


# ------------------------------------------------------------------------------------------------------------ exp rows
EXP_CASES = [(M, C, 'pitched') for M in (1, 105, 257) for C in ('k', 40, 72, 3, 5)] + [(105, 40, 'tight')]


def ulp_error(y32, ref64):
    """largest |y - ref| in units of the f32 spacing at ref (subnormal spacing below the normal range); on whatever device the operands are"""
    r = ref64.float().abs()
    ulp = torch.nextafter(r, torch.full_like(r, float('inf'))).double() - r.double()
    return float(((y32.double() - ref64).abs() / ulp).max())


def run_exp(ops, dev, case, dt):
    """odtk_exp_rows_to_f32 within (torch.exp in f32 on the same device and inputs) + 1 ulp of float64 exp; odtk_exp_rows_bwd exact.  Returns (kernel's ulp error,
    torch.exp's ulp error)"""
    M, C, layout = case
    dtype, k = tdt(dt), kc(dt)
    C = k if C == 'k' else C
    g = _gen('exp', case, dt)
    ldx = C if layout == 'tight' else C + k
    what = f'M={M} C={C} ldx={ldx} {dt}'
    xv = ((torch.rand(M, C, generator=g) * 40. - 20.).to(dtype)).double()           # [-20, 20], rounded to the dtype first: exp of the LOADED value
    xv.reshape(-1)[:3] = torch.tensor([0., 88., -88.], dtype=torch.float64)           # (exp(-88) = 6.05e-39 is a subnormal f32)
    x = Operand(xv, ldx, dtype, dev, IN_PAD, CE.GUARD_IN)
    y = Operand(torch.full((M, C), PAD, dtype=torch.float32), C, torch.float32, dev, PAD, CE.GUARD_OUT)
    ops.exp_rows_to_f32(x.t, ldx, y.t, M, C)
    _sync(dev)
    ref = torch.exp(xv)
    got = y.G.view.cpu()
    err = ulp_error(got, ref)
    torch_err = ulp_error(torch.exp(xv.float().to(dev)).cpu(), ref)
    print(f'exp_rows_to_f32 {what}: kernel {err:.3f} ulp, torch.exp on {torch.device(dev).type} {torch_err:.3f} ulp')
    assert err <= torch_err + 1., f'exp_rows_to_f32 {what}: {err:.3f} ulp from float64 exp; torch.exp in f32 on the same inputs: {torch_err:.3f} ulp'
    assert y.G.guards_intact(), f'exp_rows_to_f32 {what}: wrote outside its output {y.G.first_guard_damage()}'
    check_input(x, 'exp_rows_to_f32 ' + what)
    # chain rule: given y, one f32 multiply and one rounding; pad columns of dx zeroed
    dyv = torch.randn(M, C, generator=g)
    dyo = Operand(dyv, C, torch.float32, dev, IN_PAD, CE.GUARD_IN)
    yo = Operand(got, C, torch.float32, dev, IN_PAD, CE.GUARD_IN)
    dx = Operand(torch.full((M, C), FRESH, dtype=dtype), ldx, dtype, dev, PAD, CE.GUARD_OUT)
    ops.exp_rows_bwd(dyo.t, yo.t, dx.t, ldx, M, C)
    _sync(dev)
    check_output(dx, (dyv * got).to(dtype), 'exp_rows_bwd ' + what, pads='zero')
    check_input(dyo, 'exp_rows_bwd ' + what)
    check_input(yo, 'exp_rows_bwd ' + what)
    return err, torch_err


# ------------------------------------------------------------------------------------------------------------ preprocess_norm
PRE_CASES = [(1, 1, 1), (2, 16, 12), (1, 17, 31)]


def run_preprocess_norm(ops, dev, case, dt, mean3=MEAN, std3=STD):
    """(images / div - mean) / std in exactly this f32 order, channels 3 .. ldx - 1 zeroed"""
    N, H, W = case
    dtype = tdt(dt)
    DT = ops.F32 if dt == 'f32' else ops.BF16
    g = _gen('pre', case, dt)
    for ldx in (kc(dt), 3, 5):
        what = f'preprocess_norm N,H,W={N},{H},{W} ldx={ldx} {dt}'
        img = torch.randint(0, 256, (N * H * W, 3), generator=g).float()
        im = Operand(img, 3, torch.float32, dev, IN_PAD, CE.GUARD_IN)
        x = Operand(torch.full((N * H * W, 3), FRESH, dtype=dtype), ldx, dtype, dev, PAD, CE.GUARD_OUT)
        ops.preprocess_norm(im.t, 255., mean3, std3, ldx, DT, x.t)
        _sync(dev)
        want = (img / 255. - torch.tensor(mean3, dtype=torch.float32)) / torch.tensor(std3, dtype=torch.float32)
        check_output(x, want.to(dtype), what, pads='zero', shape=(N, H, W))
        check_input(im, what)


# ------------------------------------------------------------------------------------------------------------ casts
CAST_NS = [0, 1, 7, 8, 9, 1000, 1001, 1007, 4099]
CAST_OFFSETS = [(s, d) for s in (0, 1, 3, 4) for d in (0, 1, 3, 4)]
# with 4-byte and 2-byte elements a view 4 elements into an aligned buffer is aligned on the f32 side and not on the bf16 side; 1 and 3 are aligned on neither:
# (0, 0) and f32-side 4 take the 8-per-thread kernel (+ its tail launch when n % 8), everything else the scalar kernel -- seen here only through the result


def _cast_source_f32(n, g):
    """f32 bit patterns for the narrowing cast: ties (low half exactly 0x8000) above even and above odd upper halves, one below and one above a tie, the largest
    finite f32 (rounds to inf), +-0, subnormals (a tie among them), +-inf, NaNs; then normals over 12 decades with every fifth turned into a tie"""
    sp = [0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001, 0x7f7fffff, 0xff7fffff, 0x00000000, 0x80000000,
          0x00000001, 0x007fffff, 0x80000001, 0x00008000, 0x00018000, 0x00007fff, 0x7f800000, 0xff800000, 0x7f7f8000, 0x7f7e8000,
          0x7fc00000, 0x7f800001, 0xffc00001, 0x7fffffff]
    sp = torch.tensor([v - 2 ** 32 if v >= 2 ** 31 else v for v in sp], dtype=torch.int64).to(torch.int32)
    if n <= sp.numel():
        return sp[:n].clone().view(torch.float32)
    m = n - sp.numel()
    v = torch.randn(m, generator=g) * 10. ** (torch.rand(m, generator=g) * 12. - 6.)
    b = v.view(torch.int32).clone()
    b[::5] = (b[::5] & -65536) | 0x8000
    return torch.cat([sp, b]).view(torch.float32)


def _flat_operand(window, n, off, dtype, dev, pad, guard):
    """1-D: `off` sentinels, the n elements the launch sees, 8 sentinels -- between guard bands; returns (Guarded, its content before, the view handed over)"""
    before = torch.full((off + n + 8,), pad, dtype=dtype)
    before[off: off + n] = window
    G = CE.Guarded(before, dtype, dev, guard)
    return G, before, G.view[off: off + n]


def _check_flat(G, before, ref, n, off, what):
    exp = before.clone()
    exp[off: off + n] = ref
    got = G.view.cpu()
    nan = torch.isnan(exp)
    assert torch.equal(torch.isnan(got), nan), f'{what}: NaN in must give NaN out (and nothing else may)'
    gb, eb = _ibits(got).masked_fill(nan, 0), _ibits(exp).masked_fill(nan, 0)
    _fail(what + ' [raw bit patterns; index = element of the buffer, the view starts at ' + str(off) + ']', G, gb.reshape(-1, 1), eb.reshape(-1, 1), None)


def run_cast(ops, dev, n, dt):
    """odtk_cast_from_f32 / odtk_cast_to_f32 on views of every alignment; the sentinels directly in front of element 0 and behind element n - 1 survive"""
    dtype = tdt(dt)
    g = _gen('cast', n, dt)
    for so, do in (CAST_OFFSETS if n >= 9 else [(0, 0)]):
        what = f'n={n} source view at +{so}, destination view at +{do}, {dt}'
        src32 = _cast_source_f32(n, g)
        S, sb, sv = _flat_operand(src32, n, so, torch.float32, dev, IN_PAD, CE.GUARD_IN)
        D, db, dv = _flat_operand(torch.full((n,), FRESH, dtype=dtype), n, do, dtype, dev, PAD, CE.GUARD_OUT)
        ops.cast_from_f32(sv, dv)
        _sync(dev)
        _check_flat(D, db, src32.to(dtype), n, do, 'cast_from_f32 ' + what)
        _check_flat(S, sb, src32, n, so, 'cast_from_f32 ' + what + ': an INPUT changed')
        # widening: arbitrary bit patterns of the narrow type, compared as raw bits
        srcn = bit_patterns((n,), dtype, g)
        S, sb, sv = _flat_operand(srcn, n, so, dtype, dev, IN_PAD, CE.GUARD_IN)
        D, db, dv = _flat_operand(torch.full((n,), FRESH), n, do, torch.float32, dev, PAD, CE.GUARD_OUT)
        ops.cast_to_f32(sv, dv)
        _sync(dev)
        _check_flat(D, db, srcn.float(), n, do, 'cast_to_f32 ' + what)
        _check_flat(S, sb, srcn, n, so, 'cast_to_f32 ' + what + ': an INPUT changed')


# ------------------------------------------------------------------------------------------------------------ over the grid cap
# Every launch here is a grid-stride loop behind `grid_for(total, 256, cap)`; below, `total` exceeds cap * 256 by one partial workgroup (130 work items or a few
# more), so that some threads run their loop a second time and the others do not.  Caps as of csrc/elementwise.hip and csrc/centernet_net.hip:
#   cast_*_x8_kernel, cast_kernel, cast_to_f32_kernel           grid_for(n8 | n, 256)             cap  8 192   (total in 8-element groups | elements)
#   add2d / upsample2x_fwd / upsample2x_bwd                     grid_for(rows * (C / kc), 256, 65536)          (16-byte chunks)
#   copy_channels, rows_to_f32, exp_rows_to_f32                 grid_for(M * C, 256, 65536)
#   rows_from_f32, exp_rows_bwd                                 grid_for(M * ldx, 256, 65536)
#   add_relu / relu_bwd / avgpool2x2                            grid_for(M * C | N Ho Wo ld, 256)  cap 65 536  (centernet_net.hip's default)
#   preprocess_norm                                             grid_for(pixels, 256, 8192)
# Operands and expectations are made on the device from index-derived integers (exact in bf16: |v| <= 256), C is as small as the kernel allows.
CAP_SMALL, CAP_LARGE, EXTRA = 8192, 65536, 130
OVERCAP = [('cast_x8', 'bf16'), ('cast_scalar', 'f32'), ('cast_scalar', 'bf16')] + [(n, dt) for n in (
    'add2d', 'upsample2x_fwd', 'upsample2x_bwd', 'copy_channels', 'add_relu', 'relu_bwd', 'avgpool2x2_fwd', 'avgpool2x2_bwd', 'rows_to_f32', 'rows_from_f32',
    'exp_rows_to_f32', 'exp_rows_bwd', 'preprocess_norm') for dt in ('f32', 'bf16')]


def _pat(n, mod, off, dev):
    """(i % mod) - off for i < n, f32 on the device"""
    return (torch.arange(n, dtype=torch.int32, device=dev) % mod - off).float()


def _dev_rows(window, ld, pad, dtype, dev, guard):
    """a Guarded [M][ld] made ON the device from the f32 window [M][C]; returns (Guarded, what it holds now)"""
    M, C = window.shape
    full = torch.full((M, ld), pad, dtype=dtype, device=dev)
    full[:, :C] = window.to(dtype)
    return CE.Guarded(full, dtype, dev, guard), full


def _check_dev(G, exp, what):
    got = G.view.reshape(exp.shape)
    if not torch.equal(got, exp):
        bad = (got != exp).nonzero()
        first = [(tuple(i), float(got[tuple(i)]), float(exp[tuple(i)])) for i in bad[:8].tolist()]
        raise AssertionError(f'{what}: {bad.shape[0]} of {exp.numel()} elements differ; first (index, got, expected): {first}')
    if not G.guards_intact():
        raise AssertionError(f'{what}: wrote outside its operand: {G.first_guard_damage()}')


def run_overcap(ops, dev, name, dt, mean3=MEAN, std3=STD):
    dtype, k = tdt(dt), kc(dt)
    what = f'{name} {dt} over the grid cap'
    big = CAP_LARGE * T + EXTRA

    def rows_for(per_row):
        return -(-big // per_row)

    if name in ('cast_x8', 'cast_scalar'):
        n = (CAP_SMALL * T + EXTRA) * 8 + 5 if name == 'cast_x8' else CAP_SMALL * T + EXTRA
        off = 1 if (name == 'cast_scalar' and dt == 'bf16') else 0               # a bf16 job reaches the scalar kernel through a misaligned view
        vals = _pat(n, 251, 125, dev)
        pre = torch.full((off,), IN_PAD, device=dev)
        S = CE.Guarded(torch.cat([pre, vals]), torch.float32, dev, CE.GUARD_IN)
        D = CE.Guarded(torch.full((off + n,), PAD, device=dev), dtype, dev, CE.GUARD_OUT)
        ops.cast_from_f32(S.view[off:], D.view[off:])
        _sync(dev)
        exp = torch.cat([torch.full((off,), PAD, device=dev), vals]).to(dtype)
        _check_dev(D, exp, what + ' (from f32)')
        W = CE.Guarded(torch.full((off + n,), PAD, device=dev), torch.float32, dev, CE.GUARD_OUT)
        ops.cast_to_f32(D.view[off:], W.view[off:])
        _sync(dev)
        _check_dev(W, exp.float(), what + ' (to f32)')
        _check_dev(D, exp, what + ' (to f32: input)')
        _check_dev(S, torch.cat([pre, vals]), what + ' (from f32: input)')
    elif name == 'add2d':
        M, C = big, k
        A, a0 = _dev_rows(_pat(M * C, 251, 125, dev).view(M, C), C, IN_PAD, dtype, dev, CE.GUARD_IN)
        B, b0 = _dev_rows(_pat(M * C, 127, 63, dev).view(M, C), C, IN_PAD, dtype, dev, CE.GUARD_IN)
        Y, y0 = _dev_rows(torch.full((M, C), FRESH, device=dev), 2 * C, PAD, dtype, dev, CE.GUARD_OUT)
        ops.add2d(A.view, C, B.view, C, Y.view, 2 * C, M, C)
        _sync(dev)
        y0[:, :C] = (a0.float() + b0.float()).to(dtype)
        _check_dev(Y, y0, what)
        _check_dev(A, a0, what + ' (input a)')
        _check_dev(B, b0, what + ' (input b)')
    elif name == 'upsample2x_fwd':
        W_, C = -(-big // 4), k                                                   # N = H = 1: 4 W rows of one chunk
        X, x0 = _dev_rows(_pat(W_ * C, 251, 125, dev).view(W_, C), C, IN_PAD, dtype, dev, CE.GUARD_IN)
        Y, y0 = _dev_rows(torch.full((4 * W_, C), FRESH, device=dev), 2 * C, PAD, dtype, dev, CE.GUARD_OUT)
        ops.upsample2x_fwd(X.view, C, Y.view, 2 * C, 1, 1, W_, C)
        _sync(dev)
        twice = x0.repeat_interleave(2, 0)
        y0[:, :C] = torch.cat([twice, twice])
        _check_dev(Y, y0, what)
        _check_dev(X, x0, what + ' (input)')
    elif name == 'upsample2x_bwd':
        W_, C = big, k                                                            # N = H = 1: W rows of one chunk, accumulating onto a non-zero dx
        DY, dy0 = _dev_rows(_pat(4 * W_ * C, 51, 25, dev).view(4 * W_, C), C, IN_PAD, dtype, dev, CE.GUARD_IN)
        prev = _pat(W_ * C, 47, 23, dev).view(W_, C)
        DX, dx0 = _dev_rows(prev, 2 * C, PAD, dtype, dev, CE.GUARD_OUT)
        ops.upsample2x_bwd(DY.view, C, DX.view, 2 * C, 1, 1, W_, C, True)
        _sync(dev)
        dx0[:, :C] = (dy0.float().view(2, W_, 2, C).sum((0, 2)) + prev).to(dtype)
        del prev
        _check_dev(DX, dx0, what)
        _check_dev(DY, dy0, what + ' (input)')
    elif name == 'copy_channels':
        M, C = rows_for(3), 3
        S, s0 = _dev_rows(_pat(M * 4, 251, 125, dev).view(M, 4), 4, IN_PAD, dtype, dev, CE.GUARD_IN)
        D, d0 = _dev_rows(torch.full((M, 5), PAD, device=dev), 5, PAD, dtype, dev, CE.GUARD_OUT)
        ops.copy_channels(S.view, 4, 1, D.view, 5, 1, M, C)
        _sync(dev)
        d0[:, 1:4] = s0[:, 1:4]
        _check_dev(D, d0, what)
        _check_dev(S, s0, what + ' (input)')
    elif name in ('add_relu', 'relu_bwd'):
        M, C = rows_for(3), 3
        A, a0 = _dev_rows(_pat(M * C, 251, 125, dev).view(M, C), 4, IN_PAD, dtype, dev, CE.GUARD_IN)
        B, b0 = _dev_rows(_pat(M * C, 127, 63, dev).view(M, C), 4 if name == 'relu_bwd' else 3, IN_PAD, dtype, dev, CE.GUARD_IN)
        if name == 'add_relu':
            Y, y0 = _dev_rows(torch.full((M, C), FRESH, device=dev), 5, PAD, dtype, dev, CE.GUARD_OUT)
            ops.add_relu_fwd(A.view, 4, B.view, 3, Y.view, 5, M, C)
            _sync(dev)
            y0[:, :C] = torch.relu(a0[:, :C].float() + b0.float()).to(dtype)
        else:                                                                      # A is the ReLU output y, B is dy (same pitch), accumulate onto dx
            prev = _pat(M * C, 47, 23, dev).view(M, C)
            Y, y0 = _dev_rows(prev, 5, PAD, dtype, dev, CE.GUARD_OUT)
            ops.relu_bwd(A.view, B.view, 4, Y.view, 5, M, C, True)
            _sync(dev)
            y0[:, :C] = (torch.where(a0[:, :C].float() > 0, b0[:, :C].float(), torch.zeros((), device=dev)) + prev).to(dtype)
        _check_dev(Y, y0, what)
        _check_dev(A, a0, what + ' (input)')
        _check_dev(B, b0, what + ' (input)')
    elif name in ('avgpool2x2_fwd', 'avgpool2x2_bwd'):
        Wo, ld = rows_for(3), 3                                                    # N = 1, Ho = 1: the large map is [2][2 Wo][3]
        if name == 'avgpool2x2_fwd':
            X, x0 = _dev_rows(_pat(4 * Wo * ld, 65, 32, dev).view(4 * Wo, ld), ld, IN_PAD, dtype, dev, CE.GUARD_IN)
            Y, y0 = _dev_rows(torch.full((Wo, ld), FRESH, device=dev), ld, PAD, dtype, dev, CE.GUARD_OUT)
            ops.avgpool2x2_fwd(X.view, Y.view, 1, 2, 2 * Wo, ld)
            _sync(dev)
            y0 = (x0.float().view(2, Wo, 2, ld).sum((0, 2)) / 4.).to(dtype)
        else:
            X, x0 = _dev_rows(_pat(Wo * ld, 129, 64, dev).view(Wo, ld), ld, IN_PAD, dtype, dev, CE.GUARD_IN)
            Y, y0 = _dev_rows(torch.full((4 * Wo, ld), FRESH, device=dev), ld, PAD, dtype, dev, CE.GUARD_OUT)
            ops.avgpool2x2_bwd(X.view, Y.view, 1, 2, 2 * Wo, ld)
            _sync(dev)
            y0 = (x0.float() / 4.).to(dtype).view(1, Wo, 1, ld).expand(2, Wo, 2, ld).reshape(4 * Wo, ld)
        _check_dev(Y, y0, what)
        _check_dev(X, x0, what + ' (input)')
    elif name == 'rows_to_f32':
        M, C = rows_for(3), 3
        X, x0 = _dev_rows(_pat(M * C, 251, 125, dev).view(M, C), 4, IN_PAD, dtype, dev, CE.GUARD_IN)
        Y, y0 = _dev_rows(torch.full((M, C), PAD, device=dev), 5, PAD, torch.float32, dev, CE.GUARD_OUT)
        ops.rows_to_f32(X.view, 4, Y.view, 5, M, 0, M, C)
        _sync(dev)
        y0[:, :C] = x0[:, :C].float()
        _check_dev(Y, y0, what)
        _check_dev(X, x0, what + ' (input)')
    elif name == 'rows_from_f32':
        M, C = rows_for(4), 3                                                      # total = M * ldx
        Yv, yv0 = _dev_rows(_pat(M * C, 251, 125, dev).view(M, C), 5, IN_PAD, torch.float32, dev, CE.GUARD_IN)
        X, x0 = _dev_rows(torch.full((M, C), FRESH, device=dev), 4, PAD, dtype, dev, CE.GUARD_OUT)
        ops.rows_from_f32(Yv.view, 5, M, 0, X.view, 4, M, C)
        _sync(dev)
        x0.zero_()
        x0[:, :C] = yv0[:, :C].to(dtype)
        _check_dev(X, x0, what)
        _check_dev(Yv, yv0, what + ' (input)')
    elif name == 'exp_rows_to_f32':
        M, C = rows_for(3), 3
        X, x0 = _dev_rows(_pat(M * C, 41, 20, dev).view(M, C), 4, IN_PAD, dtype, dev, CE.GUARD_IN)
        Y = CE.Guarded(torch.full((M, C), PAD, device=dev), torch.float32, dev, CE.GUARD_OUT)
        ops.exp_rows_to_f32(X.view, 4, Y.view, M, C)
        _sync(dev)
        xf = x0[:, :C].float()
        ref = torch.exp(xf.double())
        err, torch_err = ulp_error(Y.view, ref), ulp_error(torch.exp(xf), ref)
        assert err <= torch_err + 1., f'{what}: {err:.3f} ulp from float64 exp; torch.exp in f32: {torch_err:.3f} ulp'
        assert Y.guards_intact(), f'{what}: wrote outside its output {Y.first_guard_damage()}'
        _check_dev(X, x0, what + ' (input)')
    elif name == 'exp_rows_bwd':
        M, C = rows_for(4), 3                                                      # total = M * lddx
        DY, dy0 = _dev_rows(_pat(M * C, 23, 11, dev).view(M, C), C, IN_PAD, torch.float32, dev, CE.GUARD_IN)
        Yv, yv0 = _dev_rows(_pat(M * C, 11, -1, dev).view(M, C), C, IN_PAD, torch.float32, dev, CE.GUARD_IN)
        DX, dx0 = _dev_rows(torch.full((M, C), FRESH, device=dev), 4, PAD, dtype, dev, CE.GUARD_OUT)
        ops.exp_rows_bwd(DY.view, Yv.view, DX.view, 4, M, C)
        _sync(dev)
        dx0.zero_()
        dx0[:, :C] = (dy0 * yv0).to(dtype)
        _check_dev(DX, dx0, what)
        _check_dev(DY, dy0, what + ' (input)')
        _check_dev(Yv, yv0, what + ' (input)')
    elif name == 'preprocess_norm':
        pixels = CAP_SMALL * T + EXTRA
        img = (torch.arange(pixels * 3, dtype=torch.int32) % 256).float().view(pixels, 3)                    # (the f32 division is the CPU's: torch divides by a
        want = (img / 255. - torch.tensor(mean3, dtype=torch.float32)) / torch.tensor(std3, dtype=torch.float32)   # scalar on the device as a product with 1 / 255)
        IM = CE.Guarded(img.to(dev), torch.float32, dev, CE.GUARD_IN)
        X, x0 = _dev_rows(torch.full((pixels, 3), FRESH, device=dev), k, PAD, dtype, dev, CE.GUARD_OUT)
        ops.preprocess_norm(IM.view, 255., mean3, std3, k, ops.F32 if dt == 'f32' else ops.BF16, X.view)
        _sync(dev)
        x0.zero_()
        x0[:, :3] = want.to(dtype).to(dev)
        _check_dev(X, x0, what)
        _check_dev(IM, img.to(dev), what + ' (input)')
    else:
        raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------ the global batch-norm entry points
BN_GLOBAL_SHAPES = [(2 * 13 * 13, 96, True), (5000, 40, False)]


def global_batch_norm_case(ops, dev, shape, dt, ctx):
    """odtk_bn_moments / _fwd_given / _bwd_sums / _bwd_given (ops.SyncBN, SURVEY.md 8e option B) with the two exchanges done by hand: two replicas with half the
    rows each compute what odtk_bn_fwd / odtk_bn_bwd compute on all rows.  ctx: hip_cpu_backend.installed() on the CPU, a null context on the GPU."""
    M, C, relu = shape
    dtype = tdt(dt)
    g = torch.Generator().manual_seed(5)
    z = (torch.randn(2 * M, C, generator=g) * 1.5 + 0.3).to(dtype).to(dev)
    dy = torch.randn(2 * M, C, generator=g).to(dtype).to(dev)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
    zeros = lambda *s, **k: torch.zeros(*s, device=dev, **k)      # noqa: E731
    ones = lambda *s: torch.ones(*s, device=dev)                  # noqa: E731
    with ctx:
        p, st_ = ops._p, ops._stream()
        ws = zeros(ops.bn_workspace_bytes(2 * M, C), dtype=torch.uint8)
        # one device, all rows
        mm, mv, sm, si = zeros(C), ones(C), zeros(C), zeros(C)
        y, dz, dg, db = zeros(2 * M, C, dtype=dtype), zeros(2 * M, C, dtype=dtype), zeros(C), zeros(C)
        ops.bn_fwd(z, 2 * M, C, C, gamma, beta, mm, mv, sm, si, True, int(relu), y, C, 2 * M, 0, ws)
        ops.bn_bwd(z, y, dy, 2 * M, C, C, C, 2 * M, 0, gamma, sm, si, int(relu), dz, dg, db, ws)
        # two replicas
        zs, dys = [z[:M].clone(), z[M:].clone()], [dy[:M].clone(), dy[M:].clone()]
        mom = zeros(2, 2, C)
        for r in range(2):
            ops.call('odtk_bn_moments', p(zs[r]), M, C, C, ops.dt_of(zs[r]), p(mom[r][0]), p(mom[r][1]), p(ws), st_)
        st = [dict(mm=zeros(C), mv=ones(C), sm=zeros(C), si=zeros(C), y=zeros(M, C, dtype=dtype), dz=zeros(M, C, dtype=dtype), sums=zeros(2 * C)) for _ in range(2)]
        for r in range(2):
            d = st[r]
            ops.call('odtk_bn_fwd_given', p(zs[r]), M, C, C, ops.dt_of(zs[r]), p(gamma), p(beta), p(mom), 2, p(d['mm']), p(d['mv']), p(d['sm']), p(d['si']),
                     int(relu), p(d['y']), ops.dt_of(d['y']), C, M, 0, p(ws), st_)
            d['y1'] = y[r * M:(r + 1) * M].clone()          # the ReLU mask of the one-device pass: an activation a rounding away from zero must not flip
            ops.call('odtk_bn_bwd_sums', p(zs[r]), p(d['y1']), p(dys[r]), M, C, C, ops.dt_of(zs[r]), ops.dt_of(dys[r]), C, M, 0, p(d['sm']), p(d['si']), int(relu),
                     p(d['sums']), p(ws), st_)
        _sync(dev)
        glob = st[0]['sums'] + st[1]['sums']
        for r in range(2):
            d = st[r]
            ops.call('odtk_bn_bwd_given', p(zs[r]), p(d['y1']), p(dys[r]), M, C, C, ops.dt_of(zs[r]), ops.dt_of(dys[r]), C, M, 0, p(gamma), p(d['sm']), p(d['si']),
                     int(relu), p(glob), 2 * M, p(d['dz']), p(ws), st_)
        _sync(dev)
    tol = 2e-5 if dt == 'f32' else 2e-2

    def close(a, b, t=tol):
        a, b = a.float().cpu(), b.float().cpu()
        assert float((a - b).abs().max()) <= t * (float(b.abs().max()) + 1e-6), float((a - b).abs().max())
    for r in range(2):
        d = st[r]
        close(d['sm'], sm, 2e-5); close(d['si'], si, 2e-4); close(d['mm'], mm, 2e-5); close(d['mv'], mv, 2e-4)
        close(d['y'], y[r * M:(r + 1) * M])
        close(d['dz'], dz[r * M:(r + 1) * M])
    if dt == 'f32':                                         # (bf16: a ReLU mask taken from y rounded differently in a few entries moves the sums)
        close(glob[:C], db, 1e-4); close(glob[C:], dg, 1e-4)
    else:
        close(glob[:C], db, 3e-2); close(glob[C:], dg, 3e-2)
