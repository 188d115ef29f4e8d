"""Integer operands for which every convolution pass has ONE right answer, bit for bit (plain module, no tests; used by tests/test_gpu_conv_exact.py on the GPU
and by tests/test_conv_exact_cpu.py without one).

Every conv kernel multiplies in bf16 or f32 and accumulates in f32.  With operands in {-1, 0, +1} every product and every partial sum is a small integer, so the
result does not depend on the summation order, on split-K, on atomics or on the flush order; and while |result| <= 256 it is exactly representable in bf16, so the
store rounding is the identity.  A kernel's output must then equal the reference exactly (torch.equal), and one dropped, duplicated or mis-addressed term moves
some output by at least 1.

Arrangement A (every activation element counts): activations dense in {-1, +1}; filter in {-1, 0, +1} with at most CAP non-zeros per reduction set (per output
channel over (tap, c) forward, per input channel over (k, tap) for the input gradient), laid out through a fixed permutation so that every reduction position is
non-zero for some channel -- in `rounds_*()` rounds with shifted offsets where channels * CAP < positions.
Arrangement B (every filter element counts): filter dense in {-1, +1}; activations in {-1, 0, +1} with at most floor(CAP / (k k)) non-zero channels per pixel,
rotating with the pixel index so that every channel is hit (again in rounds where pixels * m < channels).
Filter gradient: x and dy dense in {-1, +1}: |dw| <= N Ho Wo < 2^24, f32 output, exact; `bounded=True` caps dy per pixel as in B, for a path
that stores partials narrower than f32 (none does today: DESIGN.md section 5).

The generators ASSERT the bound they promise on the reference itself, so no case is vacuously exact.  Reference: oracle.ssd300_ref.conv2d_same in f32 on the CPU
(autograd for the gradients) -- exact for the reason above; `dtype=torch.float64` gives the same numbers (checked in the CPU tier)."""
import collections

import torch
import torch.nn.functional as F

from oracle import ssd300_ref as R

CAP = 256                     # non-zero terms per output element at most: |sum| <= 256 is exact in bf16
BF16_EXACT = 256
F32_EXACT = 1 << 24
GUARD_ROWS = 512              # rows (of the operand's own pitch) in front of and behind every device operand
GUARD_IN = 16384.0            # exact in bf16; a guard row read where a mask should have given zero: an error of >= 16384
GUARD_OUT = -8192.0           # sentinel around every result


def pad_to(c, m):
    return (c + m - 1) // m * m


def _gen(*key):
    s = 12345
    for v in key:
        s = (s * 1000003 + int(v) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _signs(shape, g):
    return (torch.randint(0, 2, shape, generator=g, dtype=torch.int8) * 2 - 1).float()


def same_out(size, stride):
    return -(-size // stride)


# ------------------------------------------------------------------------------------------------------------ sparsity patterns
def stratified_mask(G, P, cap, rnd):
    """[G][P] bool: group g keeps the positions perm[(rnd G n + g n + j) mod P], j < n = min(cap, P): at most cap per group, and the union over the groups (and
    over rounds_of(G, P, cap) rounds) is every position"""
    n = min(cap, P)
    perm = torch.randperm(P, generator=_gen(P, 17))
    start = rnd * G * n + torch.arange(G) * n
    idx = (start[:, None] + torch.arange(n)[None, :]) % P
    mask = torch.zeros(G, P, dtype=torch.bool)
    mask.scatter_(1, perm[idx], True)
    return mask


def rounds_of(G, P, cap):
    return -(-P // (G * min(cap, P)))


def rotating_mask(M, Cn, m, rnd):
    """[M][Cn] bool: pixel p keeps the m channels (rnd M m + p m + j) mod Cn"""
    if m >= Cn:
        return torch.ones(M, Cn, dtype=torch.bool)
    start = ((torch.arange(M, dtype=torch.int64) + rnd * M) * m % Cn).to(torch.int16)
    diff = torch.arange(Cn, dtype=torch.int16)[None, :] - start[:, None]
    return torch.remainder(diff, Cn) < m


def per_pixel(k):
    return max(CAP // (k * k), 1)


def rounds_fwd(case, arr):
    N, H, W, C, K, k, s, d = case
    return rounds_of(K, k * k * C, CAP) if arr == 'A' else rounds_of(N * H * W, C, per_pixel(k))


def rounds_dgrad(case, arr):
    N, H, W, C, K, k, s, d = case
    return rounds_of(C, K * k * k, CAP) if arr == 'A' else rounds_of(N * same_out(H, s) * same_out(W, s), K, per_pixel(k))


def filter_fwd_A(case, rnd):
    N, H, W, C, K, k, s, d = case
    m = stratified_mask(K, k * k * C, CAP, rnd)
    return (m * _signs(m.shape, _gen(*case, rnd, 1))).reshape(K, k, k, C)


def filter_dgrad_A(case, rnd):
    N, H, W, C, K, k, s, d = case
    m = stratified_mask(C, K * k * k, CAP, rnd)
    w = m * _signs(m.shape, _gen(*case, rnd, 2))
    return w.reshape(C, K, k, k).permute(1, 2, 3, 0).contiguous()


def dense(shape, case, tag):
    return _signs(shape, _gen(*case, tag))


def sparse_act(N, H, W, Cn, k, case, rnd, tag):
    m = rotating_mask(N * H * W, Cn, per_pixel(k), rnd)
    return (m * _signs(m.shape, _gen(*case, rnd, tag))).reshape(N, H, W, Cn)


# ------------------------------------------------------------------------------------------------------------ reference
def ref_conv(x_nhwc, w_krsc, b, stride, dil):
    return R.conv2d_same(x_nhwc.permute(0, 3, 1, 2), w_krsc, b, stride, dil).permute(0, 2, 3, 1)


def rows(t_nhwc, ld, dtype=torch.bfloat16):
    """[N][H][W][C] -> [N H W][ld] with zero pad columns (bf16 holds every value here exactly and halves the cache)"""
    Cn = t_nhwc.shape[-1]
    out = torch.zeros(t_nhwc.numel() // Cn, ld, dtype=dtype)
    out[:, :Cn] = t_nhwc.reshape(-1, Cn).to(dtype)
    return out


def pad_filter(w, ldx):
    out = torch.zeros(*w.shape[:3], ldx, dtype=torch.float32)
    out[..., : w.shape[3]] = w.float()
    return out


def _absmax(t):
    return float(t.detach().abs().max()) if t.numel() else 0.0


def forward_operands(case, arr, rnd=0, dtype=torch.float32):
    """x, w, bias, z = conv + bias (before the ReLU) as NHWC / KRSC tensors of `dtype`; asserts |z| <= 256"""
    N, H, W, C, K, k, s, d = case
    if arr == 'A':
        x, w = dense((N, H, W, C), case, 3), filter_fwd_A(case, rnd)
    else:
        x, w = sparse_act(N, H, W, C, k, case, rnd, 4), dense((K, k, k, C), case, 5)
    b = torch.randint(-3, 4, (K,), generator=_gen(*case, 6)).float()
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    z = ref_conv(x, w, b, s, d)
    assert _absmax(z) <= BF16_EXACT, ('forward: result not exactly representable in bf16', case, arr, _absmax(z))
    return x, w, b, z


def dgrad_operands(case, arr, rnd=0, dtype=torch.float32):
    """dy, w, ReLU-mask source, prev, dx = the input gradient, dx2 = (dx + prev) where src > 0; asserts |dx|, |dx + prev| <= 256"""
    N, H, W, C, K, k, s, d = case
    Ho, Wo = same_out(H, s), same_out(W, s)
    if arr == 'A':
        dy, w = dense((N, Ho, Wo, K), case, 7), filter_dgrad_A(case, rnd)
    else:
        dy, w = sparse_act(N, Ho, Wo, K, k, case, rnd, 8), dense((K, k, k, C), case, 9)
    dy, w = dy.to(dtype), w.to(dtype)
    x0 = torch.zeros(N, H, W, C, dtype=dtype, requires_grad=True)
    dx, = torch.autograd.grad(ref_conv(x0, w, None, s, d), x0, dy)
    src = dense((N, H, W, C), case, 10).to(dtype)
    prev = torch.randint(-2, 3, (N, H, W, C), generator=_gen(*case, 11)).to(dtype)
    dx2 = (dx + prev) * (src > 0)
    assert _absmax(dx) <= BF16_EXACT and _absmax(dx + prev) <= BF16_EXACT, ('input gradient: result not exactly representable in bf16', case, arr, _absmax(dx))
    return dy, w, src, prev, dx, dx2


def wgrad_operands(case, bounded=False, dtype=torch.float32, x=None):
    """x, dy, dw, dbias; asserts 2 |dw|, 2 |dbias| < 2^24 (the tests call the accumulating entry point twice)"""
    N, H, W, C, K, k, s, d = case
    Ho, Wo = same_out(H, s), same_out(W, s)
    if x is None:
        x = dense((N, H, W, C), case, 3).to(dtype)
    dy = (sparse_act(N, Ho, Wo, K, k, case, 0, 12) if bounded else dense((N, Ho, Wo, K), case, 13)).to(dtype)
    w0 = torch.zeros(K, k, k, C, dtype=dtype, requires_grad=True)
    dw, = torch.autograd.grad(ref_conv(x, w0, None, s, d), w0, dy)
    db = dy.reshape(-1, K).sum(0)
    assert 2 * _absmax(dw) < F32_EXACT and 2 * _absmax(db) < F32_EXACT, ('filter gradient: sums not exact in f32', case)
    if bounded:
        assert _absmax(dy.abs().reshape(-1, K).sum(1)) <= per_pixel(k)
    return x, dy, dw, db


# ------------------------------------------------------------------------------------------------------------ cached row-form references
_CACHE = collections.OrderedDict()
_CACHE_BYTES = 3 << 30


def _cached(key, make):
    if key in _CACHE:
        _CACHE.move_to_end(key)
        return _CACHE[key]
    val = make()
    _CACHE[key] = val
    size = lambda v: sum(t.numel() * t.element_size() for t in v.values() if torch.is_tensor(t))
    total = sum(size(v) for v in _CACHE.values())
    while total > _CACHE_BYTES and len(_CACHE) > 1:
        _, old = _CACHE.popitem(last=False)
        total -= size(old)
    return val


def forward_case(case, arr, rnd, ldx, Kp):
    """rows-form forward case (+ for arrangement A the filter gradient of the same x against a dense dy): x [M_in][ldx], w [K][k][k][ldx] f32, b [K],
    y [M_out][Kp] = relu(conv + bias), dy [M_out][Kp], dw [K][k][k][ldx] f32, db [K]"""
    def make():
        x, w, b, z = forward_operands(case, arr, rnd)
        out = dict(x=rows(x, ldx), w=pad_filter(w, ldx), b=b, y=rows(torch.relu(z), Kp), shape_in=x.shape[:3], shape_out=z.shape[:3])
        if arr == 'A' and rnd == 0:
            _, dy, dw, db = wgrad_operands(case, x=x)
            out.update(dy=rows(dy, Kp), dw=pad_filter(dw, ldx), db=db)
        return out
    return _cached(('fwd', case, arr, rnd, ldx, Kp), make)


def dgrad_case(case, arr, rnd, ldx, Kp):
    def make():
        dy, w, src, prev, dx, dx2 = dgrad_operands(case, arr, rnd)
        return dict(dy=rows(dy, Kp), w=pad_filter(w, ldx), src=rows(src, ldx), prev=rows(prev, ldx), dx=rows(dx, ldx), dx2=rows(dx2, ldx),
                    shape_in=dx.shape[:3], shape_out=dy.shape[:3])
    return _cached(('dgrad', case, arr, rnd, ldx, Kp), make)


def pool2x2_ref(y_rows, shape, K):
    """tf.layers.max_pooling2d(2, 2, 'same') of a rows-form map: [N Hp Wp][ld] (pad columns zero)"""
    N, H, W = shape
    Hp, Wp = (H + 1) // 2, (W + 1) // 2
    v = y_rows[:, :K].float().reshape(N, H, W, K).permute(0, 3, 1, 2)
    p = F.max_pool2d(F.pad(v, (0, 2 * Wp - W, 0, 2 * Hp - H), value=float('-inf')), 2, 2).permute(0, 2, 3, 1)
    return rows(p, y_rows.shape[1]), (N, Hp, Wp)


# ------------------------------------------------------------------------------------------------------------ guard bands
class Guarded:
    """a device operand as a view into a larger allocation: GUARD_ROWS rows of `fill` in front of it and behind it.  Nothing here leaves the allocation."""

    def __init__(self, inner_cpu, dtype, dev, fill):
        inner = inner_cpu.reshape(inner_cpu.shape[0], -1) if inner_cpu.dim() > 1 else inner_cpu.reshape(-1, 1)
        self.M, self.ld = inner.shape
        self.g = GUARD_ROWS if inner_cpu.dim() > 1 else GUARD_ROWS * 8            # flat arrays (filters, bias): 4 096 elements
        self.fill = fill
        self.whole = torch.full((self.M + 2 * self.g, self.ld), fill, dtype=dtype, device=dev)
        self.view = self.whole[self.g: self.g + self.M]
        self.view.copy_(inner.to(dtype))
        if inner_cpu.dim() == 1:
            self.view = self.view.reshape(-1)
        elif inner_cpu.dim() > 2:
            self.view = self.view.reshape(inner_cpu.shape)

    def guards_intact(self):
        return bool((self.whole[: self.g] == self.fill).all()) and bool((self.whole[self.g + self.M:] == self.fill).all())

    def first_guard_damage(self):
        w = self.whole.float().cpu()
        w[self.g: self.g + self.M] = self.fill
        bad = (w != self.fill).nonzero()
        return [(int(r) - self.g, int(c), float(w[r, c])) for r, c in bad[:6]], int(bad.shape[0])


def describe_mismatch(got, exp, shape):
    """number of differing elements and the first few (n, h, w, channel) with got / expected"""
    N, H, W = shape
    bad = (got != exp).nonzero()
    first = []
    for r, c in bad[:8].tolist():
        first.append(((r // (H * W), r // W % H, r % W, c), float(got[r, c]), float(exp[r, c])))
    return f'{bad.shape[0]} of {got.numel()} elements differ; first (n, h, w, channel) got expected: {first}'
