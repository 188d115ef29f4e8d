"""Soft-NMS (odtk_soft_nms_image_class, odtk_detection_pack_scored): the NumPy oracle and the kernel-level case bodies shared by tests/test_gpu_soft_nms.py
(libodtk.so on the device) and tests/test_cpu_soft_nms.py (csrc/soft_nms.hip compiled from source under the fiber emulation, tests/hip_cpu_backend.py).

The oracle restates the loop of include/odtk.h.  One problem = n rows with a score, a box and a `valid` flag; a row is live when it is valid and its score is
above -inf (NaN excluded).  Until max_out picks: m = the live row with the largest current score (lower row on equal scores); emit (m, s_m); m leaves; every
live j is decayed with iou = IoU(b_m, b_j):  hard: dead if iou > thr;  linear: s_j *= (1 - iou) if iou > thr;  gaussian: s_j *= exp(-(iou * iou) / sigma);
with linear and gaussian j is dead when its score is then not >= min_score.
  * dtype = np.float32: every operation in float32 in the order written (NumPy's float32 +, -, *, / are correctly rounded, as the device's are with
    contraction off); exp is evaluated in float64 and rounded to float32, i.e. correctly rounded;
  * dtype = np.float64: the same loop, used for the preconditions of the Gaussian comparison only (`stats`).

Gaussian bound (derived, not measured): IoU, its square and the quotient by sigma are the same float32 operations on both sides, hence bit-equal; the device's
expf is documented at 1 ulp against the oracle's correctly rounded value (half an ulp of its own): their quotient is within 1.5 * 2^-23; each decay adds one
product rounding on either side, 2^-24 each, and carries the relative error of the score before.  After k decays: at most k * (1.5 + 1) * 2^-23 < 3 k 2^-23
relative.  Position 0 of a problem has seen no decay and is exact."""
import numpy as np
import torch

BAND = 4096
FILL = {torch.float32: 1357.0, torch.int32: -13579}
ULP = 2.0 ** -23


class Banded:
    """an output operand between two bands of sentinels (the pattern of refinedet_wide_cases / edge_gt_cases)"""

    def __init__(self, shape, dev, dtype=torch.float32, init=-7):
        self.n = int(np.prod(shape))
        self.fill = FILL[dtype]
        self.whole = torch.full((self.n + 2 * BAND,), self.fill, dtype=dtype, device=dev)
        self.t = self.whole[BAND: BAND + self.n].view(*shape)
        self.t.fill_(init)

    def intact(self):
        return bool((self.whole[:BAND] == self.fill).all()) and bool((self.whole[BAND + self.n:] == self.fill).all())


def _ops():
    import odtk  # noqa: F401
    from odtk import ops
    return ops


# ------------------------------------------------------------------------------------------------------------------ oracle
def soft_nms_ref(boxes, scores, valid, max_out, method, thr, sigma=0.5, min_score=0.0, dtype=np.float32):
    """-> (picks [k] int, their emitted scores [k] dtype, stats).  method 0 hard, 1 linear, 2 gaussian.  stats: `decayed` (live scores changed by a decay),
    `killed` (rows that died by min_score), `gap` (smallest relative distance between the best and the runner-up live score at a pick), `margin` (smallest
    relative distance of a decayed score from min_score)."""
    F = dtype
    b = np.asarray(boxes).astype(F)
    thr, sigma, min_score = F(np.float32(thr)), F(np.float32(sigma)), F(np.float32(min_score))
    ymin, xmin = np.minimum(b[:, 0], b[:, 2]), np.minimum(b[:, 1], b[:, 3])
    ymax, xmax = np.maximum(b[:, 0], b[:, 2]), np.maximum(b[:, 1], b[:, 3])
    area = (ymax - ymin) * (xmax - xmin)
    s = np.asarray(scores).astype(F).copy()
    with np.errstate(invalid='ignore'):
        live = np.asarray(valid, dtype=bool) & (s > -np.inf)
    picks, out = [], []
    stats = dict(decayed=0, killed=0, gap=np.inf, margin=np.inf)
    while len(picks) < max_out and live.any():
        cur = np.where(live, s, -np.inf)
        m = int(np.argmax(cur))                                   # the first maximum: the lower row on equal scores
        if live.sum() > 1:
            second = np.partition(cur, -2)[-2]
            stats['gap'] = min(stats['gap'], float(abs(cur[m] - second) / max(abs(cur[m]), 1e-30)))
        picks.append(m)
        out.append(s[m])
        live[m] = False
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            ih = np.maximum(np.minimum(ymax[m], ymax) - np.maximum(ymin[m], ymin), F(0))
            iw = np.maximum(np.minimum(xmax[m], xmax) - np.maximum(xmin[m], xmin), F(0))
            inter = ih * iw
            iou = inter / (area[m] + area - inter)
            iou = np.where((area[m] <= 0) | (area <= 0), F(0), iou).astype(F)
            if method == 0:
                live &= ~(iou > thr)
                continue
            if method == 1:
                hit = live & (iou > thr)
                new = np.where(hit, s * (F(1) - iou), s).astype(F)
            else:
                hit = live.copy()
                e = np.exp((-(iou * iou) / sigma).astype(np.float64)).astype(F)
                new = np.where(hit, s * e, s).astype(F)
            stats['decayed'] += int((hit & (new != s)).sum())
            if hit.any() and min_score > 0:
                stats['margin'] = min(stats['margin'], float((np.abs(new[hit] - min_score) / min_score).min()))
            s = new
            dead = live & ~(s >= min_score)
            stats['killed'] += int(dead.sum())
            live &= ~dead
    return np.asarray(picks, dtype=np.int64), np.asarray(out, dtype=F), stats


def reference_tables(boxes, scores, valid, n_lim, nc, max_out, method, thr, sigma, min_score, dtype=np.float32):
    """the oracle over [N][n] images x nc classes: boxes [N, n, 4], scores / valid [N, n, ld] (numpy) -> list over (img, c) of (picks, scores, stats)"""
    N, n = boxes.shape[:2]
    res = []
    for img in range(N):
        lim = n if n_lim is None else min(n, max(int(n_lim[img]), 0))
        for c in range(nc):
            v = valid[img, :lim, c] == 1 if valid is not None else np.ones(lim, dtype=bool)
            res.append(soft_nms_ref(boxes[img, :lim], scores[img, :lim, c], v, max_out, method, thr, sigma, min_score, dtype))
    return res


# ------------------------------------------------------------------------------------------------------------------ inputs and launches
def random_problem(seed, N, nc, n, density, ld=None, size=(8.0, 30.0), canvas=100.0, special=True):
    """boxes [N, n, 4] (corners in any order, on a canvas small enough for many overlaps), scores [N, n, ld] in (0.05, 1), valid u8 [N, n, ld] with
    valid[..., c] = 1 with probability density[c]; ld = nc + 1 (a stride that is not the class count; the last column is never a class).  special: a few NaN
    and -inf scores on valid rows (never live)"""
    ld = nc + 1 if ld is None else ld
    g = np.random.default_rng(seed)
    ctr = g.uniform(0, canvas, (N, n, 2)).astype(np.float32)
    hw = g.uniform(size[0], size[1], (N, n, 2)).astype(np.float32)
    lo, hi = ctr - hw / 2, ctr + hw / 2
    boxes = np.concatenate([lo, hi], 2).astype(np.float32)
    flip = g.random((N, n)) < 0.3                                     # corners the other way round: the kernel normalises
    boxes[flip] = boxes[flip][:, [2, 3, 0, 1]]
    scores = g.uniform(0.05, 1.0, (N, n, ld)).astype(np.float32)
    valid = (g.random((N, n, ld)) < np.asarray(list(density) + [1.0] * (ld - nc))[None, None, :]).astype(np.uint8)
    if special and n >= 63:
        scores[0, 5, 0] = np.nan; valid[0, 5, 0] = 1
        scores[N - 1, 7, nc - 1] = -np.inf; valid[N - 1, 7, nc - 1] = 1
    return boxes, scores, valid


class Launch:
    """one call of odtk_soft_nms_image_class (or of odtk_nms_image_class with method=None) on host arrays; outputs between sentinel bands"""

    def __init__(self, dev, boxes, scores, valid, nc, max_out, cap, method, thr, sigma=0.5, min_score=0.0, n_lim=None):
        ops = _ops()
        N, n, ld = scores.shape
        self.bx, self.sc = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
        self.vd = torch.from_numpy(valid).to(dev)
        self.lim = None if n_lim is None else torch.tensor(list(n_lim), dtype=torch.int32).to(dev)
        self.idx = Banded((N, nc, cap), dev, torch.int32)
        self.cnt = Banded((N, nc), dev, torch.int32)
        self.score = Banded((N, nc, cap), dev)
        operands = (self.bx, n * 4, self.sc, n * ld, 1, ld, self.vd, n * ld, 1, ld, 1, n, self.lim, N, nc, max_out)
        if method is None:
            ops.nms_image_class(*operands, thr, self.idx.t, cap, self.cnt.t)
        else:
            ops.soft_nms_image_class(*operands, method, thr, sigma, min_score, self.idx.t, self.score.t, cap, self.cnt.t)
        if torch.device(dev).type == 'cuda':
            torch.cuda.synchronize()
        assert self.idx.intact() and self.cnt.intact() and self.score.intact(), 'a sentinel band was written'

    def tables(self):
        return self.idx.t.cpu().numpy(), self.cnt.t.cpu().numpy(), self.score.t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ 1: hard == the existing kernel
# n just above the one internal capacity (2048 live rows kept compacted in LDS; class 0 has every row valid and takes the slow path, the sparse classes the
# compacted one), and n = 32768 with sparse `valid` (class 0 dense enough for the slow path at the full 128 KiB of scores)
HARD_SHAPES = {1: (1.0, 1.0, 1.0, 0.0), 63: (1.0, 0.5, 0.1, 0.0), 65: (1.0, 0.5, 0.1, 0.0), 1025: (1.0, 0.5, 0.02, 0.0), 2049: (1.0, 0.5, 0.02, 0.0),
               32768: (0.3, 0.01, 0.001, 0.0)}


def check_hard(dev, n, with_n_dev):
    N, nc, max_out, cap, thr = 3, 4, 10, 12, 0.5
    boxes, scores, valid = random_problem(100 + n, N, nc, n, HARD_SHAPES[n])
    n_lim = [n, n // 2, 0] if with_n_dev else None
    if with_n_dev and n == 1:
        n_lim = [1, 5, 0]
    want = Launch(dev, boxes, scores, valid, nc, max_out, cap, None, thr, n_lim=n_lim)
    got = Launch(dev, boxes, scores, valid, nc, max_out, cap, 0, thr, n_lim=n_lim)
    assert torch.equal(got.cnt.t, want.cnt.t), (n, got.cnt.t.tolist(), want.cnt.t.tolist())
    idx, cnt, sc = got.tables()
    widx = want.idx.t.cpu().numpy()
    total = 0
    for img in range(N):
        for c in range(nc):
            k = int(cnt[img, c])
            total += k
            assert np.array_equal(idx[img, c, :k], widx[img, c, :k]), (n, img, c)
            assert np.array_equal(sc[img, c, :k], scores[img, idx[img, c, :k], c]), (n, img, c)          # the ORIGINAL scores of the picks
            assert (idx[img, c, k:] == -7).all() and (sc[img, c, k:] == -7).all(), (n, img, c)             # slots behind the count are not written
    assert total > 0 and (cnt[:, nc - 1] == 0).all()
    if n >= 63 and not with_n_dev:
        assert cnt.max() == max_out
    if with_n_dev:
        assert (cnt[2] == 0).all()
    return cnt


# ------------------------------------------------------------------------------------------------------------------ 2: linear == the f32 oracle, bit for bit
def linear_case(n):
    """N = 2, 3 classes, n rows: random rows plus hand-planted ones -- (a) two identical boxes with equal scores (rows 3 < 9, the best of their class: 9 is
    decayed to 0 and dies), (b) two far-apart boxes with equal scores (rows 20 < 41: both picked, 20 first), (c) a zero-area box with a high score (row 30:
    IoU 0 with everything, never decayed), (d) image 1, class 2 without a valid row, (e) about 65 valid rows in class 1 wherever they fall among the n: enough to reach max_out"""
    N, nc = 2, 3
    boxes, scores, valid = random_problem(7 + n, N, nc, n, tuple(min(1.0, d * 65 / n) for d in (0.5, 1.0, 0.3)), size=(20.0, 40.0), canvas=120.0, special=False)
    scores *= np.float32(0.9)                                                                            # the planted scores are the best of their class
    boxes[0, 3] = boxes[0, 9] = (10.0, 10.0, 40.0, 40.0)
    scores[0, 3, 0] = scores[0, 9, 0] = 0.99
    boxes[0, 20], boxes[0, 41] = (500.0, 500.0, 520.0, 520.0), (700.0, 700.0, 720.0, 720.0)
    scores[0, 20, 0] = scores[0, 41, 0] = 0.97
    boxes[0, 30] = (60.0, 60.0, 60.0, 90.0)
    scores[0, 30, 0] = 0.98
    valid[0, [3, 9, 20, 41, 30], 0] = 1
    valid[1, :, 2] = 0
    return boxes, scores, valid


def check_linear(dev, n):
    N, nc, max_out, cap, thr, min_score = 2, 3, 12, 12, 0.3, 0.25
    boxes, scores, valid = linear_case(n)
    got = Launch(dev, boxes, scores, valid, nc, max_out, cap, 1, thr, min_score=min_score)
    idx, cnt, sc = got.tables()
    ref = reference_tables(boxes, scores, valid, None, nc, max_out, 1, thr, 0.5, min_score)
    decayed_picks = 0
    for p, (picks, want, _) in enumerate(ref):
        img, c = divmod(p, nc)
        k = len(picks)
        assert int(cnt[img, c]) == k, (n, img, c, int(cnt[img, c]), k)
        assert np.array_equal(idx[img, c, :k], picks), (n, img, c)
        assert np.array_equal(sc[img, c, :k].view(np.uint32), want.view(np.uint32)), (n, img, c)            # bit patterns
        assert (idx[img, c, k:] == -7).all() and (sc[img, c, k:] == -7).all()
        decayed_picks += int((want != scores[img, picks, c]).sum())
    # the case is what it claims to be
    p00 = ref[0][0].tolist()
    assert p00[0] == 3 and 9 not in p00                                                                  # (a) lower row first; its twin decayed to 0, dead
    assert p00[1] == 30 and ref[0][1][1] == np.float32(0.98)                                             # (c) zero area: undecayed
    assert p00.index(20) + 1 == p00.index(41) and ref[0][1][p00.index(41)] == np.float32(0.97)           # (b) equal scores: the lower row first
    assert len(ref[1 * nc + 2][0]) == 0 and valid[1, :, 2].sum() == 0                                    # (d)
    assert any(len(r[0]) == max_out for r in ref)                                                        # (e)
    assert decayed_picks > 0 and sum(r[2]['killed'] for r in ref) > 0
    return cnt


# ------------------------------------------------------------------------------------------------------------------ 3: gaussian against the f32 oracle
GAUSS_MIN_SCORE, GAUSS_THR, GAUSS_MAX_OUT = 0.1, 0.5, 20
GAUSS_SEEDS = {(65, 0.5): 1, (65, 0.1): 1, (1025, 0.5): 1, (1025, 0.1): 0}         # checked on the CPU (find_gauss_seed): the preconditions hold


def gauss_case(n, sigma, seed):
    """N = 2, 3 classes; about 14 valid rows per problem anywhere among the n rows, log-uniform scores, boxes on a small canvas (most pairs overlap)"""
    N, nc = 2, 3
    boxes, scores, valid = random_problem(seed, N, nc, n, (14.0 / n,) * 3, size=(20.0, 40.0), canvas=60.0, special=False)
    g = np.random.default_rng(seed + 1)
    scores[...] = np.exp(g.uniform(np.log(0.15), 0.0, scores.shape)).astype(np.float32)
    valid[:, n - 1, 0] = 1                                                                                # the last row is in play
    return boxes, scores, valid


def gauss_preconditions(n, sigma, seed):
    """float64 oracle: at every pick the best and the runner-up differ by >= 1e-3 relative; no decayed score within 1e-3 relative of min_score"""
    boxes, scores, valid = gauss_case(n, sigma, seed)
    ref = reference_tables(boxes, scores, valid, None, 3, GAUSS_MAX_OUT, 2, GAUSS_THR, sigma, GAUSS_MIN_SCORE, np.float64)
    gap, margin = min(r[2]['gap'] for r in ref), min(r[2]['margin'] for r in ref)
    return gap >= 1e-3 and margin >= 1e-3, gap, margin, sum(len(r[0]) for r in ref)


def find_gauss_seed(n, sigma, start=0):
    seed = start
    while not gauss_preconditions(n, sigma, seed)[0]:
        seed += 1
    return seed


def compare_gaussian(got_scores, want_scores):
    """rule 3: position k of a problem within 3 k 2^-23 relative, position 0 exact -> the largest error seen in ulp (2^-23 relative) per decay"""
    worst = 0.0
    for k, (g, w) in enumerate(zip(got_scores, want_scores)):
        g, w = float(g), float(w)
        assert abs(g - w) <= 3 * k * ULP * w, (k, g, w, abs(g - w) / (ULP * w))
        if k:
            worst = max(worst, abs(g - w) / (ULP * w) / k)
    return worst


def check_gaussian(dev, n, sigma):
    N, nc, cap = 2, 3, GAUSS_MAX_OUT
    seed = GAUSS_SEEDS[(n, sigma)]
    ok, gap, margin, npicks = gauss_preconditions(n, sigma, seed)
    assert ok, (n, sigma, seed, gap, margin)                                                             # never skipped
    boxes, scores, valid = gauss_case(n, sigma, seed)
    got = Launch(dev, boxes, scores, valid, nc, GAUSS_MAX_OUT, cap, 2, GAUSS_THR, sigma, GAUSS_MIN_SCORE)
    idx, cnt, sc = got.tables()
    ref = reference_tables(boxes, scores, valid, None, nc, GAUSS_MAX_OUT, 2, GAUSS_THR, sigma, GAUSS_MIN_SCORE)
    worst, deep = 0.0, 0
    for p, (picks, want, _) in enumerate(ref):
        img, c = divmod(p, nc)
        k = len(picks)
        assert int(cnt[img, c]) == k and np.array_equal(idx[img, c, :k], picks), (n, sigma, img, c)
        worst = max(worst, compare_gaussian(sc[img, c, :k], want))
        deep = max(deep, k)
    assert deep >= 4 and sum(r[2]['decayed'] for r in ref) > 0 and npicks == int(cnt.sum())
    print(f'gaussian n={n} sigma={sigma} seed={seed}: {npicks} picks, deepest problem {deep}, gap {gap:.2e}, margin {margin:.2e}, '
          f'largest error {worst:.3f} ulp per decay (bound 3)')
    return worst


# ------------------------------------------------------------------------------------------------------------------ 4: refusals
def check_refusals(dev):
    ops = _ops()
    N, nc, n, cap = 2, 3, 16, 4
    bx = torch.zeros(N, n, 4, device=dev); sc = torch.zeros(N, n, nc, device=dev); vd = torch.ones(N, n, nc, dtype=torch.uint8, device=dev)
    idx = torch.zeros(N, nc, cap, dtype=torch.int32, device=dev); cnt = torch.zeros(N, nc, dtype=torch.int32, device=dev); out = torch.zeros(N, nc, cap, device=dev)

    def call(boxes=bx, scores=sc, n=n, N=N, nc=nc, method=1, sigma=0.5, out_idx=idx, out_score=out, cap=cap, out_cnt=cnt):
        ops.soft_nms_image_class(boxes, n * 4, scores, n * nc, 1, nc, vd, n * nc, 1, nc, 1, n, None, N, nc, 3, method, 0.5, sigma, 0.0, out_idx, out_score, cap,
                                 out_cnt)
    call()                                                                                               # the good call goes through
    bad = [dict(boxes=None), dict(scores=None), dict(out_idx=None), dict(out_score=None), dict(out_cnt=None), dict(method=-1), dict(method=3),
           dict(method=2, sigma=0.0), dict(method=2, sigma=-1.0), dict(n=0), dict(n=32769), dict(N=0), dict(N=21846, nc=3), dict(cap=0)]
    for kw in bad:
        try:
            call(**kw)
        except Exception as e:                                   # noqa: BLE001 -- the library's error type
            assert 'soft_nms_image_class:' in str(e), (kw, str(e))
        else:
            raise AssertionError(f'accepted: {kw}')
    call(method=1, sigma=0.0)                                                                            # sigma is the Gaussian method's alone
    return len(bad)


# ------------------------------------------------------------------------------------------------------------------ 5: detection_pack_scored
def check_pack_scored(dev):
    ops = _ops()
    N, nc, cap, n = 3, 4, 5, 50
    g = torch.Generator().manual_seed(1)
    conf = torch.rand(N, n, nc, generator=g).to(dev); boxes = torch.rand(N, n, 4, generator=g).to(dev)
    cnt = torch.tensor([[2, 0, 5, 1], [0, 0, 0, 0], [3, 3, 0, 4]], dtype=torch.int32).to(dev)
    idx = torch.randint(0, n, (N, nc, cap), generator=g).to(torch.int32).to(dev)
    table = torch.rand(N, nc, cap, generator=g).to(dev)
    K = N * nc * cap
    outs = []
    for scored in (False, True):
        o = dict(counts=Banded((N,), dev, torch.int32), offsets=Banded((N + 1,), dev, torch.int32), scores=Banded((K,), dev), bbox=Banded((K, 4), dev),
                 cid=Banded((K,), dev, torch.int32))
        args = (conf, boxes, o['counts'].t, o['offsets'].t, o['scores'].t, o['bbox'].t, o['cid'].t)
        if scored:
            ops.detection_pack_scored(idx, cnt, table, *args)
        else:
            ops.detection_pack(idx, cnt, *args)
        assert all(b.intact() for b in o.values())
        outs.append(o)
    plain, scored = outs
    for k in ('counts', 'offsets', 'bbox', 'cid'):
        assert torch.equal(plain[k].t, scored[k].t), k
    assert scored['offsets'].t.tolist() == [0, 8, 8, 18]
    want = torch.cat([table[i, c, : int(cnt[i, c])] for i in range(N) for c in range(nc)])
    assert torch.equal(scored['scores'].t[:18], want) and bool((scored['scores'].t[18:] == -7).all())
    assert not torch.equal(plain['scores'].t[:18], want)


# ------------------------------------------------------------------------------------------------------------------ model level: the oracle on a tail's operands
def tail_reference(conf, boxes, cand, max_boxes, method, thr, sigma, min_score):
    """conf [A, >= nc], boxes [A, 4], cand [A, nc] (numpy) of ONE image -> [scores, bbox, class_id, position of each row in its problem] in the tail's order
    (ascending class, pick order) from the f32 oracle"""
    s, b, c, pos = [], [], [], []
    for k in range(cand.shape[1]):
        picks, sc, _ = soft_nms_ref(boxes, conf[:, k], cand[:, k] != 0, max_boxes, method, thr, sigma, min_score)
        s.append(sc); b.append(boxes[picks]); c.append(np.full(len(picks), k, dtype=np.int32)); pos.append(np.arange(len(picks)))
    return [np.concatenate(s).astype(np.float32), np.concatenate(b, 0).reshape(-1, 4), np.concatenate(c), np.concatenate(pos)]


def compare_detections(got, want, method):
    """classes and boxes equal; scores: rule 2 (linear: bit for bit) or rule 3 (gaussian: 3 k 2^-23 relative at position k)"""
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]), (got[2].tolist(), want[2].tolist())
    if method == 'gaussian':
        for g, w, k in zip(got[0], want[0], want[3]):
            assert abs(float(g) - float(w)) <= 3 * int(k) * ULP * float(w), (k, g, w)
    else:
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
