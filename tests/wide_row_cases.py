"""Case bodies shared by tests/test_cpu_wide_rows.py (the kernels from source under the fiber emulation) and tests/test_gpu_wide_rows.py (libodtk.so through the
C-ABI): rows of 33 .. 256 logits through odtk_ssd_loss, odtk_ssd_decode, odtk_retina_decode, odtk_ssd_decode_batched, odtk_retina_decode_batched,
odtk_retina_loss and 65 .. 256 classes through odtk_fcos_loss, against the float64 restatements below.

Shapes: N = 2 images, P = 8 ground-truth rows, A = 301 rows (no multiple of the 16 / 32 / 64 / 128 rows a workgroup or tile takes), row pitch C + 9 with
PAD_VALUE in the pad columns.  Image 0 has 5 boxes with the labels C - 2 (the last object class), 0, 17, min(33, C - 3) (a lane's third slot), C - 2; image 1 has none.
Row 0 of every logit tensor is +-80 (one class at +80, the others at -80), row 1 the same with the background class high.

Integers (keep, cand and, through them, the arg-max) must be EQUAL to the restatement.  That is a fair demand because the cases assert, on the float64 side,
that the two largest logits of every row differ by at least 2^-10 and that no confidence lies within its bound of the score threshold.

Floats are held to bounds derived from the kernels' own arithmetic, evaluated per element in float64 from the element's own row (u = 2^-24, one f32 rounding;
a 3-ulp expf / logf is within 6 u relative and powf within 16 ulp = 32 u -- the OpenCL full-profile bounds the ROCm device library is written to; glibc on
the CPU tier is within 1 ulp; TINY = 2^-126 covers results below the normal range, which carry no relative precision):
  softmax.  d_c = z_c - m is one rounding, so exp sees d_c (1 + e): the term is off by |d_c| u relative, expf adds 6 u.  The sum is K - 1 sequential adds in a
      lane (K = 4, 8, 16 register slots for C <= 64, 128, 256: wide_row.h) and 4 butterfly steps, one more u taken for the second-order terms:
      S' = S (1 + rS), rS = (6 + D + K + 4) u, D = sum |d_j| e^d_j / S (at C = 32, the limit of the one-thread kernels: 31 sequential adds, 6 + D + 32).  p_c = e_c / S is one more rounding: rp_c = (|d_c| + 6) u + rS + u.
  boxes.  cy = fl(fl(t0 ah) + ay), h = fl(ah expf(t2)) (7 u), y1 = fl(cy - h / 2): u (|t0 ah| + |cy| + 3.5 h + |y1|), and the same for the three others.
  cross entropy of a row.  logf(S') = log S + rS, 6 u |log S| of its own; z_l - m one rounding; the difference one more.
  smooth L1 of a row.  t = (g - a) / h two roundings (log(g / h): u from the quotient, 6 u |t| from logf), d = z - t one more; |f'| <= min(|d|, 1), f itself two
      roundings, the four terms three adds.
  sums over rows.  Every sum of n values through lanes, waves, workgroups and a final loop is held to (n + 48) u times the sum of the absolute values on top
      of the values' own bounds: no path through the kernels adds more than n + 48 times (at most n in a lane, 6 butterfly steps, 4 waves, 32 workgroups of
      the SSD split or the workgroups of a RetinaNet image, which the cases keep below 32, and the final additions).
  gradients.  (p_c - y) gsc: bp_c gsc, the subtraction, the product and the two roundings in gsc = grad_scale / count: 4 u |g|; a row visited twice (a best
      anchor of two boxes) adds the two bounds and one u of the sum.
  focal term.  loss and the factor k = dpt pu scale are functions of pu = p_label alone: their bound is the change of the float64 function over
      pu (1 +- rp) plus the roundings of evaluating it (two powf, logf, a quotient and six products: 80 u).
  FCOS.  sigmoid and log-sigmoid of a logit k are a few operations around one expf / log1pf: 12 u relative each; -k + log_sigmoid(k) cancels for k < 0:
      u (|k| + |ls|) absolute.  The heat-map sum of a location is C sequential adds.  The box and centre-ness gradients do not depend on C: above 64 classes
      they must EQUAL those of the one-word kernel on the first 64 classes."""
import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
PAD_VALUE = 1e30
N, P, A = 2, 8, 301
CLASSES = [33, 64, 65, 81, 255, 256]            # one past each old limit, counts that are no multiple of the group width, the cap
GAP = 2.0 ** -10


NARROW = 32                                     # up to here the one-thread-per-row kernels run: the sum of exponentials is C - 1 sequential adds


def slots(C):
    return 4 if C <= 64 else (8 if C <= 128 else 16)


def sum_adds(C):
    """additions on the longest path of the sum of exponentials"""
    return C - 1 if C <= NARROW else slots(C) - 1 + 4


def _sync(dev):
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()


# ---------------------------------------------------------------- inputs
def logits(C, seed, rows=N * A):
    """[rows, C] f32 with the top two of every row at least GAP apart; rows 0 and 1: +-80"""
    g = torch.Generator().manual_seed(seed)
    z = 2.0 * torch.randn(rows, C, generator=g)
    z[::5, C - 1] += 6.0                            # background wins in about every fifth row, whatever C is
    top = z.topk(2, dim=1)
    close = (top.values[:, 0] - top.values[:, 1]) < 4 * GAP
    z[close, top.indices[close, 0]] += 8 * GAP
    z[0] = -80.0
    z[0, C - 2] = 80.0
    z[1] = -80.0
    z[1, C - 1] = 80.0
    t2 = z.double().topk(2, dim=1).values
    assert bool(((t2[:, 0] - t2[:, 1]) >= GAP).all())
    return z


def anchors(seed):
    g = torch.Generator().manual_seed(seed)
    yx = 20.0 + 260.0 * torch.rand(A, 2, generator=g)
    hw = 16.0 + 100.0 * torch.rand(A, 2, generator=g)
    return yx, hw


def ground_truth(C):
    gt = torch.full((N, P, 5), -1.0)
    g = torch.Generator().manual_seed(C)
    G = 5
    gt[0, :G, 0:2] = 40.0 + 200.0 * torch.rand(G, 2, generator=g)
    gt[0, :G, 2:4] = 20.0 + 90.0 * torch.rand(G, 2, generator=g)
    gt[0, :G, 4] = torch.tensor([C - 2, 0, 17, min(33, C - 3), C - 2], dtype=torch.float32)
    return gt, [G, 0]


def match_state(C, kind):
    """a hand-made matching result (the matching kernels do not depend on C): ngt, best [N, P], status [N, A], rgindex [N, A], counts [N, 4].
    Image 0: 5 boxes, two of which share their best anchor (a row visited twice), 9 further positive rows, rows 0 and 1 among them; image 1: no box, so no
    positive row.  status: SSD 1 positive / 2 negative / 0 a best anchor; RetinaNet 1 / 2 / 0 ignore band / 3 a best anchor."""
    rng = np.random.default_rng(C)
    ngt = np.array([5, 0], np.int32)
    best = np.full((N, P), -1, np.int32)
    best[0, :5] = [7, 150, 7, 299, 300]
    status = np.full((N, A), 2, np.uint8)
    status[0, [7, 150, 299, 300]] = 0 if kind == 'ssd' else 3
    pos = np.array([0, 1, 15, 16, 17, 100, 131, 200, 298])
    status[0, pos] = 1
    if kind == 'retina':
        status[0, 40:50] = 0
        status[1, 60:70] = 0
    rg = rng.integers(0, 5, size=(N, A)).astype(np.int32)
    rg[0, 0], rg[0, 1] = 0, 3                       # the +-80 rows: label C - 2 (its own high class) and label 33 against a high background
    counts = np.zeros((N, 4), np.int32)
    for n in range(N):
        counts[n, 0] = ngt[n] + int((status[n] == 1).sum())
        counts[n, 1] = int((status[n] == 2).sum())
        counts[n, 2] = min(3 * counts[n, 0], counts[n, 1])
    return ngt, best, status, rg, counts


# ---------------------------------------------------------------- float64 restatements
def softmax64(z):
    """z f32 [R, C] -> p, its bound bp, m, S, rS (all float64)"""
    z = z.astype(np.float64)
    C = z.shape[1]
    m = z.max(1, keepdims=True)
    d = z - m
    e = np.exp(d)
    S = e.sum(1, keepdims=True)
    D = (np.abs(d) * e).sum(1, keepdims=True) / S
    rS = U * (6 + D + sum_adds(C) + 1)
    p = e / S
    bp = p * (U * (np.abs(d) + 6) + rS + U) + TINY
    return dict(p=p, bp=bp, m=m[:, 0], S=S[:, 0], rS=rS[:, 0], z=z)


def pick_threshold(z):
    """a score threshold in the middle of the widest gap between neighbouring float64 confidences in [0.01, 0.02]: candidates on both sides, none near it"""
    p = np.concatenate([softmax64(zn)['p'][:, :-1].ravel() for zn in z])
    v = np.sort(p[(p > 0.01) & (p < 0.02)])
    assert v.size > 10
    i = int(np.argmax(np.diff(v)))
    return float(np.float32((v[i] + v[i + 1]) / 2))


def decode64(z, tbox, yx, hw, thr):
    """SSD300.py:157-171 / RetinaNet.py:224-238 for rows z [R, C], box regressions tbox [R, 4], anchors [R, 2] x 2"""
    sm = softmax64(z)
    C = z.shape[1]
    arg = sm['p'].argmax(1)
    keep = arg < C - 1
    conf, bconf = sm['p'][:, :C - 1], sm['bp'][:, :C - 1]
    assert bool((np.abs(conf - thr) > bconf).all()), 'a confidence within its bound of the threshold'
    cand = keep[:, None] & (conf >= thr)
    t, ay, ah = tbox.astype(np.float64), yx.astype(np.float64), hw.astype(np.float64)
    c = t[:, :2] * ah + ay
    s = ah * np.exp(t[:, 2:])
    boxes = np.concatenate([c - s / 2, c + s / 2], 1)
    bb = U * (np.abs(t[:, :2] * ah) + np.abs(c) + 3.5 * s)
    bbox = np.concatenate([bb, bb], 1) + U * np.abs(boxes) + TINY
    return dict(conf=conf, bconf=bconf, keep=keep.astype(np.uint8), cand=cand.astype(np.uint8), boxes=boxes, bboxes=bbox)


def _smooth_l1_row(zb, gb, ayx, ahw):
    """loss, its bound, gradient (clip), over the 4 coordinates of one positive row (float64)"""
    t = np.array([(gb[0] - ayx[0]) / ahw[0], (gb[1] - ayx[1]) / ahw[1], np.log(gb[2] / ahw[0]), np.log(gb[3] / ahw[1])])
    bt = np.array([2 * U * abs(t[0]), 2 * U * abs(t[1]), U * (1 + 6 * abs(t[2])), U * (1 + 6 * abs(t[3]))])
    d = zb - t
    bd = bt + U * np.abs(d)
    ad = np.abs(d)
    f = np.where(ad < 1, 0.5 * d * d, ad - 0.5)
    bf = np.minimum(ad, 1) * bd + 2 * U * f
    assert bool((np.abs(ad - 1) > bd).all()) and bool((ad > bd).all()), 'a coordinate within its bound of a kink of smooth L1'
    grad = np.where(ad < 1, d, np.sign(d))
    bgrad = np.where(ad < 1, bd, 0.0)
    return f.sum(), bf.sum() + 3 * U * f.sum(), grad, bgrad


def _sum_bound(values, bounds):
    v = np.abs(np.asarray(values, np.float64))
    return float(np.sum(bounds) + (len(v) + 48) * U * v.sum())


def ssd_loss64(pred, C, yx, hw, gt, ms, negloss, sel, grad_scale):
    """SSD300.py:430-450 on a given matching result; pred f32 [N, A, ld] -> parts [N, 4], dpred [N, A, ld] and their bounds"""
    ngt, best, status, rg, counts = ms
    ld = pred.shape[2]
    parts, bparts = np.zeros((N, 4)), np.zeros((N, 4))
    dp, bdp = np.zeros((N, A, ld)), np.zeros((N, A, ld))
    with np.errstate(all='ignore'):
        for n in range(N):
            sm = softmax64(pred[n, :, :C])
            num_pos, idx = int(counts[n, 0]), sel[n]
            gsn = grad_scale / len(idx) if len(idx) else 0.0
            for a in idx:
                g = (sm['p'][a] - (np.arange(C) == C - 1)) * gsn
                dp[n, a, :C] += g
                bdp[n, a, :C] += sm['bp'][a] * gsn + 4 * U * np.abs(g)
            neg = negloss[n, idx].astype(np.float64)
            rows = [(int(best[n, g]), g) for g in range(int(ngt[n]))] + [(a, int(rg[n, a])) for a in range(A) if status[n, a] == 1]
            ce, bce, co, bco = [], [], [], []
            gsp = grad_scale / num_pos if num_pos else 0.0
            for a, g in rows:
                label = int(gt[n, g, 4])
                zl = sm['z'][a, label] - sm['m'][a]
                v = np.log(sm['S'][a]) - zl
                ce.append(v)
                bce.append(sm['rS'][a] + 6 * U * abs(np.log(sm['S'][a])) + U * abs(zl) + U * abs(v))
                gr = (sm['p'][a] - (np.arange(C) == label)) * gsp
                twice = bool(np.any(dp[n, a, :C] != 0))
                dp[n, a, :C] += gr
                bdp[n, a, :C] += sm['bp'][a] * gsp + 4 * U * np.abs(gr) + (U * np.abs(dp[n, a, :C]) if twice else 0.0)
                f, bf, gc, bgc = _smooth_l1_row(pred[n, a, C:C + 4].astype(np.float64), gt[n, g, :4].astype(np.float64), yx[a].astype(np.float64),
                                                hw[a].astype(np.float64))
                co.append(f)
                bco.append(bf)
                twice = bool(np.any(dp[n, a, C:C + 4] != 0))
                dp[n, a, C:C + 4] += gc * gsp
                bdp[n, a, C:C + 4] += bgc * gsp + 3 * U * np.abs(gc * gsp) + (U * np.abs(dp[n, a, C:C + 4]) if twice else 0.0)
            v = [neg.sum() / len(idx) if len(idx) else np.nan, np.sum(ce) / num_pos if num_pos else np.nan, np.sum(co) / num_pos if num_pos else np.nan]
            b = [_sum_bound(neg, 0.0) / max(len(idx), 1), _sum_bound(ce, bce) / max(num_pos, 1), _sum_bound(co, bco) / max(num_pos, 1)]
            parts[n, :3] = v
            parts[n, 3] = v[0] + v[1] + v[2]
            bparts[n, :3] = np.array(b) + U * np.abs(np.nan_to_num(v)) + TINY
            bparts[n, 3] = bparts[n, :3].sum() + 2 * U * abs(np.nan_to_num(parts[n, 3]))
    return dict(parts=parts, bparts=bparts, dpred=dp, bdpred=bdp + TINY)


def _focal64(pu, alpha, gamma):
    pt = np.clip(pu, 1e-8, 1.0)
    om = 1.0 - pt
    lg = np.log(pt)
    loss = -alpha * om ** gamma * lg
    dpt = np.where(pu >= 1e-8, alpha * (gamma * om ** (gamma - 1.0) * lg - om ** gamma / pt), 0.0)
    return loss, dpt * pu


def retina_loss64(pconf, pbox, yx, hw, gt, ms, alpha, gamma, grad_scale):
    """RetinaNet.py:417-474 on a given matching result -> parts [N, 2], dconf [N, A, C], dbox [N, A, 4] and their bounds"""
    ngt, best, status, rg, counts = ms
    C = pconf.shape[2]
    parts, bparts = np.zeros((N, 2)), np.zeros((N, 2))
    dc, bdc = np.zeros((N, A, C)), np.zeros((N, A, C))
    db, bdb = np.zeros((N, A, 4)), np.zeros((N, A, 4))
    with np.errstate(all='ignore'):
        for n in range(N):
            sm = softmax64(pconf[n])
            num_pos = int(counts[n, 0])
            gs = grad_scale / num_pos if num_pos else np.inf
            rows = [(a, int(rg[n, a]), int(gt[n, int(rg[n, a]), 4])) for a in range(A) if status[n, a] == 1]
            rows += [(a, -1, C - 1) for a in range(A) if status[n, a] == 2]
            rows += [(int(best[n, g]), g, int(gt[n, g, 4])) for g in range(int(ngt[n]))]
            fl, bfl, co, bco = [], [], [], []
            for a, g, label in rows:
                pu = sm['p'][a, label]
                rp = sm['bp'][a, label] / pu if pu > 0 else 0.0
                assert abs(pu - 1e-8) > sm['bp'][a, label], 'a probability within its bound of the clip'
                loss, k = _focal64(pu, alpha, gamma)
                lo, klo = _focal64(pu * (1 - rp), alpha, gamma)
                hi, khi = _focal64(min(pu * (1 + rp), 1.0), alpha, gamma)
                fl.append(loss)
                bfl.append(max(abs(lo - loss), abs(hi - loss)) + 80 * U * abs(loss) + TINY)
                bk = max(abs(klo - k), abs(khi - k)) + 80 * U * abs(k)
                y = (np.arange(C) == label).astype(np.float64)
                gr = k * gs * (y - sm['p'][a])
                twice = bool(np.any(dc[n, a] != 0))
                dc[n, a] += gr
                bdc[n, a] += gs * (bk * np.abs(y - sm['p'][a]) + abs(k) * sm['bp'][a]) + 5 * U * np.abs(gr) + (U * np.abs(dc[n, a]) if twice else 0.0)
                if g >= 0:
                    f, bf, gc, bgc = _smooth_l1_row(pbox[n, a].astype(np.float64), gt[n, g, :4].astype(np.float64), yx[a].astype(np.float64),
                                                    hw[a].astype(np.float64))
                    co.append(f)
                    bco.append(bf)
                    twice = bool(np.any(db[n, a] != 0))
                    db[n, a] += gc * gs
                    bdb[n, a] += bgc * gs + 3 * U * np.abs(gc * gs) + (U * np.abs(db[n, a]) if twice else 0.0)
            inv = 1.0 / num_pos if num_pos else np.inf
            parts[n] = [np.sum(fl) * inv, np.sum(co) * inv]
            bparts[n] = [_sum_bound(fl, bfl) * inv, _sum_bound(co, bco) * inv]
            bparts[n] += 2 * U * np.abs(np.nan_to_num(parts[n], posinf=0.0)) + TINY
    return dict(parts=parts, bparts=bparts, dconf=dc, bdconf=bdc + TINY, dbox=db, bdbox=bdb + TINY)


# ---------------------------------------------------------------- comparison
def within(got, ref, bound, what):
    """|got - ref| <= bound element by element; returns (largest deviation, its share of the bound).  NaN in the reference must be NaN."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, 'NaN pattern', got[nan], ref[nan])
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), (what, 'infinities', got[inf], ref[inf])
    ok = ~(nan | inf)
    err = np.abs(got[ok] - ref[ok])
    share = err / bound[ok]
    i = int(np.argmax(share)) if share.size else 0
    worst = (float(err.max()) if err.size else 0.0, float(share.max()) if share.size else 0.0)
    print(f'{what}: largest deviation {worst[0]:.3e}, largest share of the bound {worst[1]:.3f}')
    assert share.size == 0 or share[i] <= 1.0, (what, 'deviation', err[i], 'bound', bound[ok][i], 'got', got[ok][i], 'reference', ref[ok][i])
    return worst


# ---------------------------------------------------------------- the cases
def ssd_inputs(C, dev):
    ld = C + 9
    z = logits(C, 1000 + C).view(N, A, C)
    g = torch.Generator().manual_seed(2000 + C)
    tb = 0.5 * torch.randn(N, A, 4, generator=g)
    pred = torch.full((N, A, ld), PAD_VALUE)
    pred[..., :C], pred[..., C:C + 4] = z, tb
    yx, hw = anchors(3000 + C)
    return pred, yx, hw


def ssd_decode_run(C, dev, batched):
    """odtk_ssd_decode per image, or odtk_ssd_decode_batched over both -> conf, boxes, keep, cand (device) and the inputs"""
    from odtk import ops
    pred, yx, hw = ssd_inputs(C, dev)
    thr = pick_threshold(pred[..., :C].numpy())
    pred_d, yx_d, hw_d = pred.to(dev), yx.to(dev), hw.to(dev)
    conf = torch.full((N, A, C - 1), -7.0, device=dev)
    boxes = torch.full((N, A, 4), -7.0, device=dev)
    keep = torch.full((N, A), 7, dtype=torch.uint8, device=dev)
    cand = torch.full((N, A, C - 1), 7, dtype=torch.uint8, device=dev)
    if batched:
        ops.ssd_decode_batched(pred_d, C, yx_d, hw_d, thr, conf, boxes, keep, cand)
    else:
        for n in range(N):
            ops.ssd_decode(pred_d[n], C, yx_d, hw_d, thr, conf[n], boxes[n], keep[n], cand[n])
    _sync(dev)
    return conf, boxes, keep, cand, (pred[..., :C].numpy(), pred[..., C:C + 4].numpy(), yx.numpy(), hw.numpy(), thr)


def check_ssd_decode(C, dev, batched):
    conf, boxes, keep, cand, x = ssd_decode_run(C, dev, batched)
    return _compare_decode('ssd_decode' + ('_batched' if batched else '') + f' C={C}', *x, conf, boxes, keep, cand)


def retina_decode_run(C, dev, batched):
    from odtk import ops
    z = logits(C, 4000 + C).view(N, A, C)
    g = torch.Generator().manual_seed(5000 + C)
    tb = 0.5 * torch.randn(N, A, 4, generator=g)
    yx, hw = anchors(6000 + C)
    thr = pick_threshold(z.numpy())
    z_d, tb_d, yx_d, hw_d = z.to(dev), tb.to(dev), yx.to(dev), hw.to(dev)
    if batched:
        conf = torch.full((N, A, C - 1), -7.0, device=dev)
        boxes = torch.full((N, A, 4), -7.0, device=dev)
        keep = torch.full((N, A), 7, dtype=torch.uint8, device=dev)
        cand = torch.full((N, A, C - 1), 7, dtype=torch.uint8, device=dev)
        ops.retina_decode_batched(z_d, tb_d, yx_d, hw_d, thr, conf, boxes, keep, cand)
    else:
        outs = [ops.retina_decode(z_d[n], tb_d[n], yx_d, hw_d, thr) for n in range(N)]
        conf, boxes, keep, cand = (torch.stack([o[i] for o in outs]) for i in range(4))
    _sync(dev)
    return conf, boxes, keep, cand, (z.numpy(), tb.numpy(), yx.numpy(), hw.numpy(), thr)


def check_retina_decode(C, dev, batched):
    conf, boxes, keep, cand, x = retina_decode_run(C, dev, batched)
    return _compare_decode('retina_decode' + ('_batched' if batched else '') + f' C={C}', *x, conf, boxes, keep, cand)


def _compare_decode(what, z, tb, yx, hw, thr, conf, boxes, keep, cand):
    worst = (0.0, 0.0)
    for n in range(N):
        ref = decode64(z[n], tb[n], yx, hw, thr)
        assert 0 < int(ref['keep'].sum()) < A and int(ref['cand'].sum()) > 0
        assert n > 0 or (ref['keep'][0] == 1 and ref['keep'][1] == 0)            # the +-80 rows: the last object class, the background
        assert np.array_equal(keep[n].cpu().numpy(), ref['keep']), (what, n, 'keep')
        assert np.array_equal(cand[n].cpu().numpy(), ref['cand']), (what, n, 'cand')
        w1 = within(conf[n].cpu().numpy(), ref['conf'], ref['bconf'], f'{what} image {n} conf')
        w2 = within(boxes[n].cpu().numpy(), ref['boxes'], ref['bboxes'], f'{what} image {n} boxes')
        worst = max(worst, w1, w2, key=lambda w: w[1])
    return worst


def ssd_loss_run(C, dev, pred=None):
    """-> (loss_parts [N, 4], dpred [N, A, ld]) on the device and the inputs the restatement needs"""
    from odtk import ops
    pred0, yx, hw = ssd_inputs(C, dev)
    pred = pred0 if pred is None else pred
    ld = pred.shape[2]
    gt, _ = ground_truth(C)
    ms = match_state(C, 'ssd')
    ngt, best, status, rg, counts = ms
    sel = [np.nonzero(status[n] == 2)[0][3::4][:40].astype(np.int32) for n in range(N)]
    sel_idx = np.full((N, A), -1, np.int32)
    for n in range(N):
        sel_idx[n, : len(sel[n])] = sel[n]
    sel_cnt = np.array([len(s) for s in sel], np.int32)
    pred_d = pred.to(dev)
    negloss = torch.full((N, A), -7.0, device=dev)
    ops.softmax_ce_const(pred_d, N * A, C, ld, C - 1, negloss)
    parts = torch.full((N, 4), -7.0, device=dev)
    dpred = torch.full((N, A, ld), -7.0, device=dev)
    t = lambda x: torch.from_numpy(x).to(dev)
    ops.ssd_loss(pred_d, C, yx.to(dev), hw.to(dev), gt.to(dev), t(ngt), t(best), t(status), t(rg), t(counts), negloss, t(sel_idx), t(sel_cnt), 1.0 / N, parts,
                 dpred)
    _sync(dev)
    return parts.cpu().numpy(), dpred.cpu().numpy(), dict(pred=pred.numpy(), yx=yx.numpy(), hw=hw.numpy(), gt=gt.numpy(), ms=ms, sel=sel,
                                                         negloss=negloss.cpu().numpy())


def check_ssd_loss(C, dev):
    parts, dpred, x = ssd_loss_run(C, dev)
    ref = ssd_loss64(x['pred'], C, x['yx'], x['hw'], x['gt'], x['ms'], x['negloss'], x['sel'], 1.0 / N)
    assert np.isnan(ref['parts'][1, 1:]).all() and np.isfinite(ref['parts'][1, 0]) and np.isfinite(ref['parts'][0]).all()      # image 1: no positive row
    assert bool((dpred[..., C + 4:] == 0).all())                                  # the pad columns of the gradient are zero
    w1 = within(parts, ref['parts'], ref['bparts'], f'ssd_loss C={C} parts')
    w2 = within(dpred, ref['dpred'], ref['bdpred'], f'ssd_loss C={C} dpred')
    return max(w1, w2, key=lambda w: w[1])


def retina_loss_run(C, dev):
    from odtk import ops
    z = logits(C, 7000 + C).view(N, A, C)
    g = torch.Generator().manual_seed(8000 + C)
    tb = 0.5 * torch.randn(N, A, 4, generator=g)
    yx, hw = anchors(9000 + C)
    gt, _ = ground_truth(C)
    ms = match_state(C, 'retina')
    ngt, best, status, rg, counts = ms
    t = lambda x: torch.from_numpy(x).to(dev)
    parts = torch.full((N, 2), -7.0, device=dev)
    dconf = torch.full((N, A, C), -7.0, device=dev)
    dbox = torch.full((N, A, 4), -7.0, device=dev)
    ops.retina_loss(z.to(dev), tb.to(dev), yx.to(dev), hw.to(dev), gt.to(dev), t(ngt), t(best), t(status), t(rg), t(counts), 0.25, 2.0, 1.0 / N, parts, dconf,
                    dbox)
    _sync(dev)
    return parts.cpu().numpy(), dconf.cpu().numpy(), dbox.cpu().numpy(), dict(z=z.numpy(), tb=tb.numpy(), yx=yx.numpy(), hw=hw.numpy(), gt=gt.numpy(), ms=ms)


def check_retina_loss(C, dev):
    parts, dconf, dbox, x = retina_loss_run(C, dev)
    ref = retina_loss64(x['z'], x['tb'], x['yx'], x['hw'], x['gt'], x['ms'], 0.25, 2.0, 1.0 / N)
    assert np.isfinite(ref['parts'][0]).all() and not np.isfinite(ref['parts'][1]).any()        # image 1: sums scaled by 1 / 0
    assert not np.isfinite(parts[1]).any()
    w = [within(parts[0], ref['parts'][0], ref['bparts'][0], f'retina_loss C={C} parts'),
         within(dconf[0], ref['dconf'][0], ref['bdconf'][0], f'retina_loss C={C} dconf'),
         within(dbox[0], ref['dbox'][0], ref['bdbox'][0], f'retina_loss C={C} dbox')]
    return max(w, key=lambda v: v[1])


# ---- FCOS: the oracle takes the class count from its operands; it runs here in float64
FCOS_SIZE = 64


def fcos_inputs(C, seed):
    from oracle import fcos_ref as FR
    shapes = FR.level_shapes(FCOS_SIZE, FCOS_SIZE)
    g = torch.Generator().manual_seed(seed)
    conf = [torch.randn(N, h, w, C, generator=g) * 2.0 - 2.0 for h, w in shapes]
    reg = [torch.rand(N, h, w, 4, generator=g) * 6.0 + 0.5 for h, w in shapes]
    center = [torch.randn(N, h, w, 1, generator=g) for h, w in shapes]
    conf[0][0, 0, 0, :] = -80.0
    conf[0][0, 0, 0, C - 1] = 80.0
    gt = torch.full((N, P, 5), -1.0)
    # (the 64 x 64 box trains levels 0 and 1; levels 2 - 4 and image 1 have no box)
    gt[0, :5] = torch.tensor([[20., 22., 30., 26., C - 1], [40., 30., 36., 44., 0], [30., 36., 50., 40., min(64, C - 3)], [12., 50., 16., 20., C - 2],
                              [32., 32., 64., 64., 1]])
    return conf, reg, center, gt


def fcos_run(C, dev, operands=None):
    from odtk import ops
    conf, reg, center, gt = fcos_inputs(C, 11000 + C) if operands is None else operands
    cd, rd, ed = ([t.to(dev) for t in x] for x in (conf, reg, center))
    loss = torch.full((N,), -7.0, device=dev)
    d_conf, d_reg, d_center = ([torch.full_like(t, -7.0) for t in x] for x in (cd, rd, ed))
    ws = ops.fcos_workspace(cd, N, dev)
    ops.fcos_loss(cd, rd, ed, gt.to(dev), 1.0 / N, loss, d_conf, d_reg, d_center, ws)
    _sync(dev)
    return loss.cpu(), [t.cpu() for t in d_conf], [t.cpu() for t in d_reg], [t.cpu() for t in d_center], (conf, reg, center, gt)


def check_fcos_loss(C, dev):
    """against oracle/fcos_ref.py in float64 (loss and autograd gradients).  Bounds: the heat-map sum of a level is the sum over H W C terms, each evaluated to
    40 u relative (two 12 u functions, four products, the cancellation in -k + log_sigmoid(k) measured against the term itself only where k > -1) plus, for
    k <= -1, u (|k| + |ls|) s^2 / 4 absolute; summed to (C + 48) u.  Every term of the loss is positive, so sum|terms| / count is the loss itself: loss bound =
    (C + 90) u loss + u / 4 sum softplus(|k|) (the absolute part, softplus(|k|) >= |k| + |ls| s^2 for k < 0).  A gradient element is the
    same evaluation without a sum: 60 u relative plus u (|k| + |ls|) s^2 / 2 / count, in units of grad_scale."""
    from oracle import fcos_ref as FR
    loss, d_conf, d_reg, d_center, (conf, reg, center, gt) = fcos_run(C, dev)
    c64 = [t.double().requires_grad_(True) for t in conf]
    r64 = [t.double().requires_grad_(True) for t in reg]
    e64 = [t.double().requires_grad_(True) for t in center]
    per_image = [FR.one_image_loss([t[n] for t in c64], [t[n] for t in r64], [t[n] for t in e64], gt[n].double()) for n in range(N)]
    assert per_image[0].dtype == torch.float64
    (sum(per_image) / N).backward()
    ref = torch.stack([v.detach().double() for v in per_image]).numpy()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)         # a level no box trains: no gradient
    assert ref[0] > 0 and ref[1] == 0                                            # image 1 has no box: every level contributes 0
    mag = sum(float(torch.nn.functional.softplus(t[0].double().abs()).sum()) for t in conf)        # >= the sum of the absolute heat-map terms
    within(loss.numpy(), ref, (C + 90) * U * np.abs(ref) + U * mag / 4.0 + TINY, f'fcos_loss C={C} loss')
    worst = (0.0, 0.0)
    for l in range(len(conf)):
        gref = zero(c64[l]).numpy()
        k = conf[l].double().numpy()
        s = 1.0 / (1.0 + np.exp(-k))
        bound = 60 * U * np.abs(gref) + U * (np.abs(k) + np.abs(np.log1p(np.exp(-np.abs(k))) + np.maximum(-k, 0))) * s * s / 2.0 / N + TINY
        worst = max(worst, within(d_conf[l].numpy(), gref, bound, f'fcos_loss C={C} d_conf level {l}'), key=lambda w: w[1])
    # d_reg and d_center do not read the class logits: the wide kernel computes them with the statements of the one-word kernel, from the same operands and
    # the same count.  They are held to EQUALITY with the one-word kernel's (the first 64 classes of the same tensors, the labels replaced by their ranks) instead
    # of a bound of their own; tests/test_gpu_dense_heads.py holds the one-word kernel to the oracle.
    if C > 64:
        fold = gt.clone()                             # labels -> their rank: the same pattern of equal and different classes, below 64
        valid = fold[..., 0] >= 0
        ranks = {v: i for i, v in enumerate(sorted(set(fold[..., 4][valid].tolist())))}
        fold[..., 4][valid] = torch.tensor([float(ranks[v]) for v in fold[..., 4][valid].tolist()])
        _, _, n_reg, n_center, _ = fcos_run(64, dev, operands=([t[..., :64].contiguous() for t in conf], reg, center, fold))
        for l in range(len(conf)):
            assert torch.equal(d_reg[l], n_reg[l]) and torch.equal(d_center[l], n_center[l]), ('fcos_loss d_reg / d_center against the one-word kernel', C, l)
    return worst


# ---------------------------------------------------------------- reruns, refusals, the narrow kernels at their limit
def check_rerun(dev):
    """two runs of every entry point on the same operands give the same bytes -- also where float atomics add a row's second visit: two addends commute"""
    C = 81
    a, b = ssd_loss_run(C, dev), ssd_loss_run(C, dev)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])
    a, b = retina_loss_run(C, dev), retina_loss_run(C, dev)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:3], b[:3]))
    a, b = fcos_run(C, dev), fcos_run(C, dev)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for i in (1, 2, 3) for x, y in zip(a[i], b[i]))
    for run in (ssd_decode_run, retina_decode_run):
        for batched in (False, True):
            a, b = run(C, dev, batched), run(C, dev, batched)
            assert all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])), (run.__name__, batched)


def check_refusals(dev):
    """C = 257 is refused by every entry point, with the limit in the message"""
    import pytest
    from odtk import ops
    C = 257
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    pred, yx, hw, gt = z(1, 4, C + 4), z(4, 2), z(4, 2) + 1.0, z(1, P, 5) - 1.0
    i32, u8 = torch.int32, torch.uint8
    conf, boxes, keep, cand = z(1, 4, C - 1), z(1, 4, 4), z(1, 4, dt=u8), z(1, 4, C - 1, dt=u8)
    with pytest.raises(Exception, match=r'ssd_loss: C=257 .*256'):
        ops.ssd_loss(pred, C, yx, hw, gt, z(1, dt=i32), z(1, P, dt=i32), z(1, 4, dt=u8), z(1, 4, dt=i32), z(1, 4, dt=i32), z(1, 4), z(1, 4, dt=i32), z(1, dt=i32),
                     1.0, z(1, 4), z(1, 4, C + 4))
    with pytest.raises(Exception, match=r'ssd_decode: C=257 .*256'):
        ops.ssd_decode(pred[0], C, yx, hw, 0.5, conf[0], boxes[0], keep[0], cand[0])
    with pytest.raises(Exception, match=r'ssd_decode_batched: C=257 .*256'):
        ops.ssd_decode_batched(pred, C, yx, hw, 0.5, conf, boxes, keep, cand)
    with pytest.raises(Exception, match=r'retina_decode: C=257 .*256'):
        ops.retina_decode(z(4, C), z(4, 4), yx, hw, 0.5)
    with pytest.raises(Exception, match=r'retina_decode_batched: C=257 .*256'):
        ops.retina_decode_batched(z(1, 4, C), z(1, 4, 4), yx, hw, 0.5, conf, boxes, keep, cand)
    with pytest.raises(Exception, match=r'retina_loss: C=257 .*256'):
        ops.retina_loss(z(1, 4, C), z(1, 4, 4), yx, hw, gt, z(1, dt=i32), z(1, P, dt=i32), z(1, 4, dt=u8), z(1, 4, dt=i32), z(1, 4, dt=i32), 0.25, 2.0, 1.0,
                        z(1, 2), z(1, 4, C), z(1, 4, 4))
    lv = [z(1, s, s, C) for s in (8, 4, 2, 1, 1)]
    with pytest.raises(Exception, match=r'fcos_loss: N=1 C=257 .*256'):
        ops.fcos_loss(lv, [z(1, s, s, 4) for s in (8, 4, 2, 1, 1)], [z(1, s, s, 1) for s in (8, 4, 2, 1, 1)], gt, 1.0, z(1), [t.clone() for t in lv],
                      [z(1, s, s, 4) for s in (8, 4, 2, 1, 1)], [z(1, s, s, 1) for s in (8, 4, 2, 1, 1)], ops.fcos_workspace(lv, 1, dev))


# ---------------------------------------------------------------- the one-thread kernels at their limits, byte for byte
def limit_outputs(dev):
    """every output of the seven entry points at C = 32 (FCOS: C = 64), where the host must still pick the one-thread kernels: name -> numpy array.  The CPU
    tier compares them with a build of the same sources whose dispatch is pinned to the one-thread kernels; the GPU tier with the SHA-256 of the bytes the
    commit before the wide kernels wrote on an MI355X (tests/golden/wide_rows_limit_sha256.json)."""
    out = {}
    for name, run in (('ssd_decode', ssd_decode_run), ('retina_decode', retina_decode_run)):
        for batched in (False, True):
            r = run(NARROW, dev, batched)
            for k, t in zip(('conf', 'boxes', 'keep', 'cand'), r[:4]):
                out[f'{name}{"_batched" if batched else ""}.{k}'] = t.cpu().numpy()
    parts, dpred, _ = ssd_loss_run(NARROW, dev)
    out['ssd_loss.parts'], out['ssd_loss.dpred'] = parts, dpred
    parts, dconf, dbox, _ = retina_loss_run(NARROW, dev)
    out['retina_loss.parts'], out['retina_loss.dconf'], out['retina_loss.dbox'] = parts, dconf, dbox
    loss, d_conf, d_reg, d_center, _ = fcos_run(64, dev)
    out['fcos_loss.loss'] = loss.numpy()
    for l in range(len(d_conf)):
        out[f'fcos_loss.d_conf{l}'], out[f'fcos_loss.d_reg{l}'], out[f'fcos_loss.d_center{l}'] = d_conf[l].numpy(), d_reg[l].numpy(), d_center[l].numpy()
    return out


def sha256_of(outputs):
    import hashlib
    return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in outputs.items()}
