"""Edge cases through the box-side kernels of Light-Head R-CNN (csrc/lhrcnn.hip): the case bodies shared by tests/test_cpu_lhrcnn_edge.py (the kernel source
under the fiber emulation, tests/hip_cpu_backend.py) and tests/test_gpu_lhrcnn_edge.py (libodtk.so on the device).  Banded, the Case table idiom and the
comparison rules are those of tests/edge_gt_cases.py (imported, not copied); Light-Head R-CNN is a sibling module and not an eighth Family there because its
table runs at three picture shapes and has three more groups of cases that are not ground-truth sets.

Four groups, PARAMS = [(group, case)]:
  rpn ...... odtk_lhrcnn_match -> odtk_nms_batched x 2 -> odtk_lhrcnn_rpn_loss, chained as tests/test_gpu_lhrcnn.py::test_rpn_loss_chain_vs_oracle chains them.
             N = 2: image 0 carries LR.synthetic_gt rows, image 1 (the LAST) the edge case.  Reference: oracle/lhrcnn_ref.py rpn_one_image(detail=True) per
             image, in float32 -- the function takes its 0.5 / 0.3 / arg-max decisions in the dtype of its inputs and the cases pin exactly those decisions in
             f32, so it does not allow float64 -- and autograd for the gradients.
  rcnn ..... odtk_lhrcnn_rcnn_loss against a float64 restatement (losses and ANALYTIC gradients: autograd gives 0 * inf = NaN behind torch.where at an
             infinite box target, where the kernel -- and the formula -- give +-1 * w).
  decode ... odtk_lhrcnn_rpn_decode, odtk_lhrcnn_gather_rois, odtk_lhrcnn_rcnn_decode against float64 restatements of lhrcnn_ref.detect's pieces.
  crop ..... odtk_crop_and_resize_fwd / _bwd, f32 and bf16, against LR.crop_and_resize on a float64 picture (the sample positions stay f32: one ulp decides
             inside / outside on the border) and autograd.

Rules (those of edge_gt_cases.py):
  * every output and gradient operand of every launch -- the whole ops.lhrcnn_workspace key set, d_conf, d_bbox, d_logits, d_pbbox, the crop outputs, prop,
    score, conf, boxes, cand -- lies between two bands of BAND sentinel elements, which must be untouched after the launch;
  * index lists, counts and status bytes are exact;
  * finite reference value: the tolerance of the existing test of that kernel, quoted in TOL; no case needed a wider one;
  * non-finite reference value: the kernel's value is non-finite of the same kind at the same position; gradients are compared where the reference is finite;
  * d_conf / d_bbox start at 5.0 and must be fully written (0 where the reference gradient is 0);
  * a second launch agrees bit for bit (no float atomics), except crop_and_resize_bwd, whose atomics are compared to tolerance;
  * `rejects`: the oracle raises (G = 0: a reduction over no box).  Then the outputs are of the kind the expressions give, two runs are bit-identical, bands hold;
  * `refused`: the library returns an error naming the limit and leaves every operand as it was.
Every construction a case relies on (threshold side, best_a < G, n_pos > 128, kn short / zero, the A ranges) is asserted inside the case from the oracle alone.
"""
import math

import numpy as np
import torch

import edge_gt_cases as EG
from edge_gt_cases import BAND, Banded, Case, EDGE, _kind, _ops          # noqa: F401
from oracle import lhrcnn_ref as LR

EG.FILL.setdefault(torch.bfloat16, 1352.0)           # exact in bf16

TOL = dict(
    rpn='total loss 1e-5 |r|; d_conf / d_bbox 1e-5 of the largest reference gradient; roi_prop rtol 1e-5 atol 1e-3, roi_box rtol 1e-5 atol 1e-5, roi_truth rtol '
        '1e-4 atol 1e-5; NMS scores 1e-5 |r| (test_rpn_loss_chain_vs_oracle)',
    rcnn='loss parts 1e-5 |r|; gradients 1e-5 of the largest reference gradient (test_rcnn_loss_kernel)',
    decode='scores and confidences 1e-5 |r|; proposals rtol 1e-5 atol 1e-3 (roi_prop of test_rpn_loss_chain_vs_oracle); decoded boxes 1e-5 of the operands '
           '|centre| + |size| / 2 of the subtraction (the f32-kernel bound of tests/test_gpu_lhrcnn.py) + 1e-6',
    crop='f32 1e-5, bf16 1e-2 of the largest reference value; image gradient 1e-4 (test_crop_and_resize_kernels)')
SHAPES = dict(big=(320, 416), mid=(160, 192), small=(128, 160))        # kept anchors: 754, 96 (one pass of the ballot loop, idle lanes), 52 (< one wave)
A_RANGE = dict(big=(256, 1 << 30), mid=(65, 255), small=(1, 63))
C_RPN = 21
LH_MAX_GT, LH_MAX_POS, LH_ROIS = 128, 128, 256


def _dev(dev):
    return torch.device(dev)


def _sync(dev):
    if _dev(dev).type == 'cuda':
        torch.cuda.synchronize()


def _intact(out, what):
    for k, b in out.items():
        assert b.intact(), f'{what}: {k} written outside its operand: {b.damage()}'


def _host(out):
    return {k: b.t.detach().cpu().clone() for k, b in out.items()}


def _same_bits(a, b, what):
    for k in a:
        same = (a[k] == b[k]) | ((a[k] != a[k]) & (b[k] != b[k])) if a[k].is_floating_point() else a[k] == b[k]
        assert bool(same.all()), (what, k, 'two runs differ')


def _cmp(got, ref, rtol, atol, what):
    """finite reference: |got - ref| <= atol + rtol |ref|; non-finite reference: the same kind at the same position"""
    got, ref = got.double().flatten(), ref.double().flatten()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = torch.isfinite(ref)
    bad = torch.nonzero(fin & ~((got - ref).abs() <= atol + rtol * ref.abs())).flatten()
    assert bad.numel() == 0, (what, int(bad[0]), float(got[bad[0]]), float(ref[bad[0]]))
    for j in torch.nonzero(~fin).flatten().tolist():
        assert _kind(float(got[j])) == _kind(float(ref[j])), (what, j, float(got[j]), float(ref[j]))


def _rel_where_finite(got, ref, tol, what):
    """largest error over the finite reference entries, relative to the largest of them"""
    got, ref = got.double(), ref.double()
    m = torch.isfinite(ref)
    if not bool(m.any()):
        return
    err = float((got[m] - ref[m]).abs().max())
    scale = float(ref[m].abs().max())
    assert math.isfinite(err) and err <= tol * scale, (what, err, scale)


# ================================================================================================================== RPN chain
class LH(EG.Family):
    name, classes = 'lhrcnn', 20

    def __init__(self, key):
        self.key, self.hw = key, SHAPES[key]
        H, W = self.hw
        self.fh, self.fw = -(-H // 32), -(-W // 32)
        self.A_full = self.fh * self.fw * LR.NA
        self.anc = LR.anchors(self.fh, self.fw, H, W)
        self.A = int(self.anc['yx'].shape[0])
        self._thr = {}

    def ordinary(self, seed, pad):
        return LR.synthetic_gt(1, self.hw[0], self.hw[1], seed, pad=pad, max_obj=4)[0]

    def gt(self, case):
        P = case.pad or 7
        gt = torch.full((2, P, 5), -1.0)
        o = self.ordinary(41, P)
        gt[0] = o
        if case.name == 'reversed':
            G = LR.num_real(o)
            gt[EDGE, :G] = o[:G].flip(0)
        else:
            rows = torch.tensor(case.rows(self), dtype=torch.float64).reshape(-1, 5)
            assert rows.shape[0] <= P, case.name
            rows[:, 4] = rows[:, 4] % self.classes
            gt[EDGE, : rows.shape[0]] = rows.float()
        return gt

    def inputs(self):
        g = torch.Generator().manual_seed(self.A_full)
        return dict(conf=torch.randn(2, self.A_full, 2, generator=g), bbox=torch.randn(2, self.A_full, 4, generator=g) * 0.3)

    # ---- constructions
    def anchor_row(self, p, cls=3):
        yx, hw = self.anc['yx'], self.anc['hw']
        return [float(yx[p, 0]), float(yx[p, 1]), float(hw[p, 0]), float(hw[p, 1]), cls]

    def iou_row(self, row):
        """f32 IoU of one ground-truth row with every kept anchor, in the op order of rpn_one_image (and of lh_iou, 1e-8f included)"""
        a = self.anc
        g = torch.tensor(row[:4], dtype=torch.float32)
        y1x1, y2x2 = g[0:2] - g[2:4] / 2., g[0:2] + g[2:4] / 2.
        inter = torch.clamp(torch.minimum(a['y2x2'], y2x2) - torch.maximum(a['y1x1'], y1x1), min=0).prod(-1)
        return inter / (a['hw'].prod(-1) + g[2:4].prod() - inter + 1e-8)

    def candidates(self):
        """square anchors of 64 px well inside the picture, whose lower neighbour cell holds the same anchor; nearest the centre first"""
        yx, hw, H, W = self.anc['yx'], self.anc['hw'], self.hw[0], self.hw[1]
        ok = (hw[:, 0] == 64) & (hw[:, 1] == 64) & (yx[:, 0] + 32 + 64 <= H - 2)
        idx = torch.nonzero(ok).flatten()
        d = (yx[idx, 0] - H / 2.) ** 2 + (yx[idx, 1] - W / 2.) ** 2
        return idx[torch.argsort(d, stable=True)].tolist()

    def threshold_candidates(self):
        """anchors up to 130 px high whose lower neighbour cell holds the same anchor shape (the irrational sizes s * sqrt(2) reach IoUs that the
        64 px squares, whose areas are exact in f32, never round to)"""
        yx, hw, H = self.anc['yx'], self.anc['hw'], self.hw[0]
        return torch.nonzero((hw[:, 0] <= 130) & (yx[:, 0] + 32 + hw[:, 0] / 2 <= H - 2)).flatten().tolist()

    def threshold_row(self, thr, side):
        """a copy of anchor p moved down by d = h (1 - thr) / (1 + thr): IoU(p) = thr in exact arithmetic, and the same anchor one cell further down
        overlaps the box more, so p is NOT the box's best anchor (a best anchor is positive whatever its IoU).  The f32 neighbours of that box -- centre and
        height moved by single f32 steps -- are searched for the largest f32 IoU(p) below thr, one equal to float32(thr), and the smallest above it.
        -> (iou, row, p); the side is asserted again from the oracle's own match in the case"""
        if thr not in self._thr:
            t32 = float(np.float32(thr))
            found = {}
            for p in self.threshold_candidates():
                yc, xc, h, w, _ = self.anchor_row(p)
                y0 = np.float32(yc + h * (1. - thr) / (1. + thr))
                for kh in range(-2, 3):
                    hk = np.float32(h)
                    for _ in range(abs(kh)):
                        hk = np.nextafter(hk, np.float32(np.inf if kh > 0 else 0))
                    yk = y0
                    for _ in range(8):
                        yk = np.nextafter(yk, np.float32(0))
                    for _ in range(17):
                        row = [float(yk), xc, float(hk), w, 3]
                        iou = self.iou_row(row)
                        if int(torch.argmax(iou)) != p:
                            v = float(iou[p])
                            if v < t32 and ('below' not in found or v > found['below'][0]):
                                found['below'] = (v, row, p)
                            if v > t32 and ('above' not in found or v < found['above'][0]):
                                found['above'] = (v, row, p)
                            if v == t32:
                                found.setdefault('exact', (v, row, p))
                        yk = np.nextafter(yk, np.float32(np.inf))
                if len(found) == 3:
                    break
            assert len(found) == 3, (self.key, thr, sorted(found))
            self._thr[thr] = found
        return self._thr[thr][side]


_FAM = {}


def family(key):
    if key not in _FAM:
        _FAM[key] = LH(key)
    return _FAM[key]


class LCase(Case):
    def __init__(self, name, rows, shape='big', verify=None, **kw):
        Case.__init__(self, name, rows, **kw)
        self.shape, self.verify = shape, verify


def _crowd(n, seed, min_at=None):
    return EG._crowd(n, seed, min_at)


def _distinct_crowd(n, seed):
    """n boxes of a larger crowd whose best anchors are all different.  Two boxes with one best anchor put two rows with the SAME box and score into the
    positive list, and on exactly equal scores odtk_nms_batched visits the lower index first (include/odtk.h) where the oracle's NonMaxSuppressionV3 follows
    the heap order of the reference's priority queue: which of the copies survives -- and with it pos_gt of that row -- then differs on the device.  That
    is a documented property of the NMS kernel and not what the crowded cases are about; `same_best_anchor` and the dup_* cases keep a duplicate pair."""
    def rows(f):
        seen, out = set(), []
        for r in EG._crowd(6 * n, seed)(f):
            b = int(torch.argmax(f.iou_row(r)))
            if b not in seen:
                seen.add(b)
                out.append(r)
        assert len(out) >= n, (len(out), n)
        return out[:n]
    return rows


def _H(f):
    return float(f.hw[0])


def _W(f):
    return float(f.hw[1])


def _no_overlap_rows(f):
    # row 0: an ordinary box in the lower right part of the picture; row 1: a box below the picture -- kept anchors end at H - 2, so every IoU is 0
    return [[0.62 * _H(f), 0.6 * _W(f), 0.45 * _H(f), 0.4 * _W(f), 7], [_H(f) + 60., 0.5 * _W(f), 40., 50., 11]]


def _collide_rows(f):
    yc, xc, h, w, _ = f.anchor_row(f.candidates()[0])
    return [[yc + 1.0, xc + 0.5, h * 1.04, w * 0.97, 2], [yc - 0.5, xc - 1.0, h * 0.96, w * 1.03, 5]]


def _many_positive_rows(f):
    idx = torch.nonzero(f.anc['hw'].max(1).values < 50).flatten()[::2][:120].tolist()
    assert len(idx) == 120 and len(set(idx)) == 120
    return [f.anchor_row(p, k) for k, p in enumerate(idx)]


def _every_anchor_rows(f):
    return [f.anchor_row(p, p) for p in range(f.A)]


# ---- what a case asserts from the oracle alone (d: rpn_one_image's detail of the edge image, lab: the returned labels of the picked positives)
def _v_all_valid(f, gt, d, lab):
    assert d['G'] == 4 and bool((gt[EDGE, :, 0] >= 0).all()), 'construction: no pad row, the arg-min row is 4'


def _v_no_overlap(f, gt, d, lab):
    G, label = d['G'], gt[EDGE, :, 4].long()
    assert G == 2 and float(d['iou'][1].max()) == 0.0, 'construction: row 1 overlaps a kept anchor'
    assert int(d['best_a'][1]) == 0 and 0 < G, 'construction: best_a of the all-zero row is not 0'
    where = torch.nonzero(d['sel_p'] == 1).flatten()
    assert where.numel() == 1, 'construction: the row of box 1 does not survive the NMS'
    assert int(lab[where[0]]) == int(label[0]) and int(label[0]) != int(label[1]), 'construction: label[best_a] = label[0] must differ from the own class'


def _v_same_best(f, gt, d, lab):
    assert int(d['best_a'][0]) == int(d['best_a'][1]) and int(d['pos_a'][0]) == int(d['pos_a'][1]), 'construction: the two boxes do not share their best anchor'
    assert int((d['sel_p'] < 2).sum()) == 1, 'construction: the duplicate row survives (or both fall to) the IoU 0.7 NMS'


def _v_exact(f, gt, d, lab):
    assert float(d['iou'][0].max()) > 1 - 1e-6 and int(d['best_a'][0]) == f.candidates()[0]


def _v_threshold(thr, side):
    def v(f, gt, d, lab):
        val, row, p = f.threshold_row(thr, side)
        assert d['G'] == 1 and int(d['best_a'][0]) != p, 'construction: the chosen anchor is the best anchor'
        got = float(d['iou'][0, p])
        t32 = float(np.float32(thr))
        assert got == val and (got < t32 if side == 'below' else got == t32 if side == 'exact' else got > t32), (thr, side, got)
        want = (1 if side == 'above' else 0) if thr == 0.5 else (2 if side == 'below' else 0)
        assert _status(f, d)[p] == want, (thr, side, int(_status(f, d)[p]), want)
    return v


def _v_pad_128(f, gt, d, lab):
    assert d['G'] == 127 and len(set(d['best_a'].tolist())) == 127, 'construction: 127 boxes with 127 different best anchors'


def _v_many_positive(f, gt, d, lab):
    n_pos, n_neg = d['pos_a'].shape[0], d['neg_o'].shape[0]
    assert d['G'] == 120 and n_pos > LH_MAX_POS and min(n_pos, 128) == 128 and min(n_neg, 256 - 128) == 128, (d['G'], n_pos, n_neg)


def _v_few_negative(f, gt, d, lab):
    kp, kn = d['sel_p'].shape[0], d['sel_n'].shape[0]
    assert f.A < 64 and 0 < kn < LH_ROIS - kp, (kp, kn)


def _v_no_negative(f, gt, d, lab):
    assert d['G'] == f.A and d['neg_o'].shape[0] == 0 and d['sel_n'].shape[0] == 0, 'construction: kn is not 0'


def _v_nan_area(f, gt, d, lab):
    assert d['G'] == 2 and bool(torch.isnan(d['iou'][1]).all()) and int(d['best_a'][1]) == 0, 'construction: the IoU row is not all NaN / its arg-max not 0'


L = 'lhrcnn'
RPN_CASES = [
    # ---- the shared cases of edge_gt_cases.CASES, in this family's pixels
    LCase('one', [[30.3, 25.1, 20., 26., 1]]),
    LCase('dup_same_class', [[21., 22., 30., 16., 1], [21., 22., 30., 16., 1]]),
    LCase('dup_other_class', [[21., 22., 30., 16., 1], [21., 22., 30., 16., 2]]),
    LCase('reversed', None, note="image 1 = image 0's rows reversed, the same predictions for both"),
    LCase('one_px', lambda f: [[30.2 * _H(f) / 64, 31.7 * _W(f) / 64, 1., 1., 0]] + f.px([[10., 50., 20., 20., 1]])),
    LCase('sliver', lambda f: [[_H(f) / 2, 30. * _W(f) / 64, _H(f), 1., 0]]),
    LCase('whole_image', [[32., 32., 64., 64., 2]], note='every same-shape anchor ties for the best anchor'),
    LCase('partly_outside', [[2., 60., 20., 30., 0]]),
    LCase('centre_on_edge', lambda f: [[_H(f), 30. * _W(f) / 64, 10. * _H(f) / 64, 10. * _W(f) / 64, 0],
                                       [30. * _H(f) / 64, _W(f), 10. * _H(f) / 64, 10. * _W(f) / 64, 2]] + f.px([EG.ORD])),
    # ---- counts
    LCase('pad_minus_1', _crowd(6, 1), note='P = 7: six boxes, one pad row'),
    LCase('all_valid', _crowd(7, 2, min_at=4), verify=_v_all_valid, note='no pad row: G = the arg-min row, 4'),
    LCase('pad_128', _distinct_crowd(127, 3), pad=128, verify=_v_pad_128, note='P = LH_MAX_GT with 127 boxes (P - 1 boxes and one pad row at the limit): the last staged slot of s_g'),
    LCase('pad_129', _distinct_crowd(128, 4), pad=129, refused=(L,), note='one row more than the kernel stages: both entry points refuse, naming 128'),
    LCase('zero', lambda f: [], rejects=(L,), note='G = 0: the oracle raises on the reduction over no box; every anchor negative, the positive means 0 / 0'),
    LCase('zero_small', lambda f: [], shape='small', rejects=(L,), note='G = 0 with A < 256: counts[4] = A'),
    # ---- best rows
    LCase('no_overlap', _no_overlap_rows, verify=_v_no_overlap, note='IoU 0 everywhere: arg-max 0 < G, so the label is label[0] (tf.gather, :337)'),
    LCase('same_best_anchor', _collide_rows, verify=_v_same_best, note='two boxes claim one anchor: the positive list leads with a duplicate, the NMS drops it'),
    LCase('exact_anchor', lambda f: [f.anchor_row(f.candidates()[0])], verify=_v_exact, note='IoU 1 with one kept anchor'),
    # ---- thresholds
    LCase('iou05_below', lambda f: [f.threshold_row(0.5, 'below')[1]], verify=_v_threshold(0.5, 'below')),
    LCase('iou05_exact', lambda f: [f.threshold_row(0.5, 'exact')[1]], verify=_v_threshold(0.5, 'exact'), note='not positive: strict >'),
    LCase('iou05_above', lambda f: [f.threshold_row(0.5, 'above')[1]], verify=_v_threshold(0.5, 'above')),
    LCase('iou03_below', lambda f: [f.threshold_row(0.3, 'below')[1]], verify=_v_threshold(0.3, 'below')),
    LCase('iou03_exact', lambda f: [f.threshold_row(0.3, 'exact')[1]], verify=_v_threshold(0.3, 'exact'), note='not negative: strict <'),
    LCase('iou03_above', lambda f: [f.threshold_row(0.3, 'above')[1]], verify=_v_threshold(0.3, 'above')),
    # ---- caps
    LCase('many_positive', _many_positive_rows, pad=128, verify=_v_many_positive, note='120 copies of distinct anchors: n_pos > 128, k_pos = k_neg = 128'),
    LCase('few_negative', lambda f: [[_H(f) / 2, _W(f) / 2, _H(f), _W(f), 4]], shape='small', verify=_v_few_negative, note='A < 64: kn < 256 - kp'),
    LCase('no_negative', _every_anchor_rows, shape='small', pad=64, verify=_v_no_negative, note='a copy of every kept anchor: kn = 0, the negative mean 0 / 0'),
    # ---- anchor counts
    LCase('one_mid', [[30.3, 25.1, 20., 26., 1]], shape='mid', note='64 < A < 256: one pass of the ballot loop with idle lanes'),
    LCase('dup_mid', [[21., 22., 30., 16., 1], [21., 22., 30., 16., 2]], shape='mid'),
    LCase('one_small', [[30.3, 25.1, 20., 26., 1]], shape='small', note='A < 64, A % 64 != 0'),
    LCase('whole_image_small', [[32., 32., 64., 64., 2]], shape='small'),
    # ---- the out-of-operand write
    LCase('nan_area', lambda f: f.px([[30.3, 25.1, 20., 26., 1]]) + [[0.4 * _H(f), 0.5 * _W(f), math.inf, 0., 9]], verify=_v_nan_area,
          note='h * w = NaN: every IoU of the row is NaN.  The search used to keep bi = 0x7fffffff and write status[bi]; now anchor 0, as the arg-max'),
]
RPN_BY_NAME = {c.name: c for c in RPN_CASES}
assert sum(L in c.rejects for c in RPN_CASES) <= 2


def _status(f, d):
    st = torch.zeros(f.A, dtype=torch.uint8)
    G = d['G']
    st[d['neg_o']] = 2
    st[d['pos_a'][G:]] = 1
    st[d['best_a']] = 3
    return st


def banded_workspace(N, A, P, dev):
    """ops.lhrcnn_workspace's key set, every tensor between sentinel bands"""
    ops = _ops()
    meta = ops.lhrcnn_workspace(N, A, P, 'meta')
    bands = {k: Banded(tuple(v.shape), dev, v.dtype) for k, v in meta.items() if torch.is_tensor(v)}
    ws = {k: (bands[k].t if k in bands else v) for k, v in meta.items()}
    return bands, ws


def _run_rpn(f, x, gt, dev):
    ops = _ops()
    N, P = gt.shape[0], gt.shape[1]
    H, W = f.hw
    a = f.anc
    ad = dict(y1x1=a['y1x1'].to(dev), y2x2=a['y2x2'].to(dev), yx=a['yx'].to(dev), hw=a['hw'].to(dev),
              row=torch.nonzero(a['keep']).flatten().to(torch.int32).to(dev), A_full=f.A_full)
    out, ws = banded_workspace(N, f.A, P, dev)
    out['d_conf'] = Banded((N, f.A_full, 2), dev, init=5.0)
    out['d_bbox'] = Banded((N, f.A_full, 4), dev, init=5.0)
    cd, bd, gd = x['conf'].to(dev).contiguous(), x['bbox'].to(dev).contiguous(), gt.to(dev).contiguous()

    def chain():
        ops.lhrcnn_match(ad, cd, gd, ws)
        cap = ws['cap']
        counts = ws['counts'].view(-1)
        ops.nms_batched(ws['pos_box'], cap * 4, ws['pos_score'], cap, 1, ws['pos_valid'], cap, 1, 1, cap, N, counts[3:], 8, 0, 0.7, ws['sel_pos'], 128, ws['cnt_pos'])
        ops.nms_batched(ws['neg_box'], cap * 4, ws['neg_score'], cap, 1, ws['neg_valid'], cap, 1, 1, cap, N, counts[4:], 8, 0, 0.7, ws['sel_neg'], 256, ws['cnt_neg'])
        ops.lhrcnn_rpn_loss(ad, cd, bd, gd, ws, C_RPN, 1.0 / N, H, W, out['d_conf'].t, out['d_bbox'].t)
        _sync(dev)
    return out, ws, ad, cd, bd, gd, chain


def _oracle_rpn(f, x, gt, i):
    cf, bb = x['conf'][i].clone().requires_grad_(True), x['bbox'][i].clone().requires_grad_(True)
    keep = f.anc['keep']
    loss, pos_prop, pos_lab, truth, neg_prop, d = LR.rpn_one_image(bb[keep, :2], bb[keep, 2:], cf[keep], f.anc, gt[i], detail=True)
    g1, g2 = torch.autograd.grad(loss / gt.shape[0], [cf, bb], allow_unused=True)
    z = torch.zeros_like
    return dict(loss=loss.detach(), pos_prop=pos_prop.detach(), pos_lab=pos_lab, truth=truth.detach(), neg_prop=neg_prop.detach(), d=d,
                d_conf=z(cf) if g1 is None else g1, d_bbox=z(bb) if g2 is None else g2)


def _compare_image(f, gt, out, r, i):
    """the assertions of test_rpn_loss_chain_vs_oracle for one image, plus status, labels, validity flags and the NMS inputs"""
    H, W = f.hw
    d = r['d']
    G = d['G']
    what = (f.key, i)
    n_pos, n_neg = d['pos_a'].shape[0], d['neg_o'].shape[0]
    assert out['counts'][i].tolist() == [G, n_pos, n_neg, min(n_pos, 128), min(n_neg, 256 - min(n_pos, 128)), 0, 0, 0], (what, out['counts'][i].tolist(), G, n_pos, n_neg)
    assert torch.equal(out['status'][i], _status(f, d)), what
    assert torch.equal(out['pos_anchor'][i, :n_pos].long(), d['pos_a']) and torch.equal(out['pos_gt'][i, :n_pos].long(), d['pos_gi']), what
    assert torch.equal(out['neg_anchor'][i, :n_neg].long(), d['neg_o']), what
    label = gt[i, :G, 4].to(torch.int32)
    best_label = torch.where(d['best_a'] < G, label[d['best_a'].clamp(max=max(G - 1, 0))], torch.zeros_like(label))       # :337 with the GPU gather rule
    assert torch.equal(out['pos_label'][i, :n_pos], torch.cat([best_label, label[d['pos_gi'][G:]]])), what
    cap = out['pos_valid'].shape[1]
    assert torch.equal(out['pos_valid'][i].bool(), torch.arange(cap) < n_pos) and torch.equal(out['neg_valid'][i].bool(), torch.arange(cap) < n_neg), what
    a = f.anc

    def box(idx):
        return torch.cat([a['yx'][idx] - a['hw'][idx] / 2., a['yx'][idx] + a['hw'][idx] / 2.], -1)
    assert torch.equal(out['pos_box'][i, :n_pos], box(d['pos_a'])) and torch.equal(out['neg_box'][i, :n_neg], box(d['neg_o'])), what      # halving is exact
    pc = out['_conf'][i][a['keep']].double()
    _cmp(out['pos_score'][i, :n_pos], torch.softmax(pc[d['pos_a']], -1)[:, 0], 1e-5, 0., what + ('pos_score',))
    _cmp(out['neg_score'][i, :n_neg], torch.logsumexp(pc[d['neg_o']], -1) - pc[d['neg_o'], 1], 1e-5, 3e-7, what + ('neg_score',))      # (a cross entropy near 0 is the difference of two
    #                                                             f32 numbers of magnitude <= 1: a few times 6e-8 absolute)
    kp, kn = d['sel_p'].shape[0], d['sel_n'].shape[0]
    assert int(out['cnt_pos'][i]) == kp and int(out['cnt_neg'][i]) == kn, (what, int(out['cnt_pos'][i]), kp, int(out['cnt_neg'][i]), kn)
    assert torch.equal(out['sel_pos'][i, :kp].long(), d['sel_p']) and torch.equal(out['sel_neg'][i, :kn].long(), d['sel_n']), what
    _cmp(out['rpn_parts'][i, 3], r['loss'], 1e-5, 0., what + ('loss',))
    s = i * 256
    assert out['roi_counts'][i].tolist() == [kp, kn]
    lim = torch.tensor([H - 1., W - 1., H - 1., W - 1.])
    prop = torch.minimum(torch.clamp(torch.cat([r['pos_prop'], r['neg_prop']]), min=0.), lim)
    _cmp(out['roi_prop'][s: s + kp + kn], prop, 1e-5, 1e-3, what + ('roi_prop',))
    _cmp(out['roi_box'][s: s + kp + kn], prop / lim, 1e-5, 1e-5, what + ('roi_box',))
    _cmp(out['roi_truth'][s: s + kp], r['truth'], 1e-4, 1e-5, what + ('roi_truth',))
    assert bool((out['roi_truth'][s + kp: s + 256] == 0).all()) and bool((out['roi_prop'][s + kp + kn: s + 256] == 0).all()) \
        and bool((out['roi_box'][s + kp + kn: s + 256] == 0).all()), what
    assert torch.equal(out['roi_label'][s: s + kp].long(), r['pos_lab'].long()) and bool((out['roi_label'][s + kp: s + kp + kn] == C_RPN - 1).all()) \
        and bool((out['roi_label'][s + kp + kn: s + 256] == -1).all()), what
    assert bool((out['roi_img'][s: s + kp + kn] == i).all()) and bool((out['roi_img'][s + kp + kn: s + 256] == -1).all()), what
    assert out['roi_kind'][s: s + 256].tolist() == [1] * kp + [2] * kn + [0] * (256 - kp - kn), what


def check_rpn(name, dev):
    case = RPN_BY_NAME[name]
    f = family(case.shape)
    lo, hi = A_RANGE[case.shape]
    assert lo <= f.A <= hi and (case.shape != 'small' or f.A % 64 != 0), (case.shape, f.A)       # a change of the anchor rules must not void the shapes
    dev = _dev(dev)
    gt = f.gt(case)
    x = f.inputs()
    if name == 'reversed':
        for t in x.values():
            t[EDGE] = t[0]
    bands, ws, ad, cd, bd, gd, chain = _run_rpn(f, x, gt, dev)
    what = f'lhrcnn/rpn/{name}'
    if L in case.refused:
        from odtk import _lib
        ops = _ops()
        before = _host(bands)
        for call in (lambda: ops.lhrcnn_match(ad, cd, gd, ws), lambda: ops.lhrcnn_rpn_loss(ad, cd, bd, gd, ws, C_RPN, 0.5, f.hw[0], f.hw[1], bands['d_conf'].t, bands['d_bbox'].t)):
            try:
                call()
            except _lib.OdtkError as e:
                assert str(LH_MAX_GT) in str(e) and str(gt.shape[1]) in str(e), f'{what}: the refusal does not name the limit: {e}'
            else:
                raise AssertionError(f'{what}: the call was not refused')
        _sync(dev)
        _intact(bands, what)
        _same_bits(before, _host(bands), what + ' (a refused call wrote to an operand)')
        return None
    chain()
    _intact(bands, what)
    out = _host(bands)
    out['_conf'] = x['conf']
    refs = []
    for i in range(2):
        try:
            refs.append(_oracle_rpn(f, x, gt, i))
        except f.rejects_on as e:
            assert i == EDGE and L in case.rejects, f'{what}: the oracle rejects image {i} ({type(e).__name__}: {e}) and the table does not say so'
            refs.append(None)
    if L in case.rejects:
        assert refs[EDGE] is None, f'{what}: marked rejects, but the oracle accepts it'
    for i, r in enumerate(refs):
        if r is not None:
            _compare_image(f, gt, out, r, i)
    live = [i for i, r in enumerate(refs) if r is not None]
    for key in ('d_conf', 'd_bbox'):
        _rel_where_finite(out[key][live], torch.stack([refs[i][key] for i in live]), 1e-5, (what, key))
        for i in live:                                            # fully written: exactly 0 wherever the reference gradient is 0
            zero = refs[i][key] == 0
            assert bool((out[key][i][zero] == 0).all()), (what, key, i, 'not written / not zero where the reference gradient is zero')
    if case.verify is not None:
        case.verify(f, gt, refs[EDGE]['d'], refs[EDGE]['pos_lab'])
    if name == 'reversed':
        assert torch.equal(out['status'][EDGE], out['status'][0]) and out['counts'][EDGE].tolist() == out['counts'][0].tolist()
        _cmp(out['rpn_parts'][EDGE, 3], out['rpn_parts'][0, 3], 1e-5, 0., what)
    if name == 'nan_area':
        assert int(out['counts'][EDGE, 0]) == 2 and int(out['status'][EDGE, 0]) == 3
    if refs[EDGE] is None:                                        # G = 0
        A = f.A
        assert out['counts'][EDGE].tolist()[:5] == [0, 0, A, 0, min(A, 256)], out['counts'][EDGE].tolist()
        assert bool((out['status'][EDGE] == 2).all()) and int(out['cnt_pos'][EDGE]) == 0
        p = out['rpn_parts'][EDGE]
        assert math.isfinite(float(p[0])) and all(_kind(float(v)) == 'nan' for v in p[1:]), p.tolist()      # means over no positive: 0 / 0
        for key in ('d_conf', 'd_bbox'):
            assert bool((out[key][EDGE] != 5.0).all()), (what, key, 'not fully written')
    chain()
    _intact(bands, what + ' (second run)')
    again = _host(bands)
    again['_conf'] = x['conf']
    _same_bits(out, again, what)
    return out


# ================================================================================================================== R-CNN loss
RCNN_CASES = {                      # name -> (per-image (kp, kn), C, ldl, ldb)
    'empty_image': ([(5, 40), (0, 0), (3, 2)], 21, 24, 8),
    'no_positive': ([(0, 5), (0, 256), (0, 1)], 21, 24, 8),          # the box part is 0 / 0 in every image
    'full_and_single': ([(128, 128), (1, 0), (128, 0)], 21, 24, 8),
    'tight_pitch': ([(7, 9), (2, 30)], 21, 21, 4),
    'two_classes': ([(4, 6), (1, 1)], 2, 8, 8),
    'inf_truth': ([(6, 10), (3, 4)], 21, 24, 8),                     # roi_truth +-inf (pr_y == 0): loss inf, gradient -+1 * w
}


def check_rcnn(name, dev):
    ops = _ops()
    dev = _dev(dev)
    counts, C, ldl, ldb = RCNN_CASES[name]
    N = len(counts)
    g = torch.Generator().manual_seed(len(name) * 7 + N)
    R = N * 256
    kind = torch.zeros(R, dtype=torch.int32)
    label = torch.full((R,), -1, dtype=torch.int32)
    for i, (kp, kn) in enumerate(counts):
        s = i * 256
        kind[s: s + kp] = 1
        kind[s + kp: s + kp + kn] = 2
        label[s: s + kp] = torch.randint(0, C - 1, (kp,), generator=g).to(torch.int32)
        label[s + kp: s + kp + kn] = C - 1
        if kp > 1:
            label[s], label[s + 1] = 0, C - 1                                 # the first and the last class on positive rows
        elif kp == 1:
            label[s] = 0
    truth = torch.randn(R, 4, generator=g)
    logits = torch.full((R, ldl), 31.0)
    logits[:, :C] = torch.randn(R, C, generator=g) * 2
    live_rows = torch.nonzero(kind != 0).flatten()
    if live_rows.numel():                                                     # two equal maximal logits: one row on its label, one row beside it
        r0 = int(live_rows[0])
        logits[r0, :C] = -1.0
        logits[r0, int(label[r0])] = 3.0
        logits[r0, (int(label[r0]) + 1) % C] = 3.0
        r1 = int(live_rows[-1])
        logits[r1, :C] = 0.5
    pbbox = torch.full((R, ldb), 17.0)
    pbbox[:, :4] = torch.randn(R, 4, generator=g) * 1.5
    if name == 'inf_truth':
        truth[0, 0], truth[1, 1], truth[256, 0] = math.inf, -math.inf, -math.inf
    bands, ws = banded_workspace(N, 100, 4, dev)
    ws['roi_kind'].copy_(kind)
    ws['roi_label'].copy_(label)
    ws['roi_truth'].copy_(truth)
    ws['roi_counts'].copy_(torch.tensor(counts, dtype=torch.int32))
    out = dict(rcnn_parts=bands['rcnn_parts'], d_logits=Banded((R, ldl), dev, init=4.0), d_pbbox=Banded((R, ldb), dev, init=4.0))
    ld, pd = logits.to(dev), pbbox.to(dev)

    def launch():
        ops.lhrcnn_rcnn_loss(ld, ldl, pd, ldb, N, C, ws, 1.0, out['d_logits'].t, out['d_pbbox'].t)
        _sync(dev)
    what = f'lhrcnn/rcnn/{name}'
    launch()
    _intact(bands, what)
    _intact(out, what)
    got = _host(out)
    # float64 restatement of :167-170: mean cross entropy over all live rows of the batch + mean smooth L1 (summed over the 4 codes) over its positive rows
    z, b, t = logits[:, :C].double(), pbbox[:, :4].double(), truth.double()
    live, pos = kind != 0, kind == 1
    rows, npos = int(live.sum()), int(pos.sum())
    lab = label.clamp(min=0).long()
    ce = (torch.logsumexp(z, 1) - z.gather(1, lab.view(-1, 1)).squeeze(1)) * live
    dl = (torch.softmax(z, 1) - torch.nn.functional.one_hot(lab, C)) * live.view(-1, 1) / rows
    dd = b - t
    box = torch.where(dd.abs() < 1, 0.5 * dd * dd, dd.abs() - 0.5).sum(-1)
    box = torch.where(pos, box, torch.zeros_like(box))
    db = torch.where(dd.abs() < 1, dd, torch.sign(dd)) * pos.view(-1, 1)
    nan = torch.tensor(math.nan, dtype=torch.float64)
    db = db / npos if npos else torch.where(pos.view(-1, 1), nan, torch.zeros_like(db))
    for i in range(N):
        s = slice(i * 256, i * 256 + 256)
        _cmp(got['rcnn_parts'][i, 0], ce[s].sum() / rows, 1e-5, 0., (what, 'ce', i))
        _cmp(got['rcnn_parts'][i, 1], box[s].sum() / npos if npos else nan, 1e-5, 0., (what, 'box', i))
    _rel_where_finite(got['d_logits'][:, :C], dl, 1e-5, (what, 'd_logits'))
    _rel_where_finite(got['d_pbbox'][:, :4], db, 1e-5, (what, 'd_pbbox'))
    assert bool((got['d_logits'][:, :C][~live] == 0).all()) and bool((got['d_pbbox'][:, :4][~pos] == 0).all()), (what, 'rows without a loss must be written 0')
    assert bool((got['d_logits'][:, C:] == 0).all()) and bool((got['d_pbbox'][:, 4:] == 0).all()), (what, 'pad columns must be written 0')
    if name == 'inf_truth':
        w = 1.0 / npos
        assert _kind(float(got['rcnn_parts'][0, 1])) == '+inf' and _kind(float(got['rcnn_parts'][1, 1])) == '+inf'
        assert abs(float(got['d_pbbox'][0, 0]) + w) < 1e-6 * w and abs(float(got['d_pbbox'][1, 1]) - w) < 1e-6 * w and abs(float(got['d_pbbox'][256, 0]) - w) < 1e-6 * w
    if name == 'no_positive':
        assert all(_kind(float(v)) == 'nan' for v in got['rcnn_parts'][:, 1])
    launch()
    _intact(out, what)
    _same_bits(got, _host(out), what)
    return got


# ================================================================================================================== decode kernels
def check_rpn_decode(shape, dev):
    ops = _ops()
    dev = _dev(dev)
    f = family(shape)
    H, W = f.hw
    g = torch.Generator().manual_seed(f.A)
    conf, bbox = torch.randn(f.A_full, 2, generator=g) * 2, torch.randn(f.A_full, 4, generator=g) * 0.4
    row = torch.nonzero(f.anc['keep']).flatten()
    A = f.A
    plant = {0: [-40., 0., 0., 0.], 1: [40., 0., 0., 0.], 2: [0., -40., 0., 0.], 3: [0., 40., 0., 0.],      # wholly above / below / left / right of the picture
             A - 1: [0.1, -0.2, 100., 0.3], A - 2: [0., 0., 0.2, 100.], A // 2: [30., -30., 100., 100.]}     # expf overflows to inf
    for i, v in plant.items():
        bbox[row[i]] = torch.tensor(v)
    out = dict(prop=Banded((A, 4), dev, init=9.), score=Banded((A,), dev, init=9.))
    a = f.anc
    ad = dict(yx=a['yx'].to(dev), hw=a['hw'].to(dev), row=row.to(torch.int32).to(dev), A_full=f.A_full)
    cd, bd = conf.to(dev), bbox.to(dev)

    def launch():
        ops.lhrcnn_rpn_decode(ad, cd, bd, H, W, out['prop'].t, out['score'].t)
        _sync(dev)
    what = f'lhrcnn/rpn_decode/{shape}'
    launch()
    _intact(out, what)
    got = _host(out)
    b, yx0, hw0 = bbox[row].double(), a['yx'].double(), a['hw'].double()
    yx, hw = b[:, :2] * hw0 + yx0, torch.exp(b[:, 2:]) * hw0                                                 # :134-136 of the reference, in float64
    lim = torch.tensor([H - 1., W - 1., H - 1., W - 1.], dtype=torch.float64)
    ref = torch.minimum(torch.clamp(torch.cat([yx - hw / 2., yx + hw / 2.], -1), min=0.), lim)
    _cmp(got['prop'], ref, 1e-5, 1e-3, (what, 'prop'))
    _cmp(got['score'], torch.softmax(conf[row].double(), -1)[:, 0], 1e-5, 0., (what, 'score'))
    for i, (lo, hi, v) in {0: (0, 2, 0.), 1: (0, 2, H - 1.), 2: (1, 3, 0.), 3: (1, 3, W - 1.)}.items():      # clamped to zero height / width, exactly
        assert float(got['prop'][i, lo]) == v and float(got['prop'][i, hi]) == v, (what, i, got['prop'][i].tolist())
    assert got['prop'][A - 1, 0::2].tolist() == [0., H - 1.] and got['prop'][A - 2, 1::2].tolist() == [0., W - 1.], what
    assert got['prop'][A // 2].tolist() == [0., 0., H - 1., W - 1.], what
    launch()
    _same_bits(got, _host(out), what)
    return got


def check_gather_rois(cnt, dev):
    ops = _ops()
    dev = _dev(dev)
    cap, A, H, W = 300, 411, 320, 416
    n = {'0': 0, '1': 1, 'cap': cap, 'cap+5': cap + 5}[cnt]
    g = torch.Generator().manual_seed(n + 1)
    prop = torch.rand(A, 4, generator=g) * torch.tensor([H - 1., W - 1., H - 1., W - 1.])
    sel = torch.full((cap + 5,), A - 1, dtype=torch.int32)                                                  # (cnt > cap: the five rows past cap stay readable)
    sel[:cap] = torch.randperm(A, generator=g)[:cap].to(torch.int32)
    out = dict(roi_box=Banded((cap, 4), dev, init=9.), roi_prop=Banded((cap, 4), dev, init=9.), roi_img=Banded((cap,), dev, torch.int32, init=9))
    pd, sd, cd = prop.to(dev), sel.to(dev), torch.tensor([n], dtype=torch.int32).to(dev)

    def launch():
        ops.lhrcnn_gather_rois(pd, sd, cd, H, W, out['roi_box'].t, out['roi_prop'].t, out['roi_img'].t)
        _sync(dev)
    what = f'lhrcnn/gather_rois/{cnt}'
    launch()
    _intact(out, what)
    got = _host(out)
    k = min(n, cap)
    ref = torch.zeros(cap, 4)
    ref[:k] = prop[sel[:k].long()]
    assert torch.equal(got['roi_prop'], ref), what                                                          # copies, and one IEEE division: exact
    assert torch.equal(got['roi_box'], ref / torch.tensor([H - 1., W - 1., H - 1., W - 1.])), what
    assert got['roi_img'].tolist() == [0] * k + [-1] * (cap - k), what
    launch()
    _same_bits(got, _host(out), what)
    return got


def _ulp32(v):
    return float(np.spacing(np.float32(v)))


def check_rcnn_decode(R, dev):
    ops = _ops()
    dev = _dev(dev)
    C, ldl, ldb, H, W = 21, 24, 8, 320, 416
    nc = C - 1
    g = torch.Generator().manual_seed(R)
    logits = torch.full((R, ldl), 50.0)                                                                      # pad columns would win every arg-max if they were read
    logits[:, :C] = torch.randn(R, C, generator=g) * 2
    pbbox = torch.full((R, ldb), 50.0)
    pbbox[:, :4] = torch.randn(R, 4, generator=g) * 0.5
    y1, x1 = torch.rand(R, generator=g) * (H - 40), torch.rand(R, generator=g) * (W - 40)
    prop = torch.stack([y1, x1, y1 + 4 + torch.rand(R, generator=g) * 30, x1 + 4 + torch.rand(R, generator=g) * 30], 1)
    img = torch.zeros(R, dtype=torch.int32)
    # the softmax of a row whose three largest logits are equal and whose others are so small that expf underflows to 0 is 1 / 3 in f32 exactly as the
    # kernel evaluates it: expf(0) = 1, se = 1 + 1 + 1, p = 1.f / 3.f (one correctly rounded division).  thr is that number.
    one = np.float32(1.0)
    thr = float(one / (one + one + one))
    rows = {}
    if R >= 255:
        rows = dict(eq_thr=3, tie_first=5, tie_mid=6, bg_wins=7, tie_all=8, dead_first=0, dead_mid=100, dead_last=R - 1, flat_h=9, flat_w=10, big_h=11)
        logits[rows['eq_thr'], :C] = -200.
        logits[rows['eq_thr'], [2, 11, 19]] = 4.
        logits[rows['tie_first'], :C] = -3.
        logits[rows['tie_first'], [0, nc]] = 2.                          # class 0 (the start value of the search) ties with the background: class 0 wins
        logits[rows['tie_mid'], :C] = -3.
        logits[rows['tie_mid'], [13, nc]] = 2.                           # a later class ties with the background: the class wins
        logits[rows['bg_wins'], :C] = -3.
        logits[rows['bg_wins'], nc] = 2.0000002
        logits[rows['bg_wins'], 13] = 2.                                 # the background one ulp ahead: dropped although p[13] >= thr
        logits[rows['tie_all'], :C] = 0.25
        for k in ('dead_first', 'dead_mid', 'dead_last'):
            img[rows[k]] = -1
        prop[rows['flat_h']] = torch.tensor([0., 10., 0., 50.])          # proposals clamped to zero height / width
        prop[rows['flat_w']] = torch.tensor([20., W - 1., 90., W - 1.])
        pbbox[rows['big_h'], 2] = 100.                                   # expf overflows: +-inf edges
    else:
        logits[0, :C] = -200.
        logits[0, [2, 11, 19]] = 4.
        rows = dict(eq_thr=0)
    out = dict(conf=Banded((R, nc), dev, init=9.), boxes=Banded((R, 4), dev, init=9.), cand=Banded((R, nc), dev, torch.uint8, init=9))
    ld, pd, qd, idv = logits.to(dev), pbbox.to(dev), prop.to(dev), img.to(dev)

    def launch():
        ops.lhrcnn_rcnn_decode(ld, ldl, pd, ldb, qd, idv, C, thr, out['conf'].t, out['boxes'].t, out['cand'].t)
        _sync(dev)
    what = f'lhrcnn/rcnn_decode/{R}'
    launch()
    _intact(out, what)
    got = _host(out)
    live = img >= 0
    z = logits[:, :C].double()
    p = torch.softmax(z, -1)
    fg = torch.argmax(z, -1) < nc                                         # torch's arg-max returns the first maximum, as the reference's
    ref_conf = p[:, :nc] * live.view(-1, 1)
    _cmp(got['conf'], ref_conf, 1e-5, 1.2e-38, (what, 'conf'))              # (below the smallest normal f32 the kernel's expf gives 0)
    want = (fg & live).view(-1, 1) & (ref_conf >= thr)
    near = ((ref_conf - thr).abs() <= _ulp32(thr)) & (fg & live).view(-1, 1)       # within one f32 ulp of the threshold: the f32 value decides
    near_rows = torch.nonzero(near.any(1)).flatten().tolist()
    assert near_rows == [rows['eq_thr']], (what, 'rows within 1 ulp of thr', near_rows)
    assert len(near_rows) <= max(1, R // 100), what
    assert torch.equal(got['cand'][~near].bool(), want[~near]) and bool((got['cand'] <= 1).all()), what
    e = rows['eq_thr']
    assert got['cand'][e].nonzero().flatten().tolist() == [2, 11, 19] and all(float(got['conf'][e, c]) == thr for c in (2, 11, 19)), (what, 'p == thr must be a candidate')
    q, t = prop.double(), pbbox[:, :4].double()
    pyx, phw = q[:, 0:2] / 2. + q[:, 2:4] / 2., q[:, 2:4] - q[:, 0:2]
    ex = torch.exp(t[:, 2:4])
    ex = torch.where(ex > torch.finfo(torch.float32).max, torch.full_like(ex, math.inf), ex)                 # expf's overflow is a property of the f32 format
    yx, hw = t[:, 0:2] * phw + pyx, phw * ex
    ref_box = torch.cat([yx - hw / 2., yx + hw / 2.], -1) * live.view(-1, 1)
    mag = (yx.abs() + hw.abs() / 2.).repeat(1, 2)
    fin = torch.isfinite(ref_box)
    err = (got['boxes'].double() - ref_box).abs()
    assert bool((err[fin] <= 1e-5 * mag[fin] + 1e-6).all()), (what, 'boxes', float(err[fin].max()))
    for j in torch.nonzero(~fin).tolist():
        assert _kind(float(got['boxes'][j[0], j[1]])) == _kind(float(ref_box[j[0], j[1]])), (what, j)
    if R >= 255:
        for k in ('dead_first', 'dead_mid', 'dead_last'):
            r = rows[k]
            assert bool((got['conf'][r] == 0).all()) and bool((got['cand'][r] == 0).all()) and bool((got['boxes'][r] == 0).all()), (what, k)
        assert got['cand'][rows['tie_first']].nonzero().flatten().tolist() == [0] and got['cand'][rows['tie_mid']].nonzero().flatten().tolist() == [13], what
        assert int(got['cand'][rows['bg_wins']].sum()) == 0 and float(got['conf'][rows['bg_wins'], 13]) >= thr, what
        assert int(got['cand'][rows['tie_all']].sum()) == 0                 # every class at 1 / 21 < thr; arg-max 0 is a class
        assert float(got['boxes'][rows['flat_h'], 0]) == float(got['boxes'][rows['flat_h'], 2]) == 0.0, what
        assert float(got['boxes'][rows['flat_w'], 1]) == float(got['boxes'][rows['flat_w'], 3]) == W - 1., what
        assert got['boxes'][rows['big_h'], 0::2].tolist() == [-math.inf, math.inf], what
    launch()
    _same_bits(got, _host(out), what)
    return got


# ================================================================================================================== crop_and_resize
CROP_CASES = {                     # name -> (crop, H, W, C, every box in one image)
    'c7_490': (7, 5, 6, 490, False), 'c7_1': (7, 5, 6, 1, False), 'c2_7': (2, 5, 6, 7, False), 'c1_7': (1, 5, 6, 7, False), 'c1_1': (1, 5, 6, 1, False),
    'c1_490': (1, 4, 3, 490, False), 'c7_h1': (7, 1, 6, 7, False), 'c2_w1': (2, 5, 1, 1, False), 'c1_h1w1': (1, 1, 1, 7, False), 'c7_one_image': (7, 5, 6, 7, True),
    'c2_one_image': (2, 3, 4, 490, True),
}
OUTSIDE = [1.5, 1.5, 2.0, 2.5]


def check_crop(name, dt, dev):
    ops = _ops()
    dev = _dev(dev)
    crop, H, W, C, one_image = CROP_CASES[name]
    dtype = torch.float32 if dt == 'f32' else torch.bfloat16
    N = 2
    g = torch.Generator().manual_seed(crop * 1000 + H * 100 + W * 10 + C)
    ld = ops.pad_to(C, 8) + 8
    feat = torch.full((N * H * W, ld), 21.0, dtype=dtype)
    feat[:, :C] = torch.randn(N * H * W, C, generator=g).to(dtype)
    nr = 30 if one_image else 8
    y1, x1 = torch.rand(nr, generator=g) * 0.8 - 0.15, torch.rand(nr, generator=g) * 0.8 - 0.15                 # some start / end outside [0, 1]
    rnd = torch.stack([y1, x1, y1 + 0.05 + torch.rand(nr, generator=g) * 0.6, x1 + 0.05 + torch.rand(nr, generator=g) * 0.6], 1)
    fixed = torch.tensor([[0.1, 0.2, 0.7, 0.9],                     # 0: box_img = -1, the first row
                          [0.8, 0.1, 0.2, 0.9],                     # 1: reversed, y1 > y2
                          [0., 0., 1., 1.],                         # 2: the whole picture
                          [1., 1., 1., 1.],                         # 3: zero size on the bottom-right corner
                          OUTSIDE,                                  # 4: wholly outside
                          [-1.0, -1.0, -0.5, -0.2],                 # 5: wholly outside, the other way
                          [math.nan, 0.1, 0.5, 0.5],                # 6: NaN: a zero row, no gradient
                          [0.25, 0.5, 0.25, 0.5]])                  # 7: zero size inside
    boxes = torch.cat([fixed, rnd, torch.tensor([[0.2, 0.1, 0.9, 0.6]])])                                       # last: box_img = -1
    R = boxes.shape[0]
    img = torch.full((R,), N - 1, dtype=torch.int32) if one_image else torch.randint(0, N, (R,), generator=g).to(torch.int32)
    img[0] = -1
    img[R - 1] = -1
    n_out = crop * crop * C
    ldo = ops.pad_to(n_out, 8) + 8
    dout = torch.full((R, ldo), 23.0, dtype=dtype)
    dout[:, :n_out] = torch.randn(R, n_out, generator=g).to(dtype)
    # reference: the picture in float64, the sample positions in f32 as LR.crop_and_resize computes them.  Its index arithmetic cannot take a NaN box
    # (NaN -> int64); that box is, as in tf.image.crop_and_resize, a zero row without a gradient: the reference row is masked like an empty one
    f4 = feat[:, :C].double().reshape(N, H, W, C).requires_grad_(True)
    rb = boxes.clone()
    rb[6] = torch.tensor([0., 0., 1., 1.])
    live = (img >= 0).view(-1, 1).clone()
    live[6] = False
    ref = LR.crop_and_resize(f4, rb, img.clamp(min=0), crop).reshape(R, -1) * live
    gref, = torch.autograd.grad(ref, f4, dout[:, :n_out].double())
    out = dict(out=Banded((R, ldo), dev, dtype, init=3.0), dfeat=Banded((N * H * W, ld), dev, init=9.0))
    fd, bd, idv, dd = feat.to(dev), boxes.to(dev), img.to(dev), dout.to(dev)

    def launch():
        ops.crop_and_resize_fwd(fd, ld, N, H, W, C, bd, idv, crop, out['out'].t, ldo)
        ops.crop_and_resize_bwd(dd, ldo, N, H, W, C, bd, idv, crop, out['dfeat'].t, ld)
        _sync(dev)
    what = f'lhrcnn/crop/{name}/{dt}'
    launch()
    _intact(out, what)
    got = _host(out)

    def rel(a, b):
        return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))
    tol = 1e-5 if dt == 'f32' else 1e-2
    e_out, e_grad = rel(got['out'][:, :n_out], ref.detach()), rel(got['dfeat'][:, :C], gref.reshape(-1, C))
    assert e_out < tol, (what, 'out', e_out)
    assert e_grad < 1e-4, (what, 'dfeat', e_grad)
    assert bool((got['out'][:, n_out:].float() == 3.0).all()), (what, 'forward pad columns touched')
    assert bool((got['dfeat'][:, C:] == 0).all()), (what, 'backward pad columns not zero')
    zero_rows = set(torch.nonzero((ref.detach() == 0).all(1)).flatten().tolist())
    assert {0, 6, R - 1} <= zero_rows and (H * W == 1 or {4, 5} <= zero_rows), (what, sorted(zero_rows))
    for r in zero_rows:
        assert bool((got['out'][r, :n_out].float() == 0).all()), (what, 'row', r, 'must be zero')
    if one_image:
        assert bool((got['dfeat'][: H * W] == 0).all()), (what, 'gradient in the image without a box')
    first = got
    launch()
    _intact(out, what)
    again = _host(out)
    assert torch.equal(first['out'].float(), again['out'].float()), (what, 'forward: two runs differ')
    assert rel(again['dfeat'][:, :C], first['dfeat'][:, :C]) < 1e-4 or float(first['dfeat'][:, :C].abs().max()) == 0.0, (what, 'backward: two runs differ')
    return got


# ================================================================================================================== the table
PARAMS = [('rpn', c.name) for c in RPN_CASES] + [('rcnn', n) for n in RCNN_CASES] \
    + [('rpn_decode', s) for s in ('big', 'mid', 'small')] + [('gather_rois', c) for c in ('0', '1', 'cap', 'cap+5')] + [('rcnn_decode', str(r)) for r in (1, 255, 257)] \
    + [('crop_' + dt, n) for n in CROP_CASES for dt in ('f32', 'bf16')]


def check(group, name, dev):
    if group == 'rpn':
        return check_rpn(name, dev)
    if group == 'rcnn':
        return check_rcnn(name, dev)
    if group == 'rpn_decode':
        return check_rpn_decode(name, dev)
    if group == 'gather_rois':
        return check_gather_rois(name, dev)
    if group == 'rcnn_decode':
        return check_rcnn_decode(int(name), dev)
    if group.startswith('crop_'):
        return check_crop(name, group[5:], dev)
    raise KeyError(group)
