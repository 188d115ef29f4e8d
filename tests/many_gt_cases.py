"""Crowded images: more than 128 and up to 1 024 ground-truth rows per image through the matching and loss kernels of csrc/boxes.hip, retina.hip,
refinedet.hip and dense_heads.hip -- the case bodies shared by tests/test_cpu_many_gt.py (the kernel source under the fiber emulation) and
tests/test_gpu_many_gt.py (libodtk.so on the device).  The harness is tests/edge_gt_cases.py's: its FAMILIES (run, oracle, loss_tol, grad_tol, check_ints,
inputs at N = 2: 64 x 64 for CenterNet / FCOS, 32 x 32 for YOLOv3, 300^2 for SSD, 320 x 256 for RetinaNet, 320^2 for RefineDet), Banded, _crowd and Case.
Image 0 carries the family's ordinary row set, image 1 (the last one) the case; every operand lies between two bands of sentinels.

Comparison rules of check(family, case, dev):
  * integer outputs (ngt, best, status, rgindex, counts; RefineDet: the mined rows too) equal the oracle's at EVERY position (family.check_ints);
  * losses and gradients: the family's existing tolerance (FAMILIES[...].loss_tol / grad_tol, quoted in its .tol).  No case needed a wider one: the
    "bound" column of the table below is that tolerance for every row;
  * pad_1025: the call is refused with an OdtkError naming 1025 and 1024, every operand and band keeps what it held.

Seeds.  A thousand random boxes make near-tied IoUs likely, and a tie that the last bit breaks is no kernel error.  A seed qualifies for a case only if
the oracle's own integer outputs (box count, best anchor per box, positive / negative / ignored / best per anchor, arg-max box per anchor) are the same
with the match evaluated in float32 and in float64 on the same (float32) inputs: build() asserts it for the three anchor families on the CPU, for both
images, before anything is launched.  About one random box in twenty lies wholly inside several priors of one shape, whose IoUs with it differ in the
last bit only, so no plain seed qualifies at these counts: the rows that tie take the same row of another seed's draw (REDRAWS, found once by
tools/many_gt_redraws.py and kept in tests/golden/many_gt_redraws.json), and the assertion runs on the result.  The dense families' kernels return no
integer output; their cases are the plain draws.

    case            pad   boxes  ground truth of image 1                                                             bound
    pad_129         129   128    random crowd: one row past the old capacity                                         family tolerance
    pad_257         257   256    random crowd: past a second multiple of 128                                         family tolerance
    pad_1024        1024  1023   random crowd: the last slot at the limit                                            family tolerance
    all_valid_1024  1024  700    1 024 boxes, the smallest yc at row 700: G = 700 by the arg-min rule                family tolerance
    late_owner      200   199    small boxes in the upper left quarter; row 150 the only box that matches well       family tolerance
                                 (an exact prior for the anchor families, the only box over its cells for the dense ones)
    dup_across      231   230    random crowd; rows 5 and 200 hold the same box                                      family tolerance
    pad_1025        1025  100    refused
"""
import json
import os

import torch

import edge_gt_cases as EG
from edge_gt_cases import ANCHOR, EDGE, FAMILIES, Banded, Case, _crowd
from oracle import refinedet_ref as DR
from oracle import retinanet_ref as RR
from oracle import ssd300_ref as SR

IN_SCOPE = ('ssd', 'retinanet', 'refinedet', 'centernet', 'fcos', 'yolov3')
LIMIT = 1024
MATCH = {'ssd': SR.match, 'retinanet': RR.match, 'refinedet': DR.match}
LATE, DUP_A, DUP_B = 150, 5, 200
OWNER_BOX = [48., 48., 16., 16., 1]          # dense late_owner: canvas units; the others stay inside [0, 32) x [0, 32)


def _small_upper_left(n, seed, lo, hi):
    """n boxes of lo .. hi canvas units whose extents stay inside the upper left quarter of the canvas"""
    g = torch.Generator().manual_seed(seed)
    h = torch.rand(n, generator=g) * (hi - lo) + lo
    w = torch.rand(n, generator=g) * (hi - lo) + lo
    return torch.stack([h / 2 + torch.rand(n, generator=g) * (30 - h), w / 2 + torch.rand(n, generator=g) * (30 - w), h, w,
                        torch.randint(0, 20, (n,), generator=g).float()], 1).tolist()


def _late_owner(seed):
    def rows(fam):
        # anchor families: at most 3 canvas units a side, under a fifth of the area of the smallest prior (30 px squares in 300, 32 px in 320), so that
        # none of them has an IoU above 0.4 with any prior
        return fam.px(_small_upper_left(199, seed, 1., 3.) if fam.name in ANCHOR else _small_upper_left(199, seed, 2., 8.))
    return rows


# name -> (seed -> rows(fam)), seed of the case, rows that are written after the draw and never redrawn
DRAWS = {
    'pad_129': (lambda s: _crowd(128, s), 11, ()),
    'pad_257': (lambda s: _crowd(256, s), 12, ()),
    'pad_1024': (lambda s: _crowd(1023, s), 13, ()),
    'all_valid_1024': (lambda s: _crowd(1024, s, min_at=700), 14, (700,)),
    'late_owner': (_late_owner, 15, (LATE,)),
    'dup_across': (lambda s: _crowd(230, s), 16, (DUP_A, DUP_B)),
    'pad_1025': (lambda s: _crowd(100, s), 17, ()),
}
# "<family>/<case>" -> [[row, seed], ...]: rows of the anchor families' draws that left a tie to the last bit (the oracle's float32 and float64 matches
# disagreed on an integer) and take the same row of another seed's draw instead.  Written by tools/many_gt_redraws.py; build() asserts the result.
REDRAWS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'many_gt_redraws.json')
REDRAWS = json.load(open(REDRAWS_FILE)) if os.path.exists(REDRAWS_FILE) else {}


def _rows_of(name, redraws=None):
    draw, seed, _ = DRAWS[name]

    def rows(fam):
        r = draw(seed)(fam)
        for row, s in (REDRAWS.get(f'{fam.name}/{name}', []) if redraws is None else redraws):
            r[row] = draw(s)(fam)[row]
        if name == 'late_owner':
            r[LATE] = fam.prior_row(fam.candidates()[0]) if fam.name in ANCHOR else fam.px([OWNER_BOX])[0]
        if name == 'dup_across':
            if fam.name in ANCHOR:                  # a box that owns anchors: one prior, slightly moved
                yc, xc, h, w, _ = fam.prior_row(fam.candidates()[0])
                r[DUP_A] = [yc + 1.0, xc + 0.5, h * 1.04, w * 0.97, 2]
            r[DUP_B] = list(r[DUP_A])
        return r
    return rows


CASES = [
    Case('pad_129', _rows_of('pad_129'), pad=129, note='128 boxes in 129 rows: one past the old capacity'),
    Case('pad_257', _rows_of('pad_257'), pad=257, note='256 boxes in 257 rows'),
    Case('pad_1024', _rows_of('pad_1024'), pad=1024, note='1 023 boxes in 1 024 rows: the last slot at the limit'),
    Case('all_valid_1024', _rows_of('all_valid_1024'), pad=1024, note='no pad row: G = 700 by the arg-min rule, rows 700.. ignored'),
    Case('late_owner', _rows_of('late_owner'), pad=200, note='the only box that matches well sits at row 150'),
    Case('dup_across', _rows_of('dup_across'), pad=231, note='the same box at rows 5 and 200'),
    Case('pad_1025', _rows_of('pad_1025'), pad=1025, refused=IN_SCOPE, note='one row more than the limit: refused'),
]
BY_NAME = {c.name: c for c in CASES}
PARAMS = [(f, c.name) for f in IN_SCOPE for c in CASES]


def _ints(mt):
    """the integer outputs of a family's match(), whichever names it gives them"""
    out = dict(G=mt['G'], best=mt['best'].tolist(), rgindex=mt['rgindex'].tolist())
    if 'status' in mt:
        out['status'] = mt['status'].tolist()
    else:
        out['other'], out['pos'] = mt['othermask'].tolist(), mt['pos'].tolist()
        if 'neg' in mt:
            out['neg'] = mt['neg'].tolist()
    return out


_BUILT = {}


def build(family, name):
    """(family object, case, ground truth [2, pad, 5]); anchor families: the seed is asserted to give the same integers in float32 and float64"""
    if (family, name) not in _BUILT:
        fam, case = FAMILIES[family], BY_NAME[name]
        gt = fam.gt(case)
        if family in ANCHOR and family not in case.refused:
            anc32 = fam.anc()[:4]
            anc64 = tuple(t.double() for t in anc32)
            for i in range(2):
                a, b = _ints(MATCH[family](anc32, gt[i])), _ints(MATCH[family](anc64, gt[i].double()))
                assert a == b, f'{family}/{name}: image {i}: the seed leaves a tie to the last bit ({[k for k in a if a[k] != b[k]]} differ between float32 and float64)'
        _BUILT[(family, name)] = (fam, case, gt)
    return _BUILT[(family, name)]


def check(family, name, dev):
    fam, case, gt = build(family, name)
    gt = gt.clone()
    x = fam.inputs()
    dev = torch.device(dev)
    if family in case.refused:
        return _check_refused(fam, x, gt, dev, family, name)
    o = fam.run(x, gt, dev)
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    for k, b in o.items():
        assert b.intact(), f'{family}/{name}: {k} written outside its operand: {b.damage()}'
    out = {k: b.t.detach().cpu().clone() for k, b in o.items()}
    out = fam.project(out) if hasattr(fam, 'project') else out
    refs = [fam.oracle(x, gt, i) for i in range(2)]
    max_form = getattr(fam, 'loss_max_form', False)
    for key, (rel, ab) in fam.loss_tol.items():
        for i, r in enumerate(refs):
            print(f'{family}/{name} {key}[{i}]: got {out[key][i].flatten().tolist()} ref {r[key].flatten().tolist()}')
            EG._close_loss(out[key][i], r[key], rel, ab, max_form, (family, name, key, i))
    group = getattr(fam, 'grad_scale_group', False)
    gscale = EG._scale(torch.cat([r[k].flatten() for r in refs for k in fam.grad_tol]))
    for key, (rel, ab) in fam.grad_tol.items():
        scale = gscale if group else EG._scale(torch.cat([r[key].flatten() for r in refs]))
        for i, r in enumerate(refs):
            err = float((out[key][i].double() - r[key].double()).abs().max())
            print(f'{family}/{name} {key}[{i}]: max error {err:.3e}, bound {rel * scale + ab:.3e}')
            EG._close_grad(out[key][i], r[key], rel, ab, scale, (family, name, key, i))
    fam.check_ints(case, out, gt, refs)
    G = int(torch.argmin(gt[EDGE, :, 0]))
    if 'ngt' in out:
        assert int(out['ngt'][EDGE]) == G
    if name == 'all_valid_1024':
        assert G == 700
    elif name != 'late_owner' and name != 'dup_across':
        assert G == case.pad - 1
    if name == 'late_owner':
        _check_late_owner(fam, family, out, gt, refs[EDGE])
    if name == 'dup_across':
        _check_dup_across(family, out, gt, refs[EDGE])
    return out


def _positive_rg(family, ref):
    """(arg-max box of the oracle's positive anchors that are no best anchor, the oracle's best anchors)"""
    mt = EG._match_of(ref)
    if 'status' in mt:
        return mt['rgindex'][mt['status'] == 1], mt['best']
    return mt['rgindex'][mt['pos']], mt['best']


def _check_late_owner(fam, family, out, gt, ref):
    rows = gt[EDGE]
    assert int(torch.argmin(rows[:, 0])) == 199
    if family in ANCHOR:
        p = fam.candidates()[0]
        rg, best = _positive_rg(family, ref)
        assert int(best[LATE]) == p, 'construction: row 150 does not own its prior'
        assert rg.numel() > 0 and bool((rg == LATE).all()), 'construction: a box other than row 150 matches an anchor well'
        assert int(out['best'][EDGE, LATE]) == p
        assert bool((out['rg'][EDGE][out['status'][EDGE] == 1] == LATE).all()) and int((out['status'][EDGE] == 1).sum()) == rg.numel()
    else:
        sy, sx = fam.hw[0] / 64.0, fam.hw[1] / 64.0
        others = torch.cat([rows[:LATE], rows[LATE + 1: 199]])
        assert float((others[:, 0] + others[:, 2] / 2).max()) < 32 * sy and float((others[:, 1] + others[:, 3] / 2).max()) < 32 * sx, \
            'construction: another box reaches the cells of row 150'
        assert float(rows[LATE, 0] - rows[LATE, 2] / 2) >= 40 * sy and float(rows[LATE, 1] - rows[LATE, 3] / 2) >= 40 * sx


def _check_dup_across(family, out, gt, ref):
    rows = gt[EDGE]
    assert torch.equal(rows[DUP_A], rows[DUP_B]) and int(torch.argmin(rows[:, 0])) == 230
    if family in ANCHOR:
        rg, best = _positive_rg(family, ref)
        assert int(best[DUP_A]) == int(best[DUP_B]), 'construction'
        assert bool((rg == DUP_A).any()), 'construction: the doubled box owns no positive anchor'
        assert int(out['best'][EDGE, DUP_A]) == int(out['best'][EDGE, DUP_B])
        pos = out['status'][EDGE] == 1
        assert bool((out['rg'][EDGE][pos] == DUP_A).any()) and not bool((out['rg'][EDGE][pos] == DUP_B).any()), 'the first of two equal maxima owns the anchor'


def _check_refused(fam, x, gt, dev, family, name):
    """the library refuses the call before any launch: the error names P and the limit, the operands and their bands keep what they held"""
    from odtk import _lib
    held, orig, msg = [], Banded.__init__, None

    def keep(self, *a, **k):
        orig(self, *a, **k)
        held.append((self, self.t.clone()))
    Banded.__init__ = keep
    try:
        try:
            fam.run(x, gt, dev)
        except _lib.OdtkError as e:
            msg = str(e)
    finally:
        Banded.__init__ = orig
    assert msg is not None, f'{family}/{name}: the call was not refused'
    assert str(gt.shape[1]) in msg and str(LIMIT) in msg, f'{family}/{name}: the error does not name P and the limit: {msg}'
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    assert held
    for b, before in held:
        assert b.intact() and torch.equal(b.t, before), (family, name, 'a refused call wrote to an operand')
    return None
