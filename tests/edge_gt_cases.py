"""Edge-case ground truth through the box-side loss and matching kernels: the case bodies shared by tests/test_cpu_edge_gt.py (the kernel source under the
fiber emulation, tests/hip_cpu_backend.py) and tests/test_gpu_edge_gt.py (libodtk.so on the device).

CASES is a table of named ground-truth sets, rows [yc, xc, h, w, cls] written on a 64 x 64 canvas and scaled to the input of the family under test (sizes given
in pixels -- the 1 px box, the sliver, `size - 0.1` -- are kept in pixels), padded with rows of -1.  Every call has N = 2 images: image 0 carries an ordinary
synthetic_gt() row set of the family's own oracle, image 1 (the LAST one, so that a write one cell or anchor past its end leaves the operand) the edge case.

Comparison rules of check(family, case, dev):
  * every output and gradient operand lies between two bands of BAND sentinel elements, which must be untouched after every launch;
  * finite reference value: the tolerance of the family's existing test (FAMILIES[...].tol quotes it); no case here needed a wider one;
  * non-finite reference value (0 / 0 of an empty set, log 0 of a box that covers no grid point): the kernel's value must be non-finite of the same kind --
    NaN, +inf or -inf -- at the same position; gradients are compared wherever the reference gradient is finite;
  * the reference rejects the input (`rejects` in the table: torch raises where TensorFlow's gather / reduction over an empty axis fails): all outputs of the
    kernel are finite (zero objects in SSD / RetinaNet: the loss parts are of the kind their expressions give on empty sets), a second run agrees (bit for bit where the kernel has no floating atomics), the bands hold.
    At most two such cases per family; a case that is NOT marked and raises fails.
"""
import math

import numpy as np
import torch

from oracle import centernet_ref as CR
from oracle import fcos_ref as FR
from oracle import refinedet_ref as DR
from oracle import retinanet_ref as RR
from oracle import ssd300_ref as SR
from oracle import yolov2_ref as Y2
from oracle import yolov3_ref as Y3

BAND = 4096
FILL = {torch.float32: 1357.0, torch.int32: -13579, torch.uint8: 77}
PAD = 60
EDGE = 1                     # the image that carries the edge case


def _ops():
    import odtk  # noqa: F401
    from odtk import ops
    return ops


class Banded:
    """an output operand between two bands of sentinels"""

    def __init__(self, shape, dev, dtype=torch.float32, init=0):
        self.n = int(np.prod(shape))
        self.fill = FILL[dtype]
        self.whole = torch.full((self.n + 2 * BAND,), self.fill, dtype=dtype, device=dev)
        self.t = self.whole[BAND: BAND + self.n].view(*shape)
        self.t.fill_(init)

    def intact(self):
        return bool((self.whole[:BAND] == self.fill).all()) and bool((self.whole[BAND + self.n:] == self.fill).all())

    def damage(self):
        w = self.whole.cpu()
        w[BAND: BAND + self.n] = self.fill
        bad = (w != self.fill).nonzero().flatten()
        return [(int(i) - BAND, float(w[i])) for i in bad[:6]], int(bad.numel())


# ------------------------------------------------------------------------------------------------------------------ families
class Family:
    name, hw, classes, rejects_on = '', (64, 64), 20, (IndexError, RuntimeError)
    atomics = True                     # floating atomics in the gradient path: a second run agrees to the tolerance, not to the bit

    def ordinary(self, seed, pad):
        raise NotImplementedError

    def gt(self, case):
        pad = case.pad or PAD
        gt = torch.full((2, pad, 5), -1.0)
        o = self.ordinary(41, pad)
        o[:, 4] = torch.where(o[:, 4] >= 0, o[:, 4] % self.classes, o[:, 4])
        gt[0] = o
        if case.name == 'reversed':
            G = int(torch.argmin(o[:, 0]))
            gt[EDGE, :G] = o[:G].flip(0)
        else:
            rows = torch.tensor(case.rows(self), dtype=torch.float64).reshape(-1, 5)
            assert rows.shape[0] <= pad, case.name
            rows[:, 4] = rows[:, 4] % self.classes
            gt[EDGE, : rows.shape[0]] = rows.float()
        return gt

    def check_ints(self, case, out, gt, refs):
        pass

    def same_cell_rows(self):
        return self.px([[21., 22., 30., 16., 1], [22.5, 20.5, 12., 40., 1]])

    def same_cell_holds(self, gt_rows, ref):
        return True

    def px(self, rows):
        """canvas rows -> pixels of this family's input"""
        sy, sx = self.hw[0] / 64.0, self.hw[1] / 64.0
        return [[r[0] * sy, r[1] * sx, r[2] * sy, r[3] * sx, r[4]] for r in rows]


def _first(gt_rows):
    return int(torch.argmin(gt_rows[:, 0]))


# ---- dense heads
class CenterNet(Family):
    name, hw, classes = 'centernet', (64, 64), 3
    tol = 'parts 2e-5 |r| + 1e-6; d_keypoints 2e-4, d_offset / d_size 1e-5 of the largest reference gradient'

    def ordinary(self, seed, pad):
        return CR.synthetic_gt(1, 64, seed, pad=pad)[0]

    def inputs(self):
        g = torch.Generator().manual_seed(3)
        return dict(kp=torch.randn(2, 16, 16, 3, generator=g) * 1.5 - 2.0, off=torch.rand(2, 16, 16, 2, generator=g),
                    size=torch.rand(2, 16, 16, 2, generator=g) * 10)

    def run(self, x, gt, dev):
        ops = _ops()
        N, H, W, C = x['kp'].shape
        kd, od, zd = (x[k].to(dev).contiguous() for k in ('kp', 'off', 'size'))
        out = dict(parts=Banded((N, 4), dev), dk=Banded(kd.shape, dev, init=7.), do=Banded(od.shape, dev, init=7.), dz=Banded(zd.shape, dev, init=7.))
        ws = ops.centernet_workspace(N, H, W, C, dev)
        ops.centernet_loss(kd, od, zd, gt.to(dev), CR.STRIDE, 1.0 / N, out['parts'].t, out['dk'].t, out['do'].t, out['dz'].t, ws)
        return out

    def oracle(self, x, gt, i):
        leaves = [x[k][i].clone().requires_grad_(True) for k in ('kp', 'off', 'size')]
        d = CR.one_image_loss(*leaves, gt[i], detail=True)
        (d['total'] / 2).backward()
        return dict(parts=torch.stack([d[k].detach() for k in ('keypoints_loss', 'offset_loss', 'size_loss', 'total')]),
                    dk=_g(leaves[0]), do=_g(leaves[1]), dz=_g(leaves[2]))

    def same_cell_holds(self, gt_rows, ref):
        c = torch.floor(gt_rows[:2, :2] / CR.STRIDE)
        return bool((c[0] == c[1]).all())

    loss_tol = dict(parts=(2e-5, 1e-6))
    grad_tol = dict(dk=(2e-4, 0.), do=(1e-5, 0.), dz=(1e-5, 0.))


class FCOS(Family):
    name, hw, classes = 'fcos', (64, 64), 3
    atomics = False
    tol = 'loss 3e-5 |r| + 1e-6; gradients 3e-4 of the largest reference gradient'

    def ordinary(self, seed, pad):
        return FR.synthetic_gt(1, 64, seed, pad=pad)[0]

    def inputs(self):
        g = torch.Generator().manual_seed(5)
        sh = FR.level_shapes(64, 64)
        return dict(conf=[torch.randn(2, a, b, 4, generator=g) * 1.5 - 2.0 for a, b in sh], reg=[torch.exp(torch.randn(2, a, b, 4, generator=g)) * 2 for a, b in sh],
                    cen=[torch.randn(2, a, b, 1, generator=g) for a, b in sh])

    def run(self, x, gt, dev):
        ops = _ops()
        cd, rd, zd = ([t.to(dev).contiguous() for t in x[k]] for k in ('conf', 'reg', 'cen'))
        out = dict(loss=Banded((2,), dev))
        for k, lst in (('dconf', cd), ('dreg', rd), ('dcen', zd)):
            for l, t in enumerate(lst):
                out[f'{k}{l}'] = Banded(t.shape, dev, init=7.)
        ws = ops.fcos_workspace(cd, 2, dev)
        ops.fcos_loss(cd, rd, zd, gt.to(dev), 0.5, out['loss'].t, [out[f'dconf{l}'].t for l in range(5)], [out[f'dreg{l}'].t for l in range(5)],
                      [out[f'dcen{l}'].t for l in range(5)], ws)
        return out

    def oracle(self, x, gt, i):
        lv = {k: [t[i].clone().requires_grad_(True) for t in x[k]] for k in ('conf', 'reg', 'cen')}
        tot = FR.one_image_loss(lv['conf'], lv['reg'], lv['cen'], gt[i])
        if tot.requires_grad:
            (tot / 2).backward()
        r = dict(loss=tot.detach())
        for k, n in (('dconf', 'conf'), ('dreg', 'reg'), ('dcen', 'cen')):
            for l in range(5):
                r[f'{k}{l}'] = _g(lv[n][l])
        return r

    loss_tol = dict(loss=(3e-5, 1e-6))
    grad_tol = {f'{k}{l}': (3e-4, 0.) for k in ('dconf', 'dreg', 'dcen') for l in range(5)}
    grad_scale_group = True          # the existing helper scales by the largest gradient of all levels and kinds


class YOLOv3(Family):
    name, hw, classes = 'yolov3', (32, 32), 20
    tol = 'parts 3e-5 |r| + 1e-5; gradients 2e-5 of the largest reference gradient'

    def ordinary(self, seed, pad):
        return Y3.synthetic_gt(1, 32, seed, pad=pad)[0]

    def inputs(self):
        g = torch.Generator().manual_seed(17)
        return dict(pred=[torch.randn(2, h, h, 3, 25, generator=g) * 1.2 for h in (1, 2, 4)])

    def run(self, x, gt, dev):
        ops = _ops()
        pd = [p.to(dev).contiguous() for p in x['pred']]
        out = dict(parts=Banded((2, 5), dev))
        for l, p in enumerate(pd):
            out[f'dp{l}'] = Banded(p.shape, dev, init=7.)
        ws = ops.yolov3_workspace(pd, 2, dev)
        flat = [float(v) for l in Y3.head_priors() for v in l.reshape(-1).tolist()]
        ops.yolov3_loss(pd, flat, Y3.HEAD_STRIDE, gt.to(dev), (1., 1., 5., 1.), 0.5, out['parts'].t, [out[f'dp{l}'].t for l in range(3)], ws)
        return out

    def oracle(self, x, gt, i):
        pr = [p[i].clone().requires_grad_(True) for p in x['pred']]
        d = Y3.one_image_loss(pr, gt[i], detail=True)
        (d['total'] / 2).backward()
        r = dict(parts=torch.stack([d[k].detach() for k in ('coord', 'cls', 'obj', 'noobj', 'total')]))
        for l in range(3):
            r[f'dp{l}'] = _g(pr[l])
        r['detail'] = d
        return r

    def same_cell_rows(self):
        return [[13., 14., 10., 12., 1], [14.5, 13., 11., 12.5, 1]]

    def same_cell_holds(self, gt_rows, ref):
        d = ref['detail']
        lv = [l for l in range(3) if bool(d['masks'][l][0])]
        return len(lv) == 1 and bool(d['masks'][lv[0]][1]) and bool((d['levels'][lv[0]]['cell'][0] == d['levels'][lv[0]]['cell'][1]).all()) \
            and int(d['levels'][lv[0]]['best'][0]) == int(d['levels'][lv[0]]['best'][1])

    loss_tol = dict(parts=(3e-5, 1e-5))
    grad_tol = {f'dp{l}': (2e-5, 0.) for l in range(3)}
    grad_scale_group = True


class YOLOv2(Family):
    name, hw, classes = 'yolov2', (6 * 32, 7 * 32), 4
    atomics = False
    tol = 'total 2e-5 |r|; gradient 1e-5 of the largest reference gradient + 1e-7; two runs bit-identical'
    geom = (2, 6, 7, 3, 4)

    def ordinary(self, seed, pad):
        return Y2.synthetic_gt(1, 6 * 32, seed, pad=pad, max_obj=6, num_classes=4)[0]

    def inputs(self):
        N, H, W, P, C = self.geom
        g = torch.Generator().manual_seed(7)
        return dict(pred=torch.randn(N, H, W, P, C + 5, generator=g))

    def run(self, x, gt, dev):
        ops = _ops()
        N, H, W, P, C = self.geom
        out = dict(parts=Banded((N, 5), dev), d=Banded((N, H * W * P, C + 5), dev, init=9.))
        ops.yolov2_loss(x['pred'].to(dev), [v for hw in Y2.PRIORS[:P] for v in hw], 32.0, gt.to(dev), (1., 1., 5., 1.), 0.5, out['parts'].t, out['d'].t)
        return out

    def oracle(self, x, gt, i):
        N, H, W, P, C = self.geom
        p = x['pred'][i].clone().requires_grad_(True)
        tot = Y2.image_loss(p, gt[i], Y2.PRIORS[:P], (1., 1., 5., 1.), C)
        (tot * 0.5).backward()
        return dict(total=tot.detach(), d=_g(p).reshape(-1, C + 5))

    def project(self, out):
        return dict(total=out['parts'][:, 4], d=out['d'])

    def same_cell_rows(self):
        return [[74., 108., 40., 40., 1], [80., 112., 44., 42., 1]]

    def same_cell_holds(self, gt_rows, ref):
        """same cell and same arg-max prior, by the arithmetic of yolov2_ref.image_loss"""
        g = gt_rows[:2, :4] / 32.0
        cell = torch.floor(g[:, :2])
        pri = torch.tensor(Y2.PRIORS[:self.geom[3]]).view(1, -1, 2)
        a = (cell + 0.5).view(2, 1, 2)
        g1, g2 = (g[:, :2] - g[:, 2:] / 2).unsqueeze(1), (g[:, :2] + g[:, 2:] / 2).unsqueeze(1)
        inter = (torch.minimum(g2, a + pri / 2) - torch.maximum(g1, a - pri / 2)).prod(-1)
        best = torch.argmax(inter / (pri.prod(-1) + (g2 - g1).prod(-1) - inter), dim=-1)
        return bool((cell[0] == cell[1]).all()) and int(best[0]) == int(best[1])

    loss_tol = dict(total=(2e-5, 0.))
    grad_tol = dict(d=(1e-5, 1e-7))


# ---- anchor families
def _iou_row(anc, row):
    """f32 IoU of one ground-truth row with every anchor, in the oracles' op order (ssd300_ref.match)"""
    a_y1x1, a_y2x2, _, a_hw = anc
    g = torch.tensor(row[:4], dtype=torch.float32)
    y1x1, y2x2 = g[0:2] - g[2:4] / 2., g[0:2] + g[2:4] / 2.
    inter = torch.clamp(torch.minimum(a_y2x2, y2x2) - torch.maximum(a_y1x1, y1x1), min=0).prod(-1)
    return inter / (a_hw.prod(-1) + g[2:4].prod() - inter)


class AnchorFamily(Family):
    _anc = None
    _thr = None

    def anchors(self):
        raise NotImplementedError

    def anc(self):
        if self._anc is None:
            type(self)._anc = self.anchors()
        return self._anc

    def candidates(self):
        """anchors entirely inside the picture, of middling size, nearest the centre first"""
        y1x1, y2x2, yx, hw = self.anc()
        H, W = self.hw
        side = hw.prod(-1).sqrt()
        ok = (y1x1[:, 0] > 8) & (y1x1[:, 1] > 8) & (y2x2[:, 0] < H - 8) & (y2x2[:, 1] < W - 8) & (side > 0.15 * min(H, W)) & (side < 0.45 * min(H, W))
        idx = torch.nonzero(ok).flatten()
        d = ((yx[idx, 0] - H / 2.) ** 2 + (yx[idx, 1] - W / 2.) ** 2)
        return idx[torch.argsort(d, stable=True)].tolist()

    def prior_row(self, p, cls=3):
        _, _, yx, hw = self.anc()
        return [float(yx[p, 0]), float(yx[p, 1]), float(hw[p, 0]), float(hw[p, 1]), cls]

    def threshold_rows(self, side):
        """a box inside prior p with p's centre and width and (about) half its height: IoU = 0.5 in exact arithmetic.  The construction is made in float64 and
        the height then moved by single f32 steps; the side of the threshold each step lands on is read off the f32 IoU (and checked again by the oracle's
        match in check_threshold).  Only steps at which p is NOT the box's own best anchor count: a best anchor is positive whatever its IoU.
        -> (row, p) with IoU(p) the largest below ('below'), exactly ('exact') or the smallest above ('above') 0.5"""
        if self._thr is None:
            found = {}
            for p in self.candidates()[:40]:
                yc, xc, h, w, _ = self.prior_row(p)
                hk = np.float32(np.float64(h) * 0.5)
                for _ in range(6):
                    hk = np.nextafter(hk, np.float32(0))
                res = {}
                for _ in range(13):
                    row = [yc, xc, float(hk), w, 3]
                    iou = _iou_row(self.anc(), row)
                    if int(torch.argmax(iou)) != p:
                        v = float(iou[p])
                        if v < 0.5 and ('below' not in res or v > res['below'][0]):
                            res['below'] = (v, row, p)
                        if v > 0.5 and ('above' not in res or v < res['above'][0]):
                            res['above'] = (v, row, p)
                        if v == 0.5:
                            res.setdefault('exact', (v, row, p))
                    hk = np.nextafter(hk, np.float32(np.inf))
                for k, v in res.items():
                    found.setdefault(k, v)
                if len(found) == 3:
                    break
            assert len(found) == 3, (self.name, sorted(found))
            type(self)._thr = found
        return self._thr[side]

    def collide_rows(self):
        p = self.candidates()[0]
        yc, xc, h, w, _ = self.prior_row(p)
        return [[yc + 1.0, xc + 0.5, h * 1.04, w * 0.97, 2], [yc - 0.5, xc - 1.0, h * 0.96, w * 1.03, 5]]

class SSD(AnchorFamily):
    name, hw, classes = 'ssd', (300, 300), 20
    tol = 'parts 2e-5 max(1, |r|); gradient 1e-5 + 1e-3 of the largest reference gradient; match indices, status, counts equal'

    def anchors(self):
        return SR.priors()

    def ordinary(self, seed, pad):
        return _ssd_gt(seed, pad)

    def inputs(self):
        g = torch.Generator().manual_seed(12)
        return dict(pred=torch.randn(2, 8828, 25, generator=g))

    def run(self, x, gt, dev):
        ops = _ops()
        from odtk.ssd300 import prior_spec
        fs, nas, hwp = prior_spec()
        pri = ops.ssd_priors(300, fs, nas, hwp, dev)
        N, A, ld = x['pred'].shape
        P = gt.shape[1]
        i32 = torch.int32
        out = dict(ngt=Banded((N,), dev, i32), best=Banded((N, P), dev, i32), status=Banded((N, A), dev, torch.uint8), rg=Banded((N, A), dev, i32),
                   counts=Banded((N, 4), dev, i32), parts=Banded((N, 4), dev), dpred=Banded((N, A, ld), dev))
        gtd, predd = gt.to(dev), x['pred'].to(dev).contiguous()
        ops.ssd_match(pri[0], pri[1], pri[3], gtd, out['ngt'].t, out['best'].t, out['status'].t, out['rg'].t, out['counts'].t)
        out.update(negloss=Banded((N, A), dev), sel=Banded((N, A), dev, i32, init=-1), cnt=Banded((N,), dev, i32))
        negloss, sel, cnt = out['negloss'].t, out['sel'].t, out['cnt'].t
        ops.softmax_ce_const(predd, N * A, 21, ld, 20, negloss)
        ops.nms_batched(pri[4], 0, negloss, A, 1, out['status'].t, A, 1, 2, A, N, out['counts'].t[:, 2:], 4, 0, 0.7, sel, A, cnt)
        ops.ssd_loss(predd, 21, pri[2], pri[3], gtd, out['ngt'].t, out['best'].t, out['status'].t, out['rg'].t, out['counts'].t, negloss, sel, cnt, 1.0 / N,
                     out['parts'].t, out['dpred'].t)
        return out

    def oracle(self, x, gt, i):
        p = x['pred'][i].clone().requires_grad_(True)
        d = SR.one_image_loss(p[:, 21:23], p[:, 23:], p[:, :21], self.anc(), gt[i], detail=True)
        (d['total'] / 2).backward()
        return dict(parts=torch.stack([d[k].detach() for k in ('neg_loss', 'pos_conf_loss', 'coord', 'total')]), dpred=_g(p), match=d['match'], detail=d)

    def check_ints(self, case, out, gt, refs):
        for i, r in enumerate(refs):
            if r is None:
                continue
            mt, G = r['match'], r['match']['G']
            assert int(out['ngt'][i]) == G
            assert torch.equal(out['best'][i, :G].long(), mt['best']) and bool((out['best'][i, G:] == -1).all())
            st = torch.zeros(8828, dtype=torch.uint8)
            other = torch.nonzero(mt['othermask']).squeeze(1)
            st[other] = torch.where(mt['pos'], torch.tensor(1, dtype=torch.uint8), torch.tensor(2, dtype=torch.uint8))
            assert torch.equal(out['status'][i], st), (case.name, i)
            assert torch.equal(out['rg'][i].long()[other], mt['rgindex'])
            num_pos, num_neg = G + int(mt['pos'].sum()), int((~mt['pos']).sum())
            assert out['counts'][i].tolist()[:3] == [num_pos, num_neg, min(3 * num_pos, num_neg)]

    zero_parts = ('nan', 'nan', 'nan', 'nan')     # means over no mined negative and over no positive row (SSD300.py:434, :445, :450), and their sum
    loss_tol = dict(parts=(2e-5, 2e-5))          # 2e-5 * max(1, |r|) <= 2e-5 |r| + 2e-5: checked in _close with the max() form
    loss_max_form = True
    grad_tol = dict(dpred=(1e-3, 1e-5))


def _ssd_gt(seed, pad):
    g = torch.Generator().manual_seed(seed)
    n = int(torch.randint(1, 7, (1,), generator=g))
    h = torch.rand(n, generator=g) * 240. + 30.
    w = torch.rand(n, generator=g) * 240. + 30.
    yc = h / 2 + torch.rand(n, generator=g) * (300 - h)
    xc = w / 2 + torch.rand(n, generator=g) * (300 - w)
    gt = torch.full((pad, 5), -1.0)
    gt[:n] = torch.stack([yc, xc, h, w, torch.randint(0, 20, (n,), generator=g).float()], 1)
    return gt


class _RetinaMatch(AnchorFamily):
    def match(self, ops, anc_d, gt, dev):
        N, P, _ = gt.shape
        A = anc_d[0].shape[0]
        i32 = torch.int32
        out = dict(ngt=Banded((N,), dev, i32), best=Banded((N, P), dev, i32, init=-1), status=Banded((N, A), dev, torch.uint8), rg=Banded((N, A), dev, i32),
                   counts=Banded((N, 4), dev, i32))
        ws = ops.retina_match_workspace(A, N, P, dev)
        ops.retina_match(anc_d[0], anc_d[1], anc_d[3], gt.to(dev), out['ngt'].t, out['best'].t, out['status'].t, out['rg'].t, out['counts'].t, ws)
        return out


class RetinaNet(_RetinaMatch):
    name, hw, classes = 'retinanet', (320, 256), 20
    tol = 'parts 2e-5 |r| + 1e-6; gradients 1e-6 + 1e-4 of the largest reference gradient; match indices, status, counts equal'
    shape = [320, 256, 3]

    def anchors(self):
        return RR.anchors(self.shape, RR.pyramid_shapes(320, 256))

    def ordinary(self, seed, pad):
        return RR.synthetic_gt(1, 256, seed, pad=pad)[0]

    def inputs(self):
        A = self.anc()[0].shape[0]
        g = torch.Generator().manual_seed(A)
        return dict(pconf=torch.randn(2, A, 21, generator=g) * 2, pbox=torch.randn(2, A, 4, generator=g) * 0.7)

    def run(self, x, gt, dev):
        ops = _ops()
        flat = [v for s in RR.ANCHOR_SIZES for hw in RR.level_priors(s) for v in hw]
        anc_d = ops.retina_anchors(256, RR.pyramid_shapes(320, 256), [RR.NUM_ANCHORS] * 5, flat, dev)
        out = self.match(ops, anc_d, gt, dev)
        N, A, C = x['pconf'].shape
        out.update(parts=Banded((N, 2), dev), dconf=Banded((N, A, C), dev, init=7.), dbox=Banded((N, A, 4), dev, init=7.))
        ops.retina_loss(x['pconf'].to(dev), x['pbox'].to(dev), anc_d[2], anc_d[3], gt.to(dev), out['ngt'].t, out['best'].t, out['status'].t, out['rg'].t,
                        out['counts'].t, 0.25, 2.0, 1.0 / N, out['parts'].t, out['dconf'].t, out['dbox'].t)
        return out

    def oracle(self, x, gt, i):
        pc, pb = x['pconf'][i].clone().requires_grad_(True), x['pbox'][i].clone().requires_grad_(True)
        d = RR.one_image_loss(pb[:, :2], pb[:, 2:], pc, self.anc(), gt[i], 0.25, 2.0, detail=True)
        (d['total'] / 2).backward()
        return dict(parts=torch.stack([d['conf_loss'].detach(), d['coord'].detach()]), dconf=_g(pc), dbox=_g(pb), match=d['match'])

    def check_ints(self, case, out, gt, refs):
        A = self.anc()[0].shape[0]
        for i, r in enumerate(refs):
            if r is None:
                continue
            mt, G = r['match'], r['match']['G']
            assert int(out['ngt'][i]) == G and out['best'][i, :G].tolist() == mt['best'].tolist()
            st = torch.full((A,), 3, dtype=torch.uint8)
            other = torch.nonzero(mt['othermask']).squeeze(1)
            one, two, zero = (torch.tensor(v, dtype=torch.uint8) for v in (1, 2, 0))
            st[other] = torch.where(mt['pos'], one, torch.where(mt['neg'], two, zero))
            assert torch.equal(out['status'][i], st), (case.name, i)
            assert torch.equal(out['rg'][i].long()[other], mt['rgindex'])
            assert out['counts'][i].tolist()[:2] == [G + int(mt['pos'].sum()), int(mt['neg'].sum())]

    # both parts are sums scaled by 1 / num_pos = 1 / 0.  The reference stops at its arg-max over no box, and nothing documents a kind: the focal
    # part would be x / 0 = +inf by its form (RetinaNet.py:474), the kernel multiplies by 1 / 0 and a workgroup without rows gives 0 * inf = NaN.
    # Held to: not a finite number.
    zero_parts = ('not finite', 'not finite')
    loss_tol = dict(parts=(2e-5, 1e-6))
    grad_tol = dict(dconf=(1e-4, 1e-6), dbox=(1e-4, 1e-6))


class RefineDet(_RetinaMatch):
    name, hw, classes = 'refinedet', (320, 320), 20
    tol = 'parts 2e-5 |r| + 1e-6; gradients 1e-4 of the largest reference gradient; match indices, status, counts, mined rows equal'

    def anchors(self):
        return DR.anchors(320)

    def ordinary(self, seed, pad):
        return DR.synthetic_gt(1, 320, seed, pad=pad)[0]

    def inputs(self):
        A = self.anc()[0].shape[0]
        g = torch.Generator().manual_seed(23)
        return dict(arm_loc=torch.randn(2, A, 4, generator=g) * 0.5, arm_conf=torch.randn(2, A, 2, generator=g) * 1.5,
                    odm_loc=torch.randn(2, A, 4, generator=g) * 0.5, odm_conf=torch.randn(2, A, 21, generator=g) * 1.5)

    def run(self, x, gt, dev):
        ops = _ops()
        from odtk import heads
        anc_d = heads.refinedet_anchors(320, dev)
        out = self.match(ops, anc_d, gt, dev)
        N, A = x['arm_loc'].shape[:2]
        xd = {k: v.to(dev).contiguous() for k, v in x.items()}
        out.update(negloss=Banded((N, A), dev), sel=Banded((N, A), dev, torch.int32), cnt=Banded((N,), dev, torch.int32))
        negloss, sel, cnt = out['negloss'].t, out['sel'].t, out['cnt'].t
        ops.softmax_ce_const(xd['arm_conf'], N * A, 2, 2, 1, negloss)
        ops.nms_batched(anc_d[4], 0, negloss, A, 1, out['status'].t, A, 1, 2, A, N, out['counts'].t[:, 2:], 4, 0, 0.7, sel, A, cnt)
        out.update(parts=Banded((N, 8), dev), d_arm_loc=Banded((N, A, 4), dev), d_arm_conf=Banded((N, A, 2), dev), d_odm_loc=Banded((N, A, 4), dev),
                   d_odm_conf=Banded((N, A, 21), dev))
        ops.refinedet_loss(xd['arm_loc'], xd['arm_conf'], xd['odm_loc'], xd['odm_conf'], anc_d[2], anc_d[3], gt.to(dev), out['ngt'].t, out['best'].t,
                           out['status'].t, out['rg'].t, out['counts'].t, negloss, sel, cnt, 1.0 / N, out['parts'].t, out['d_arm_loc'].t, out['d_arm_conf'].t,
                           out['d_odm_loc'].t, out['d_odm_conf'].t)
        return out

    def oracle(self, x, gt, i):
        lv = [x[k][i].clone().requires_grad_(True) for k in ('arm_loc', 'arm_conf', 'odm_loc', 'odm_conf')]
        d = DR.one_image_loss(lv[0][:, :2], lv[0][:, 2:], lv[1], lv[2][:, :2], lv[2][:, 2:], lv[3], self.anc(), gt[i], detail=True)
        (d['total'] / 2).backward()
        return dict(parts=torch.stack([p.detach() for p in d['parts']] + [d['total'].detach()]), d_arm_loc=_g(lv[0]), d_arm_conf=_g(lv[1]), d_odm_loc=_g(lv[2]),
                    d_odm_conf=_g(lv[3]), detail=d)

    def project(self, out):
        o = dict(out)
        o['parts'] = out['parts'][:, :7]
        return o

    def check_ints(self, case, out, gt, refs):
        for i, r in enumerate(refs):
            if r is None:
                continue
            d = r['detail']
            mt = d['match']
            G = mt['G']
            assert int(out['ngt'][i]) == G and out['best'][i, :G].tolist() == mt['best'].tolist()
            assert torch.equal(out['status'][i], mt['status']), (case.name, i)
            other = mt['status'] != 3
            assert torch.equal(out['rg'][i].long()[other], mt['rgindex'][other])
            assert out['counts'][i].tolist()[:3] == [d['num_pos'], d['num_neg'], min(3 * d['num_pos'], d['num_neg'])]
            assert out['sel'][i, : int(out['cnt'][i])].tolist() == d['sel_rows'].tolist()

    loss_tol = dict(parts=(2e-5, 1e-6))
    grad_tol = dict(d_arm_loc=(1e-4, 0.), d_arm_conf=(1e-4, 0.), d_odm_loc=(1e-4, 0.), d_odm_conf=(1e-4, 0.))


FAMILIES = {f.name: f for f in (SSD(), RetinaNet(), RefineDet(), CenterNet(), FCOS(), YOLOv3(), YOLOv2())}
ANCHOR = ('ssd', 'retinanet', 'refinedet')
DENSE = ('centernet', 'fcos', 'yolov3', 'yolov2')


def _g(leaf):
    return leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)


# ------------------------------------------------------------------------------------------------------------------ the table
class Case:
    def __init__(self, name, rows, only=None, rejects=(), pad=None, note='', refused=()):
        self.name, self._rows, self.only, self.rejects, self.pad, self.note, self.refused = name, rows, only, tuple(rejects), pad, note, tuple(refused)

    def rows(self, fam):
        return self._rows(fam) if callable(self._rows) else fam.px(self._rows)

    def applies(self, family):
        return self.only is None or family in self.only


def _crowd(n, seed, min_at=None):
    """n boxes of 2 .. 32 canvas units inside the canvas; with min_at, row min_at gets the smallest yc of all"""
    def rows(fam):
        g = torch.Generator().manual_seed(seed)
        h = torch.rand(n, generator=g) * 30 + 2
        w = torch.rand(n, generator=g) * 30 + 2
        r = torch.stack([h / 2 + torch.rand(n, generator=g) * (64 - h), w / 2 + torch.rand(n, generator=g) * (64 - w), h, w,
                         torch.randint(0, 20, (n,), generator=g).float()], 1)
        if min_at is not None:
            k = int(torch.argmin(r[:, 0]))
            r[[k, min_at]] = r[[min_at, k]]
        return fam.px(r.tolist())
    return rows


def _H(f):
    return float(f.hw[0])


def _W(f):
    return float(f.hw[1])


ORD = [20., 20., 10., 10., 1]          # an ordinary companion box (canvas units)
CASES = [
    # ---- counts
    Case('one', [[30.3, 25.1, 20., 26., 1]]),
    Case('pad_minus_1', _crowd(PAD - 1, 1), note='59 objects, exactly one pad row'),
    Case('zero', lambda f: [], only=('ssd', 'retinanet') + DENSE, rejects=('ssd', 'retinanet'),
         note='the first row is already -1: G = 0.  SSD / RetinaNet: tf.argmax over the empty box axis fails in the reference itself; the dense heads go through '
              'their oracles (empty reductions give the +-inf identity, as in TensorFlow): NaN / inf for CenterNet and YOLOv3, the finite no-object sum for YOLOv2'),
    Case('all_valid', _crowd(PAD, 2, min_at=37), note='no pad row: arg-min over column 0 picks the smallest yc, row 37, so G = 37 and rows 37.. are ignored'),
    Case('pad_128', _crowd(127, 3), only=('yolov2',), pad=128, note='DH_MAX_GT = 128 rows, 127 of them boxes: the last slot of the staged boxes'),
    Case('pad_130', _crowd(129, 4), only=('yolov2',), pad=130, refused=('yolov2',),
         note='129 boxes in 130 rows: more than the DH_MAX_GT = 128 the kernel stages.  It used to clamp G to 128 silently (the reference uses all 129); '
              'odtk_yolov2_loss now refuses pad > 128, as the other dense heads do, and must leave its operands alone'),
    # ---- duplicates and collisions
    Case('dup_same_class', [[21., 22., 30., 16., 1], [21., 22., 30., 16., 1]]),
    Case('dup_other_class', [[21., 22., 30., 16., 1], [21., 22., 30., 16., 2]]),
    Case('same_cell', lambda f: f.same_cell_rows(), only=DENSE,
         note='two different boxes whose centres share a cell (YOLO: and the level and prior), so both add into the same gradient words; asserted in check()'),
    Case('same_best_anchor', lambda f: f.collide_rows(), only=ANCHOR, note='one prior perturbed two ways: both boxes claim it'),
    # ---- thresholds
    Case('exact_prior', lambda f: [f.prior_row(f.candidates()[0])], only=ANCHOR, note='IoU 1 with one prior'),
    Case('iou_below', lambda f: [f.threshold_rows('below')[1]], only=ANCHOR, note='largest f32 IoU < 0.5 with the chosen prior'),
    Case('iou_exact', lambda f: [f.threshold_rows('exact')[1]], only=ANCHOR, note='f32 IoU == 0.5: not positive (strict >)'),
    Case('iou_above', lambda f: [f.threshold_rows('above')[1]], only=ANCHOR, note='smallest f32 IoU > 0.5 with the chosen prior'),
    Case('cell_boundary', [[32., 32., 20., 20., 1], ORD], only=DENSE),
    Case('origin_cell', [[0.5, 0.5, 8., 8., 0], ORD], only=DENSE),
    Case('last_cell', lambda f: [[_H(f) - 0.1, _W(f) - 0.1, 6. * _H(f) / 64, 6. * _W(f) / 64, 2]] + f.px([ORD]), only=DENSE),
    # ---- geometry
    Case('one_px', lambda f: [[30.2 * _H(f) / 64, 31.7 * _W(f) / 64, 1., 1., 0]] + f.px([[10., 50., 20., 20., 1]])),
    Case('sliver', lambda f: [[_H(f) / 2, 30. * _W(f) / 64, _H(f), 1., 0]], note='full height, 1 px wide; FCOS: covers no grid point of its level, log 0'),
    Case('whole_image', [[32., 32., 64., 64., 2]], note='anchor families: every same-shape prior inside the picture ties for the best anchor'),
    Case('partly_outside', [[2., 60., 20., 30., 0]]),
    Case('centre_on_edge', lambda f: [[_H(f), 30. * _W(f) / 64, 10. * _H(f) / 64, 10. * _W(f) / 64, 0], [30. * _H(f) / 64, _W(f), 10. * _H(f) / 64,
                                                                                                   10. * _W(f) / 64, 2]] + f.px([ORD]),
         rejects=('centernet', 'yolov3', 'yolov2'), note='one centre on the bottom edge, one on the right edge: floor(centre / stride) is one past the last cell'),
    Case('fcos_tiny', [[30., 30., 2., 2., 0], ORD], only=('fcos',), note='below the stride of the finest level'),
    Case('fcos_huge', [[32., 32., 600., 600., 1], ORD], only=('fcos',), note='sqrt(h w) >= 512: the last band'),
    # ---- order
    Case('reversed', None, note="image 1 = image 0's rows reversed"),
]
BY_NAME = {c.name: c for c in CASES}
PARAMS = [(f, c.name) for f in FAMILIES for c in CASES if c.applies(f)]
for _f in FAMILIES:
    assert sum(_f in c.rejects for c in CASES) <= 2, _f


# ------------------------------------------------------------------------------------------------------------------ comparison
def _kind(v):
    return 'nan' if math.isnan(v) else ('+inf' if v == math.inf else ('-inf' if v == -math.inf else 'finite'))


def _close_loss(got, ref, rel, ab, max_form, what):
    got, ref = got.double().flatten(), ref.double().flatten()
    for j in range(ref.numel()):
        g, r = float(got[j]), float(ref[j])
        if _kind(r) != 'finite':
            assert _kind(g) == _kind(r), (what, j, g, r)
        else:
            bound = rel * max(1.0, abs(r)) if max_form else rel * abs(r) + ab
            assert abs(g - r) <= bound, (what, j, g, r, abs(g - r), bound)


def _close_grad(got, ref, rel, ab, scale, what):
    m = torch.isfinite(ref)
    if not bool(m.any()):
        return
    err = float((got[m].double() - ref[m].double()).abs().max())
    assert math.isfinite(err) and err <= rel * scale + ab, (what, err, rel * scale + ab)


def _scale(refs_cat):
    m = torch.isfinite(refs_cat)
    return float(refs_cat[m].abs().max()) if bool(m.any()) else 0.0


def check(family, name, dev):
    fam, case = FAMILIES[family], BY_NAME[name]
    assert case.applies(family)
    gt = fam.gt(case)
    x = fam.inputs()
    if name == 'reversed':                                   # the same predictions for both images: only the row order differs
        for v in x.values():
            for t in (v if isinstance(v, list) else [v]):
                t[EDGE] = t[0]
    dev = torch.device(dev)

    def launch():
        o = fam.run(x, gt, dev)
        if dev.type == 'cuda':
            torch.cuda.synchronize()
        for k, b in o.items():
            assert b.intact(), f'{family}/{name}: {k} written outside its operand: {b.damage()}'
        o = {k: b.t.detach().cpu().clone() for k, b in o.items()}
        return fam.project(o) if hasattr(fam, 'project') else o

    if family in case.refused:
        _check_refused(fam, x, gt, dev, family, name)
        return None
    out = launch()
    refs = []
    for i in range(2):
        try:
            refs.append(fam.oracle(x, gt, i))
        except fam.rejects_on as e:
            assert i == EDGE and family in case.rejects, f'{family}/{name}: the oracle rejects image {i} ({type(e).__name__}: {e}) and the table does not say so'
            refs.append(None)
    if family in case.rejects:
        assert refs[EDGE] is None, f'{family}/{name}: marked reference_rejects, but the oracle accepts it'
    max_form = getattr(fam, 'loss_max_form', False)
    for key, (rel, ab) in fam.loss_tol.items():
        for i, r in enumerate(refs):
            if r is not None:
                _close_loss(out[key][i], r[key], rel, ab, max_form, (family, name, key, i))
    group = getattr(fam, 'grad_scale_group', False)
    live = [r for r in refs if r is not None]
    gscale = _scale(torch.cat([r[k].flatten() for r in live for k in fam.grad_tol])) if live else 0.0
    for key, (rel, ab) in fam.grad_tol.items():
        scale = gscale if group else (_scale(torch.cat([r[key].flatten() for r in live])) if live else 0.0)
        for i, r in enumerate(refs):
            if r is not None:
                _close_grad(out[key][i], r[key], rel, ab, scale, (family, name, key, i))
    fam.check_ints(case, out, gt, refs)
    if family in ANCHOR and name.startswith('iou_'):
        _check_threshold(fam, name, refs[EDGE])
    if family in ANCHOR and name == 'same_best_anchor':
        b = refs[EDGE]['match']['best'] if 'match' in refs[EDGE] else refs[EDGE]['detail']['match']['best']
        assert int(b[0]) == int(b[1]), 'construction: the two boxes do not share their best anchor'
    if name == 'same_cell':
        assert fam.same_cell_holds(gt[EDGE], refs[EDGE]), 'construction: the two boxes do not collide'
    if name == 'all_valid':
        assert _first(gt[EDGE]) == 37 and ('ngt' not in out or int(out['ngt'][EDGE]) == 37)
    if name == 'reversed':
        _check_reversed(fam, out, gt)
    if refs[EDGE] is None:
        _check_rejected(fam, family, name, out, launch())
    return out


def _check_refused(fam, x, gt, dev, family, name):
    """the library refuses the call with an error; the outputs keep what they held"""
    from odtk import _lib
    held = {}
    orig = Banded.__init__

    def keep(self, *a, **k):
        orig(self, *a, **k)
        held[len(held)] = (self, self.t.clone())
    Banded.__init__ = keep
    try:
        try:
            fam.run(x, gt, dev)
        except _lib.OdtkError:
            pass
        else:
            raise AssertionError(f'{family}/{name}: the call was not refused')
    finally:
        Banded.__init__ = orig
    assert held
    for b, before in held.values():
        assert b.intact() and torch.equal(b.t, before), (family, name, 'a refused call wrote to an operand')


def _match_of(ref):
    return ref['match'] if 'match' in ref else ref['detail']['match']


def _check_threshold(fam, name, ref):
    """the side of the threshold, as the oracle's own match sees it"""
    side = name[4:]
    v, row, p = fam.threshold_rows(side)
    mt = _match_of(ref)
    assert int(mt['best'][0]) != p, 'construction: the chosen prior is the best anchor'
    if 'status' in mt:
        positive = int(mt['status'][p]) == 1
    else:
        other = torch.nonzero(mt['othermask']).squeeze(1)
        positive = bool(mt['pos'][(other == p).nonzero()[0, 0]])
    assert positive == (side == 'above'), (fam.name, name, v)


def _check_reversed(fam, out, gt):
    """losses agree with the forward order to the family's tolerance; match indices follow the permutation"""
    G = _first(gt[0])
    max_form = getattr(fam, 'loss_max_form', False)
    for key, (rel, ab) in fam.loss_tol.items():
        _close_loss(out[key][EDGE], out[key][0], rel, ab, max_form, (fam.name, 'reversed', key))
    if 'best' in out:
        assert out['best'][EDGE, :G].tolist() == out['best'][0, :G].flip(0).tolist()
        assert torch.equal(out['status'][EDGE], out['status'][0])
        pos = out['status'][0] == 1
        assert torch.equal(out['rg'][EDGE][pos], G - 1 - out['rg'][0][pos])
        assert torch.equal(out['counts'][EDGE], out['counts'][0])


def _check_rejected(fam, family, name, out, again):
    for k, t in out.items():
        if not t.is_floating_point():
            assert torch.equal(t, again[k]), (family, name, k)
            continue
        e = t[EDGE]
        if name == 'zero':
            # G = 0 in SSD / RetinaNet: the reference's arg-max over no box fails, but what its loss expressions give on empty sets is fixed by their
            # form, and the kernels document it ("NaN, as TF").  fam.zero_parts states the kind of every loss part; the gradients have no reference.
            if k == 'parts':
                assert all(_kind(float(v)) == w or (w == 'not finite' and _kind(float(v)) != 'finite') for v, w in zip(e.flatten(), fam.zero_parts)), (family, name, e)
        else:
            assert bool(torch.isfinite(e).all()), (family, name, k, 'not finite')
        same = (t == again[k]) | (torch.isnan(t) & torch.isnan(again[k]))
        if not fam.atomics:
            assert bool(same.all()), (family, name, k, 'two runs differ')
        else:
            rel, ab = fam.grad_tol.get(k, fam.loss_tol.get(k, (0., 0.)))
            m = torch.isfinite(t) & torch.isfinite(again[k])
            assert bool((torch.isfinite(t) == torch.isfinite(again[k])).all())
            if bool(m.any()):
                sc = float(t[m].abs().max())
                assert float((t[m] - again[k][m]).abs().max()) <= rel * max(sc, 1.0) + ab, (family, name, k, 'two runs differ')


def _entry(family):
    def f(case, dev):
        return check(family, case, dev)
    f.__name__ = f'check_{family}'
    return f


check_ssd, check_retinanet, check_refinedet, check_centernet, check_fcos, check_yolov3, check_yolov2 = (_entry(f) for f in FAMILIES)
