"""Case bodies shared by tests/test_cpu_refinedet_wide.py (csrc/refinedet.hip from source under the fiber emulation) and tests/test_gpu_refinedet_wide.py
(libodtk.so through the C-ABI): ODM rows of 97 .. 256 logits through odtk_refinedet_loss, odtk_refinedet_decode and odtk_refinedet_decode_batched, against
the float64 restatements below, and the one-thread kernels at 21 and 96 logits, byte for byte.

Shapes: N = 2 images, P = 5 ground-truth rows, A = 301 anchors (no multiple of the 4 rows of a wave, of 16 or of 64: the last wave has a ragged group) and
A = 64 (one full workgroup of the loss), C in {97, 128, 129, 200, 256}: one past the old limit, a multiple of 16, one past it (8 -> 16 register slots), no
multiple of 16, the cap.  The anchors are a seeded table (wide_row_cases.anchors, for any A) in which anchor 10 is anchor 7 moved by a pixel and a half and
anchor 20 is anchor 33 moved, so that the matching finds positive rows next to the best anchors.

Ground truth (the matching counts the rows in front of the first -1 row, so at most P - 1 = 4 boxes).  Image 0 has 4 boxes: boxes 0 and 2 sit on anchor 7
(two boxes share their best anchor: the row is visited twice), box 1 on anchor 33, box 3 on anchor 50; labels C - 2, 0, 17, min(33, C - 3).  Image 1 has 2 boxes, and every ARM background LOGIT of it is above 0.99, so none
of its mined negatives enters the ODM term: loss_parts[1, 3] is 0 / 0.

Match state.  ngt, best, status, rgindex, counts come out of odtk_retina_match, the mined rows out of odtk_softmax_ce_const and odtk_nms_batched, as
heads.RefineDetLoss launches them; kernels and restatement read the same tensors.  ONE entry is then rewritten by hand, between the matching and the
mining: status[0, 33] = 1 with rgindex[0, 33] = 1 and one more positive in counts[0, 0].  The matching itself marks every best anchor 3, so it never hands
out a best anchor that is ALSO a status-1 row; the loss kernel takes such a state (its gradient store accumulates), and this is the only way to reach it.

ODM logits: wide_row_cases.logits (top two of a row at least 2^-10 apart; row 0 has the last object class at +80, row 1 the background) with two rows
rewritten: row 4 has class 3 and the background EQUAL at the top (two lanes of the group), row 5 class (C - 1) mod 16 and the background (two slots of one
lane).  The first maximum wins in the one-thread kernel (`p > best`, ascending c), so both rows are kept; a later-wins rule in either the lane loop or the
butterfly drops one of them.  ARM logits of image 0: rows 2 and 3 are (0, 4) and (0, 6): background probability 0.982 and 0.9975, either side of 0.99.

Bounds (u = 2^-24; the derivations of wide_row_cases.py hold, with its softmax64 / _smooth_l1_row / _sum_bound / within):
  ODM softmax, cross entropy, gradient rows, sums: as ssd_loss64 there; a two-logit ARM row is the same restatement with one add.
  refined anchor.  ryx = fl(fl(al ahw) + ayx): u (|al ahw| + |ryx|); rhw = fl(expf(al) ahw): 7 u relative.
  ODM box target.  oyx = (g - ryx) / rhw: (b_ryx + u |g - ryx|) / rhw + 8 u |oyx|; log(g / rhw): 8 u from the quotient's operands, 6 u |t| from logf.
  ARM box gradient.  sl1'(d_yx) + s_yx (ahw / rhw) and sl1'(d_hw) + s_yx oyx + s_hw: the bounds of the clipped derivatives (that of d where |d| < 1, else 0),
      9 u on ahw / rhw, b_oyx on oyx, u per product and add on the running magnitude, then gsc (3 u).
  the total.  (o0 + o1 + o2) + (o3 + o4 + o5): the six bounds and 3 u of the sum of the absolute parts.
Integers (keep, cand) must be EQUAL; the cases assert in float64 that no confidence lies within its bound of the threshold (pick_threshold: the middle of
the widest gap) and no ARM background probability within 1e-5 of 0.99: zero rows are excluded for the seeds committed here.
boxes must be BIT-EQUAL to those of the one-thread kernel (the same entry point at 21 logits on the same ARM / ODM-loc tensors): they do not depend on C."""
import numpy as np
import torch

import edge_gt_cases as E
import wide_row_cases as W
from wide_row_cases import TINY, U, sha256_of, within  # noqa: F401

N, P = 2, 5
SIZES = [301, 64]
CLASSES = [97, 128, 129, 200, 256]
NARROW = [96, 21]                       # the one-thread kernels: their limit and the default
LIMIT = 256
TIE_ROWS = (4, 5)
GRAD_SCALE = 1.0 / N


def _sync(dev):
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()


# ---------------------------------------------------------------- inputs
def anchors(A, seed):
    """(y1x1, y2x2, yx, hw, nmsbox) of a seeded table: centres in [20, 280], sides in [16, 116]"""
    g = torch.Generator().manual_seed(seed)
    yx = 20.0 + 260.0 * torch.rand(A, 2, generator=g)
    hw = 16.0 + 100.0 * torch.rand(A, 2, generator=g)
    for twin, of, dy, dx in ((10, 7, 1.5, -1.0), (20, 33, -1.0, 2.0)):
        yx[twin] = yx[of] + torch.tensor([dy, dx])
        hw[twin] = hw[of]
    y1x1, y2x2 = yx - hw / 2, yx + hw / 2
    return y1x1, y2x2, yx, hw, torch.cat([y1x1, y2x2], 1).contiguous()


def ground_truth(C, anc):
    yx, hw = anc[2], anc[3]
    gt = torch.full((N, P, 5), -1.0)

    def on(a, dy, dx, sh, sw, label):
        return torch.tensor([float(yx[a, 0]) + dy, float(yx[a, 1]) + dx, float(hw[a, 0]) * sh, float(hw[a, 1]) * sw, float(label)])
    gt[0, 0] = on(7, 0.25, -0.25, 1.02, 0.97, C - 2)
    gt[0, 1] = on(33, -0.5, 0.25, 0.95, 1.04, 0)
    gt[0, 2] = on(7, -0.25, 0.5, 0.96, 1.03, 17)
    gt[0, 3] = on(50, 0.5, 0.5, 1.05, 1.05, min(33, C - 3))
    gt[1, 0] = on(5, 0.5, -0.5, 1.03, 0.96, 1)
    gt[1, 1] = on(40, -0.5, 0.25, 0.97, 1.02, C - 2)
    return gt


def inputs(C, A):
    """the four prediction tensors, the anchors, the ground truth (all on the host, float32)"""
    anc = anchors(A, 3000 + A)
    g = torch.Generator().manual_seed(5000 + 7 * C + A)
    arm_loc = 0.5 * torch.randn(N, A, 4, generator=g)
    odm_loc = 0.5 * torch.randn(N, A, 4, generator=g)
    arm_conf = 1.5 * torch.randn(N, A, 2, generator=g)
    arm_conf[1, :, 1] = 1.5 + arm_conf[1, :, 1].abs()                 # image 1: no ARM background logit below 0.99
    arm_conf[0, 2] = torch.tensor([0.0, 4.0])
    arm_conf[0, 3] = torch.tensor([0.0, 6.0])
    z = W.logits(C, 1000 + 3 * C + A, rows=N * A).view(N, A, C).clone()
    for n in range(N):
        for r, c in zip(TIE_ROWS, (3, (C - 1) % 16)):
            top = float(z[n, r].max()) + 1.0
            z[n, r, c] = top
            z[n, r, C - 1] = top
    return dict(arm_loc=arm_loc, arm_conf=arm_conf, odm_loc=odm_loc, odm_conf=z, anc=anc, gt=ground_truth(C, anc))


# ---------------------------------------------------------------- decode
def decode_run(C, A, dev, batched, x=None):
    """odtk_refinedet_decode per image or odtk_refinedet_decode_batched over both, into operands between sentinel bands -> dict of Banded, inputs, thr"""
    from odtk import ops
    x = inputs(C, A) if x is None else x
    thr = W.pick_threshold(x['odm_conf'].numpy())
    d = {k: x[k].to(dev).contiguous() for k in ('arm_loc', 'arm_conf', 'odm_loc', 'odm_conf')}
    yx, hw = x['anc'][2].to(dev), x['anc'][3].to(dev)
    out = dict(conf=E.Banded((N, A, C - 1), dev, init=-7.0), boxes=E.Banded((N, A, 4), dev, init=-7.0), keep=E.Banded((N, A), dev, torch.uint8, init=7),
               cand=E.Banded((N, A, C - 1), dev, torch.uint8, init=7))
    if batched:
        ops.refinedet_decode_batched(d['arm_loc'], d['arm_conf'], d['odm_loc'], d['odm_conf'], yx, hw, thr, out['conf'].t, out['boxes'].t, out['keep'].t,
                                     out['cand'].t)
    else:
        for n in range(N):
            r = ops.refinedet_decode(d['arm_loc'][n], d['arm_conf'][n], d['odm_loc'][n], d['odm_conf'][n], yx, hw, thr)
            for k, t in zip(('conf', 'boxes', 'keep', 'cand'), r):
                out[k].t[n].copy_(t)
    _sync(dev)
    return out, x, thr


def decode64(arm_conf, odm_conf, thr):
    """RefineDet.py:189-206 for one image's rows, without the boxes (float64)"""
    C = odm_conf.shape[1]
    sm = W.softmax64(odm_conf)
    arm = W.softmax64(arm_conf)
    p1 = arm['p'][:, 1]
    assert bool((np.abs(p1 - 0.99) > 1e-5).all()), 'an ARM background probability next to 0.99'
    arg = sm['p'].argmax(1)                                   # the first maximum
    keep = (p1 < 0.99) & (arg < C - 1)
    conf, bconf = sm['p'][:, :C - 1], sm['bp'][:, :C - 1]
    assert bool((np.abs(conf - thr) > bconf).all()), 'a confidence within its bound of the threshold'
    cand = keep[:, None] & (conf >= thr)
    return dict(conf=conf, bconf=bconf, keep=keep.astype(np.uint8), cand=cand.astype(np.uint8), arm_ok=p1 < 0.99, arg=arg)


_NARROW_BOXES = {}


def narrow_boxes(x, A, dev):
    """boxes of the one-thread kernel on x's ARM / ODM-loc tensors (21 logits: the box arithmetic does not read them)"""
    key = (A, str(dev), x['arm_loc'].data_ptr())
    if key not in _NARROW_BOXES:
        from odtk import ops
        g = torch.Generator().manual_seed(A)
        z21 = torch.randn(N, A, 21, generator=g).to(dev)
        yx, hw = x['anc'][2].to(dev), x['anc'][3].to(dev)
        b = [ops.refinedet_decode(x['arm_loc'][n].to(dev).contiguous(), x['arm_conf'][n].to(dev).contiguous(), x['odm_loc'][n].to(dev).contiguous(), z21[n],
                                  yx, hw, 0.5)[1] for n in range(N)]
        _sync(dev)
        _NARROW_BOXES.clear()
        _NARROW_BOXES[key] = (torch.stack(b).cpu(), x)        # (x is kept alive: its data_ptr is the key)
    return _NARROW_BOXES[key][0]


def check_decode(C, A, dev, batched):
    out, x, thr = decode_run(C, A, dev, batched)
    what = f'refinedet_decode{"_batched" if batched else ""} C={C} A={A}'
    for k, b in out.items():
        assert b.intact(), (what, k, 'sentinel band', b.damage())
    got = {k: b.t.cpu() for k, b in out.items()}
    worst = (0.0, 0.0)
    for n in range(N):
        ref = decode64(x['arm_conf'][n].numpy(), x['odm_conf'][n].numpy(), thr)
        assert 0 < int(ref['keep'].sum()) < A and int(ref['cand'].sum()) > 0
        for r in TIE_ROWS:                                                          # two equal maxima, the background one of them: the first wins
            assert ref['arg'][r] < C - 1 and (not ref['arm_ok'][r] or ref['keep'][r] == 1)
        if n == 0:
            assert ref['arg'][1] == C - 1 and ref['keep'][1] == 0                   # the maximum on the background column
            assert ref['arm_ok'][2] and not ref['arm_ok'][3] and ref['keep'][3] == 0      # ARM background probability 0.982 / 0.9975
        assert np.array_equal(got['keep'][n].numpy(), ref['keep']), (what, n, 'keep', np.nonzero(got['keep'][n].numpy() != ref['keep'])[0][:8])
        assert np.array_equal(got['cand'][n].numpy(), ref['cand']), (what, n, 'cand')
        worst = max(worst, within(got['conf'][n].numpy(), ref['conf'], ref['bconf'], f'{what} image {n} conf'), key=lambda w: w[1])
    assert torch.equal(got['boxes'], narrow_boxes(x, A, dev)), (what, 'boxes against the one-thread kernel')
    return worst


def check_tie_rows_are_kept(C, A, dev):
    """the rows with two equal maxima, with an ARM row that lets them through: keep = 1 and their candidates, single and batched"""
    x = inputs(C, A)
    for n in range(N):
        for r in TIE_ROWS:
            x['arm_conf'][n, r] = torch.tensor([1.0, -1.0])
    for batched in (False, True):
        out, _, thr = decode_run(C, A, dev, batched, x=x)
        keep, cand, conf = out['keep'].t.cpu(), out['cand'].t.cpu(), out['conf'].t.cpu()
        for n in range(N):
            ref = decode64(x['arm_conf'][n].numpy(), x['odm_conf'][n].numpy(), thr)
            for r, c in zip(TIE_ROWS, (3, (C - 1) % 16)):
                assert ref['keep'][r] == 1 and ref['arg'][r] == c
                assert int(keep[n, r]) == 1, (C, A, batched, n, r, 'a later maximum won')
                assert ref['cand'][r, c] == 1 and int(cand[n, r, c]) == 1 and float(conf[n, r, c]) >= thr
            assert np.array_equal(keep[n].numpy(), ref['keep'])


def check_batched_equals_single(C, A, dev):
    a, _, _ = decode_run(C, A, dev, False)
    b, _, _ = decode_run(C, A, dev, True)
    for k in a:
        assert torch.equal(a[k].t, b[k].t), (C, A, k)


# ---------------------------------------------------------------- loss
def match_and_mine(x, dev):
    """the launches of heads.RefineDetLoss in front of the loss, and the one hand-made entry (module docstring) -> dict of device tensors"""
    from odtk import ops
    anc = [t.to(dev) for t in x['anc']]
    A = anc[0].shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    ms = dict(ngt=torch.zeros(N, **i32), best=torch.full((N, P), -1, **i32), status=torch.zeros(N, A, dtype=torch.uint8, device=dev),
              rg=torch.zeros(N, A, **i32), counts=torch.zeros(N, 4, **i32), negloss=torch.zeros(N, A, device=dev), sel_idx=torch.full((N, A), -1, **i32),
              sel_cnt=torch.zeros(N, **i32))
    gt = x['gt'].to(dev)
    ws = ops.retina_match_workspace(A, N, P, dev)
    ops.retina_match(anc[0], anc[1], anc[3], gt, ms['ngt'], ms['best'], ms['status'], ms['rg'], ms['counts'], ws)
    _sync(dev)
    assert int(ms['status'][0, 33]) == 3 and int(ms['best'][0, 1]) == 33
    ms['status'][0, 33] = 1
    ms['rg'][0, 33] = 1
    ms['counts'][0, 0] += 1
    arm_conf = x['arm_conf'].to(dev).contiguous()
    ops.softmax_ce_const(arm_conf, N * A, 2, 2, 1, ms['negloss'])
    ops.nms_batched(anc[4], 0, ms['negloss'], A, 1, ms['status'], A, 1, 2, A, N, ms['counts'][:, 2:], 4, 0, 0.7, ms['sel_idx'], A, ms['sel_cnt'])
    _sync(dev)
    ms['anc'], ms['gt'] = anc, gt
    return ms


def loss_run(C, A, dev, x=None):
    """-> dict of Banded outputs (parts [N, 8], d_arm_loc, d_arm_conf, d_odm_loc, d_odm_conf), the inputs, the match state (numpy)"""
    from odtk import ops
    x = inputs(C, A) if x is None else x
    ms = match_and_mine(x, dev)
    d = {k: x[k].to(dev).contiguous() for k in ('arm_loc', 'arm_conf', 'odm_loc', 'odm_conf')}
    out = dict(parts=E.Banded((N, 8), dev, init=-7.0), d_arm_loc=E.Banded((N, A, 4), dev, init=7.0), d_arm_conf=E.Banded((N, A, 2), dev, init=7.0),
               d_odm_loc=E.Banded((N, A, 4), dev, init=7.0), d_odm_conf=E.Banded((N, A, C), dev, init=7.0))
    ops.refinedet_loss(d['arm_loc'], d['arm_conf'], d['odm_loc'], d['odm_conf'], ms['anc'][2], ms['anc'][3], ms['gt'], ms['ngt'], ms['best'], ms['status'],
                       ms['rg'], ms['counts'], ms['negloss'], ms['sel_idx'], ms['sel_cnt'], GRAD_SCALE, out['parts'].t, out['d_arm_loc'].t,
                       out['d_arm_conf'].t, out['d_odm_loc'].t, out['d_odm_conf'].t)
    _sync(dev)
    state = {k: ms[k].cpu().numpy() for k in ('ngt', 'best', 'status', 'rg', 'counts', 'sel_idx', 'sel_cnt')}
    return out, x, state


def _ce(sm, a, label):
    """cross entropy of row a of a softmax64 result against label, and its bound"""
    zl = sm['z'][a, label] - sm['m'][a]
    v = np.log(sm['S'][a]) - zl
    return v, sm['rS'][a] + 6 * U * abs(np.log(sm['S'][a])) + U * abs(zl) + U * abs(v)


def _add_rows(dst, bdst, a, g, bg):
    twice = bool(np.any(dst[a] != 0))
    dst[a] += g
    bdst[a] += bg + (U * np.abs(dst[a]) if twice else 0.0)


def _clip(d, bd):
    ad = np.abs(d)
    assert bool((np.abs(ad - 1) > bd).all()) and bool((ad > bd).all()), 'a coordinate within its bound of a kink of smooth L1'
    return np.where(ad < 1, d, np.sign(d)), np.where(ad < 1, bd, 0.0)


def _positive_boxes(al, ol, gb, ayx, ahw):
    """the two smooth-L1 terms of one positive row (RefineDet.py:505-563) and the gradients by arm_loc / odm_loc, with bounds; all float64 [4] / scalars"""
    fa, bfa, ga, bga = W._smooth_l1_row(al, gb, ayx, ahw)
    ryx = al[:2] * ahw + ayx
    bryx = U * (np.abs(al[:2] * ahw) + np.abs(ryx))
    rhw = np.exp(al[2:]) * ahw
    oyx = (gb[:2] - ryx) / rhw
    boyx = (bryx + U * np.abs(gb[:2] - ryx)) / rhw + 8 * U * np.abs(oyx)
    thw = np.log(gb[2:] / rhw)
    bthw = U * (8 + 6 * np.abs(thw))
    e = np.concatenate([ol[:2] - oyx, ol[2:] - thw])
    be = np.concatenate([boyx, bthw]) + U * np.abs(e)
    ae = np.abs(e)
    f = np.where(ae < 1, 0.5 * e * e, ae - 0.5)
    bf = np.minimum(ae, 1) * be + 2 * U * f
    s, bs = _clip(e, be)
    q = ahw / rhw
    g_yx = ga[:2] + s[:2] * q
    bg_yx = bga[:2] + bs[:2] * q + 10 * U * np.abs(s[:2] * q) + U * np.abs(g_yx)
    g_hw = ga[2:] + s[:2] * oyx + s[2:]
    mag = np.abs(ga[2:]) + np.abs(s[:2] * oyx) + np.abs(s[2:])
    bg_hw = bga[2:] + bs[:2] * np.abs(oyx) + np.abs(s[:2]) * boyx + bs[2:] + 3 * U * mag
    return (fa, bfa), (f.sum(), bf.sum() + 3 * U * f.sum()), (np.concatenate([g_yx, g_hw]), np.concatenate([bg_yx, bg_hw])), (s, bs)


def loss64(x, state, grad_scale):
    """RefineDet.py:422-567 on a given match state, in float64 -> parts [N, 8], the four gradients and their bounds"""
    f64 = lambda t: t.numpy().astype(np.float64)
    arm_loc, odm_loc = f64(x['arm_loc']), f64(x['odm_loc'])
    yx, hw, gt = f64(x['anc'][2]), f64(x['anc'][3]), f64(x['gt'])
    A, C = x['odm_conf'].shape[1:]
    parts, bparts = np.zeros((N, 8)), np.zeros((N, 8))
    names = ('d_arm_loc', 'd_arm_conf', 'd_odm_loc', 'd_odm_conf')
    g = {k: np.zeros((N, A, w)) for k, w in zip(names, (4, 2, 4, C))}
    b = {k: np.zeros((N, A, w)) for k, w in zip(names, (4, 2, 4, C))}
    with np.errstate(all='ignore'):
        for n in range(N):
            odm = W.softmax64(x['odm_conf'][n].numpy())
            arm = W.softmax64(x['arm_conf'][n].numpy())
            num_pos, nsel = int(state['counts'][n, 0]), int(state['sel_cnt'][n])
            idx = state['sel_idx'][n, :nsel]
            to_odm = [a for a in idx if x['arm_conf'][n, a, 1].numpy() < np.float32(0.99)]              # the LOGIT (sic, RefineDet.py:535)
            nodm = len(to_odm)
            g_arm, g_odm, gsc = grad_scale / nsel if nsel else 0.0, grad_scale / nodm if nodm else 0.0, grad_scale / num_pos if num_pos else 0.0
            t = {k: ([], []) for k in ('neg_arm', 'armc', 'armx', 'neg_odm', 'odmc', 'odmx')}

            def ce(sm, a, label, scale, key, dst):
                v, bv = _ce(sm, a, label)
                t[key][0].append(v)
                t[key][1].append(bv)
                gr = (sm['p'][a] - (np.arange(sm['p'].shape[1]) == label)) * scale
                _add_rows(g[dst][n], b[dst][n], a, gr, sm['bp'][a] * scale + 4 * U * np.abs(gr))
            for a in idx:
                ce(arm, a, 1, g_arm, 'neg_arm', 'd_arm_conf')
            for a in to_odm:
                ce(odm, a, C - 1, g_odm, 'neg_odm', 'd_odm_conf')
            rows = [(int(state['best'][n, k]), k) for k in range(int(state['ngt'][n]))] + [(a, int(state['rg'][n, a])) for a in range(A)
                                                                                         if state['status'][n, a] == 1]
            for a, k in rows:
                ce(arm, a, 0, gsc, 'armc', 'd_arm_conf')
                ce(odm, a, int(gt[n, k, 4]), gsc, 'odmc', 'd_odm_conf')
                (fa, bfa), (fo, bfo), (ga, bga), (go, bgo) = _positive_boxes(arm_loc[n, a], odm_loc[n, a], gt[n, k, :4], yx[a], hw[a])
                t['armx'][0].append(fa); t['armx'][1].append(bfa)
                t['odmx'][0].append(fo); t['odmx'][1].append(bfo)
                _add_rows(g['d_arm_loc'][n], b['d_arm_loc'][n], a, ga * gsc, bga * gsc + 3 * U * np.abs(ga * gsc))
                _add_rows(g['d_odm_loc'][n], b['d_odm_loc'][n], a, go * gsc, bgo * gsc + 3 * U * np.abs(go * gsc))
            den = dict(neg_arm=nsel, armc=num_pos, armx=num_pos, neg_odm=nodm, odmc=num_pos, odmx=num_pos)
            for i, k in enumerate(('neg_arm', 'armc', 'armx', 'neg_odm', 'odmc', 'odmx')):
                parts[n, i] = np.sum(t[k][0]) / den[k] if den[k] else np.nan
                bparts[n, i] = W._sum_bound(t[k][0], t[k][1]) / max(den[k], 1) + U * abs(np.nan_to_num(parts[n, i])) + TINY
            parts[n, 6] = (parts[n, 0] + parts[n, 1] + parts[n, 2]) + (parts[n, 3] + parts[n, 4] + parts[n, 5])
            bparts[n, 6] = bparts[n, :6].sum() + 3 * U * np.abs(np.nan_to_num(parts[n, :6])).sum()
            parts[n, 7] = nodm
    return dict(parts=parts, bparts=bparts, rows=rows, **g, **{'b' + k: v + TINY for k, v in b.items()})


def check_state(state, A):
    """what the cases are there for, asserted on the match state itself"""
    best, status, ngt = state['best'], state['status'], state['ngt']
    assert ngt.tolist() == [4, 2]
    assert best[0, 0] == best[0, 2] == 7                                            # two boxes share their best anchor
    assert best[0, 1] == 33 and status[0, 33] == 1                                  # a best anchor that is also a status-1 row
    assert status[0, 10] == 1 and status[0, 20] == 1                                # positives of the matching itself
    assert int(state['sel_cnt'][0]) > 0 and int(state['sel_cnt'][1]) > 0
    assert int(state['counts'][0, 0]) == 4 + int((status[0] == 1).sum())
    for n in range(N):                                                              # no row is visited three times: two addends commute, three do not
        visits = np.bincount(np.concatenate([best[n, :ngt[n]], np.nonzero(status[n] == 1)[0]]), minlength=A)
        assert visits.max() <= 2 and (n > 0 or (visits[7] == 2 and visits[33] == 2))


def check_loss(C, A, dev):
    out, x, state = loss_run(C, A, dev)
    what = f'refinedet_loss C={C} A={A}'
    check_state(state, A)
    for k, o in out.items():
        assert o.intact(), (what, k, 'sentinel band', o.damage())
    ref = loss64(x, state, GRAD_SCALE)
    parts = out['parts'].t.cpu().numpy()
    assert np.isfinite(ref['parts'][0]).all() and ref['parts'][0, 7] > 0
    assert ref['parts'][1, 7] == 0 and np.isnan(ref['parts'][1, 3]) and np.isnan(ref['parts'][1, 6]) and np.isfinite(ref['parts'][1, [0, 1, 2, 4, 5]]).all()
    assert np.isnan(parts[1, 3]) and np.isnan(parts[1, 6])                          # 0 / 0, the kind the one-thread kernel gives (check_nan_kind)
    assert np.array_equal(parts[:, 7], ref['parts'][:, 7])
    worst = [within(parts[:, :7], ref['parts'][:, :7], ref['bparts'][:, :7], f'{what} parts')]
    for k in ('d_arm_loc', 'd_arm_conf', 'd_odm_loc', 'd_odm_conf'):
        worst.append(within(out[k].t.cpu().numpy(), ref[k], ref['b' + k], f'{what} {k}'))
    return max(worst, key=lambda w: w[1])


def check_nan_kind(C, A, dev):
    """image 1 has no mined ODM negative: loss_parts[1, 3] and the total are the non-finite values the one-thread kernel gives on the same ARM tensors"""
    wide, x, _ = loss_run(C, A, dev)
    x21 = dict(x, odm_conf=x['odm_conf'][..., :21].contiguous(), gt=x['gt'].clone())
    x21['gt'][..., 4] = torch.where(x21['gt'][..., 4] >= 0, x21['gt'][..., 4] % 20, x21['gt'][..., 4])
    narrow, _, _ = loss_run(21, A, dev, x=x21)
    a, b = wide['parts'].t.cpu().numpy(), narrow['parts'].t.cpu().numpy()
    assert np.isnan(a[1, 3]) and np.isnan(a[1, 6]) and a[1, 7] == 0
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))
    assert np.array_equal(a[:, 7], b[:, 7])                                         # the count of ODM negatives does not read the ODM logits


def check_rerun(dev):
    """the same call twice on the same inputs, C = 129: the same bytes (a row's second visit is the second of two addends: they commute)"""
    C, A = 129, 301
    a, b = loss_run(C, A, dev), loss_run(C, A, dev)
    for k in a[0]:
        assert np.array_equal(a[0][k].t.cpu().numpy(), b[0][k].t.cpu().numpy(), equal_nan=True), k
    for batched in (False, True):
        a, b = decode_run(C, A, dev, batched), decode_run(C, A, dev, batched)
        for k in a[0]:
            assert torch.equal(a[0][k].t, b[0][k].t), (k, batched)


def check_refusals(dev):
    """C = 257 is refused by the three entry points, with the limit in the message"""
    import pytest
    from odtk import _lib, ops
    C = LIMIT + 1
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    i32, u8 = torch.int32, torch.uint8
    yx, hw = z(4, 2), z(4, 2) + 1.0
    with pytest.raises(_lib.OdtkError, match=r'refinedet_loss: .*C=257 .*256'):
        ops.refinedet_loss(z(1, 4, 4), z(1, 4, 2), z(1, 4, 4), z(1, 4, C), yx, hw, z(1, P, 5) - 1.0, z(1, dt=i32), z(1, P, dt=i32), z(1, 4, dt=u8),
                           z(1, 4, dt=i32), z(1, 4, dt=i32), z(1, 4), z(1, 4, dt=i32), z(1, dt=i32), 1.0, z(1, 8), z(1, 4, 4), z(1, 4, 2), z(1, 4, 4),
                           z(1, 4, C))
    with pytest.raises(_lib.OdtkError, match=r'refinedet_decode: .*C=257 .*256'):
        ops.refinedet_decode(z(4, 4), z(4, 2), z(4, 4), z(4, C), yx, hw, 0.5)
    with pytest.raises(_lib.OdtkError, match=r'refinedet_decode: .*C=257 .*256'):
        ops.refinedet_decode_batched(z(1, 4, 4), z(1, 4, 2), z(1, 4, 4), z(1, 4, C), yx, hw, 0.5, z(1, 4, C - 1), z(1, 4, 4), z(1, 4, dt=u8),
                                     z(1, 4, C - 1, dt=u8))


# ---------------------------------------------------------------- the one-thread kernels, byte for byte
def limit_outputs(dev):
    """every output of the three entry points at C = 96 and C = 21, A = 301 and A = 64: name -> numpy array.  The CPU tier compares them with an emulated
    build of the previous commit's csrc/refinedet.hip; the GPU tier with the SHA-256 of the bytes that commit wrote on an MI355X
    (tests/golden/refinedet_limit_sha256.json)."""
    res = {}
    for C in NARROW:
        for A in SIZES:
            for batched in (False, True):
                out, _, _ = decode_run(C, A, dev, batched)
                for k, o in out.items():
                    res[f'C{C}.A{A}.decode{"_batched" if batched else ""}.{k}'] = o.t.cpu().numpy()
            out, _, state = loss_run(C, A, dev)
            check_state(state, A)
            for k, o in out.items():
                res[f'C{C}.A{A}.loss.{k}'] = o.t.cpu().numpy()
    return res
