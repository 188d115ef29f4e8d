"""Writes tests/golden/many_gt_redraws.json: for every (anchor family, case) of tests/many_gt_cases.py the rows of the case's random draw that leave a tie to
the last bit -- the oracle's match gives another integer in float64 than in float32 -- and the seed whose draw replaces each of them.  Runs on the CPU:
    python tools/many_gt_redraws.py [case ...]
Every round evaluates both matches, redraws the boxes involved in a disagreement from the next seed, and stops when none is left."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import many_gt_cases as MG               # noqa: E402
from edge_gt_cases import ANCHOR, EDGE, FAMILIES, Case          # noqa: E402


def _full(mt, A):
    """per-anchor (arg-max box, class of the anchor: 0 ignored, 1 positive, 2 negative, 3 best) on all A anchors"""
    if 'status' in mt:
        return mt['rgindex'].clone(), mt['status'].long()
    rg, st = torch.zeros(A, dtype=torch.long), torch.full((A,), 3, dtype=torch.long)
    other = torch.nonzero(mt['othermask']).squeeze(1)
    rg[other] = mt['rgindex']
    neg = mt['neg'] if 'neg' in mt else ~mt['pos']
    st[other] = torch.where(mt['pos'], 1, torch.where(neg, 2, 0))
    return rg, st


def disagreeing_boxes(family, fam, gt_rows):
    anc32 = fam.anc()[:4]
    anc64 = tuple(t.double() for t in anc32)
    a, b = MG.MATCH[family](anc32, gt_rows), MG.MATCH[family](anc64, gt_rows.double())
    assert a['G'] == b['G']
    bad = set(torch.nonzero(a['best'] != b['best']).flatten().tolist())
    if bad:
        return bad
    A = anc32[0].shape[0]
    (rga, sta), (rgb, stb) = _full(a, A), _full(b, A)
    live = sta != 3
    d = live & ((rga != rgb) | (sta != stb))
    return set(rga[d].tolist()) | set(rgb[d].tolist())


def main():
    torch.set_num_threads(16)
    only = set(sys.argv[1:])                     # case names to search again; the entries of the others are kept
    out = {k: v for k, v in MG.REDRAWS.items() if only and k.split('/')[1] not in only}
    for family in ANCHOR:
        fam = FAMILIES[family]
        for case in MG.CASES:
            if family in case.refused or (only and case.name not in only):
                continue
            draw, seed, fixed = MG.DRAWS[case.name]
            redraws, tries = [], {}
            for rnd in range(60):
                c = Case(case.name, MG._rows_of(case.name, redraws), pad=case.pad)
                gt = fam.gt(c)
                bad = disagreeing_boxes(family, fam, gt[EDGE])
                print(family, case.name, 'round', rnd, 'boxes that tie:', sorted(bad), flush=True)
                if not bad:
                    break
                G = int(torch.argmin(gt[EDGE, :, 0]))
                ymin = float(gt[EDGE, G, 0]) if G < case.pad and float(gt[EDGE, G, 0]) > 0 else None          # all_valid: row G keeps the smallest yc
                for row in sorted(bad):
                    if row in fixed or (case.name == 'dup_across' and row in (MG.DUP_A, MG.DUP_B)):
                        raise SystemExit(f'{family}/{case.name}: the constructed row {row} ties: choose another construction')
                    while True:
                        tries[row] = tries.get(row, 0) + 1
                        s = seed + 1000 * tries[row]
                        new = draw(s)(fam)[row]
                        if ymin is None or new[0] > ymin:
                            break
                    redraws = [r for r in redraws if r[0] != row] + [[row, s]]
            else:
                raise SystemExit(f'{family}/{case.name}: ties left after 60 rounds')
            if redraws:
                out[f'{family}/{case.name}'] = sorted(redraws)
    with open(MG.REDRAWS_FILE, 'w') as f:
        json.dump(out, f, separators=(',', ':'))
        f.write('\n')
    print('written', MG.REDRAWS_FILE, {k: len(v) for k, v in out.items()})


if __name__ == '__main__':
    main()
