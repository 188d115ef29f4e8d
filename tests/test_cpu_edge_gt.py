"""CPU tier of the edge-case ground truth (tests/edge_gt_cases.py): the loss and matching kernels of csrc/boxes.hip, retina.hip, refinedet.hip and
dense_heads.hip run FROM SOURCE under the fiber emulation (tests/hip_cpu_backend.py; the SSD and RefineDet hard-negative NMS is the oracle's there) through
the same check() the GPU tier calls.  This is where the table and the oracles are proved before anything reaches a device."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import edge_gt_cases as EG               # noqa: E402
import hip_cpu_backend as HC             # noqa: E402


@pytest.mark.parametrize('family,case', EG.PARAMS, ids=[f'{f}-{c}' for f, c in EG.PARAMS])
def test_emulated_edge_ground_truth(family, case):
    with HC.installed():
        EG.check(family, case, 'cpu')


def test_table_is_complete():
    """every family has every case that applies to it, and at most two that its reference rejects"""
    for f in EG.FAMILIES:
        names = {c for g, c in EG.PARAMS if g == f}
        assert {'one', 'pad_minus_1', 'all_valid', 'dup_same_class', 'dup_other_class', 'one_px', 'sliver', 'whole_image', 'partly_outside', 'centre_on_edge',
                'reversed'} <= names, f
        assert ('zero' in names) == (f != 'refinedet')
        if f in EG.ANCHOR:
            assert {'same_best_anchor', 'exact_prior', 'iou_below', 'iou_exact', 'iou_above'} <= names, f
        else:
            assert {'same_cell', 'cell_boundary', 'origin_cell', 'last_cell'} <= names, f
        assert sum(f in c.rejects for c in EG.CASES) <= 2, f
    assert ('yolov2', 'pad_130') in EG.PARAMS and {('fcos', 'fcos_tiny'), ('fcos', 'fcos_huge')} <= set(EG.PARAMS)
