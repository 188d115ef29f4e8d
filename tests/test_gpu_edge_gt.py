"""GPU tier of the edge-case ground truth (tests/edge_gt_cases.py): every (family, case) of the table through libodtk.so on the device -- same-address
atomics, wave reductions and the matching / NMS kernels of csrc/boxes.hip that the CPU tier only emulates.  One or two launches per case at the table's sizes."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_gt_cases as EG               # noqa: E402


@pytest.mark.parametrize('family,case', EG.PARAMS, ids=[f'{f}-{c}' for f, c in EG.PARAMS])
def test_edge_ground_truth(family, case, dev):
    EG.check(family, case, dev)
