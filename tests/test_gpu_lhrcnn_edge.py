"""GPU tier of the Light-Head R-CNN edge cases (tests/lhrcnn_edge_cases.py): every case of the table through libodtk.so on the device -- the wave shuffles and
ballots of lh_match_kernel, the NMS kernels of csrc/boxes.hip and the same-address atomics of crop_and_resize_bwd that the CPU tier only emulates.  A few tiny
launches per case."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lhrcnn_edge_cases as LE           # noqa: E402


@pytest.mark.parametrize('group,case', LE.PARAMS, ids=[f'{g}-{c}' for g, c in LE.PARAMS])
def test_lhrcnn_edge(group, case, dev):
    LE.check(group, case, dev)
