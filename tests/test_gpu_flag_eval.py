"""Ground-truth flags (VOC `difficult`, COCO ignore / crowd) on the MI355X: odtk_voc_eval_flags / odtk_coco_eval_flags against the restatement
(tests/flag_eval_ref.py) on the hand-worked sets and the two random shapes of tests/flag_eval_cases.py, gt_flags = NULL against the unflagged entry
points bit for bit, empty sides, the refused flag value, bit-identical reruns, and the generator's sixth ground-truth column after a crop.

Comparison rule: that of tests/test_cpu_flag_eval.py (match, npos, num_ignored_gt and the NaN pattern equal; |AP - ref| <= 1e-12, recall the same)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import flag_eval_cases as K               # noqa: E402
import test_cpu_flag_eval as TF           # noqa: E402
import test_cpu_voc_difficult as TD       # noqa: E402


def test_kernels_on_the_hand_worked_sets(dev):
    TF.check_hand_voc(lambda d, g, f, C, metric: TF.run_voc(d, g, f, C, metric, dev))
    TF.check_hand_coco(lambda d, g, f, C, **kw: TF.run_coco(d, g, f, C, dev, **kw))


@pytest.mark.parametrize('name', list(K.SHAPES))
def test_kernels_vs_ref(dev, name):
    TF.check_random(name, dev)


def test_null_flags_equal_the_plain_entry_points(dev):
    TF.check_null_flags_equal_the_plain_entry_points(dev)


def test_empty_sides(dev):
    TF.check_empty_sides(dev)


def test_flag_3_is_refused_by_the_library(dev):
    TF.check_flag_3_is_refused_by_the_library(dev)


def test_reruns_bit_identical(dev):
    dets, gts, flags, C = K.case('40img-5cls')
    a, b = (TF.run_coco(dets, gts, flags, C, dev) for _ in range(2))
    assert a['match'].tobytes() == b['match'].tobytes() and a['ap'].tobytes() == b['ap'].tobytes() and a['recall'].tobytes() == b['recall'].tobytes()
    a, b = (TF.run_voc(dets, gts, flags, C, 'area', dev) for _ in range(2))
    assert a['match'].tobytes() == b['match'].tobytes() and a['AP'].tobytes() == b['AP'].tobytes()


def test_generator_sixth_column_follows_the_boxes_through_the_crop(dev, tmp_path):
    """one batch of two pictures through the JPEG decoder and the augmentor on the device: scripted draws crop three boxes out of one picture and two out
    of the other; the flags arrive in the rows where their boxes end up"""
    from odtk.augment import Augmentor
    from odtk.voc_data import dataset2tfrecord, get_generator
    xml_dir, img_dir = TD.voc_dir(tmp_path)
    paths = dataset2tfrecord(xml_dir, img_dir, str(tmp_path / 'f'), 'voc', total_shards=1, with_difficult=True)
    it = iter(get_generator(paths, 2, 1, TD.CONFIG, device=dev, seed=0, with_difficult=True, augmentor=TD.scripted(Augmentor(**TD.CONFIG))))
    try:
        img, gt = next(it)
    finally:
        it.close()
    assert tuple(img.shape) == (2, 16, 16, 3) and gt.device.type == 'cuda'
    TD.check_batch(gt, True)
    assert np.isfinite(img.cpu().numpy()).all()
