"""CPU tier of the crowded-image ground truth (tests/many_gt_cases.py): more than 128 and up to 1 024 rows per image through the matching and loss kernels
of csrc/boxes.hip, retina.hip, refinedet.hip and dense_heads.hip, run FROM SOURCE under the fiber emulation (tests/hip_cpu_backend.py; the SSD and
RefineDet hard-negative NMS is the oracle's there) -- and the classes' own check of the ground truth's shape in set_batch, over mocked launches."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hip_cpu_backend as HC             # noqa: E402
import many_gt_cases as MG               # noqa: E402
import mock_ops                          # noqa: E402


@pytest.mark.parametrize('family,case', MG.PARAMS, ids=[f'{f}-{c}' for f, c in MG.PARAMS])
def test_emulated_many_ground_truth_rows(family, case):
    with HC.installed():
        MG.check(family, case, 'cpu')


def test_table_is_complete():
    assert {c.name for c in MG.CASES} == {'pad_129', 'pad_257', 'pad_1024', 'all_valid_1024', 'late_owner', 'dup_across', 'pad_1025'}
    assert len(MG.PARAMS) == 6 * 7 and all(c.pad > 128 for c in MG.CASES)


def test_limits_are_the_constants_of_ops():
    import odtk
    from odtk import ops
    assert (ops.GT_ROWS_MAX, ops.GT_ROWS_MAX_NARROW) == (1024, 128) and MG.LIMIT == ops.GT_ROWS_MAX
    wide = (odtk.SSD300, odtk.SSD512, odtk.RetinaNet, odtk.RefineDet320, odtk.PFPNetR, odtk.FCOS, odtk.CenterNet, odtk.YOLOv3)
    assert all(c.GT_ROWS_LIMIT == 1024 for c in wide) and odtk.YOLOv2.GT_ROWS_LIMIT == 128 and odtk.LHRCNN.GT_ROWS_LIMIT == 128
    assert odtk._lib.load().odtk_version() >= 109


# ---- host logic: every class checks P where it first sees the ground truth's shape
_SSD = {'mode': 'train', 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'batch_size': 1, 'nms_score_threshold': 0.5,
        'nms_max_boxes': 20, 'nms_iou_threshold': 0.5, 'pretraining_weight': '', 'verbose': False, 'compute_dtype': 'f32', 'seed': 0, 'use_graph': False,
        'device': 'cpu'}
_RD = {'mode': 'train', 'input_size': 320, 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'batch_size': 1,
       'nms_score_threshold': 0.1, 'nms_max_boxes': 20, 'nms_iou_threshold': 0.45, 'pretraining_weight': '', 'verbose': False, 'compute_dtype': 'f32',
       'device': 'cpu'}


def _prov(shape, n):
    return {'data_shape': shape, 'num_train': n, 'num_val': 0, 'train_generator': [], 'val_generator': None}


def _make(kind):
    """(model on the mocked launches, image shape)"""
    import odtk
    if kind == 'SSD300':
        return odtk.SSD300(dict(_SSD), _prov([300, 300, 3], 1)), (1, 300, 300, 3)
    if kind == 'SSD512':
        return odtk.SSD512(dict(_SSD), _prov([512, 512, 3], 1)), (1, 512, 512, 3)
    if kind == 'RetinaNet':
        cfg = {'is_bottleneck': True, 'residual_block_list': [3, 4, 6, 3], 'init_conv_filters': 16, 'mode': 'train', 'is_pretraining': False,
               'data_shape': [128, 128, 3], 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'data_format': 'channels_last', 'batch_size': 1,
               'gamma': 2.0, 'alpha': 0.25, 'nms_score_threshold': 0.8, 'nms_max_boxes': 10, 'nms_iou_threshold': 0.45, 'verbose': False,
               'compute_dtype': 'f32', 'device': 'cpu'}
        return odtk.RetinaNet(cfg, _prov([128, 128, 3], 1)), (1, 128, 128, 3)
    if kind == 'RefineDet320':
        return odtk.RefineDet320(dict(_RD), _prov([320, 320, 3], 1)), (1, 320, 320, 3)
    if kind == 'PFPNetR':
        return odtk.PFPNetR(dict(_RD), _prov([320, 320, 3], 1)), (1, 320, 320, 3)
    if kind == 'FCOS':
        cfg = {'mode': 'train', 'data_shape': [128, 160, 3], 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5,
               'batch_size': 1, 'nms_score_threshold': 0.5, 'nms_max_boxes': 10, 'nms_iou_threshold': 0.45, 'verbose': False, 'compute_dtype': 'f32',
               'device': 'cpu'}
        return odtk.FCOS(cfg, _prov([128, 160, 3], 1)), (1, 128, 160, 3)
    if kind == 'CenterNet':
        cfg = {'mode': 'train', 'input_size': 64, 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5,
               'batch_size': 1, 'score_threshold': 0.1, 'top_k_results_output': 100, 'verbose': False, 'compute_dtype': 'f32', 'device': 'cpu'}
        return odtk.CenterNet(cfg, _prov([64, 64, 3], 1)), (1, 64, 64, 3)
    if kind == 'YOLOv3':
        from oracle import yolov3_ref as YR
        cfg = {'mode': 'train', 'data_shape': [64, 64, 3], 'num_classes': 20, 'weight_decay': 5e-4, 'keep_prob': 0.5, 'data_format': 'channels_last',
               'batch_size': 1, 'coord_scale': 1, 'noobj_scale': 1, 'obj_scale': 5., 'class_scale': 1., 'num_priors': 3, 'nms_score_threshold': 0.5,
               'nms_max_boxes': 10, 'nms_iou_threshold': 0.5, 'priors': YR.PRIORS_PX, 'verbose': False, 'compute_dtype': 'f32', 'device': 'cpu',
               'use_graph': False}
        return odtk.YOLOv3(cfg, _prov([64, 64, 3], 1)), (1, 64, 64, 3)
    if kind == 'YOLOv2':
        from oracle import yolov2_ref as Y2
        cfg = {'mode': 'train', 'is_pretraining': False, 'data_shape': [64, 64, 3], 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5,
               'data_format': 'channels_last', 'batch_size': 1, 'coord_scale': 1, 'noobj_scale': 1, 'obj_scale': 5., 'class_scale': 1.,
               'nms_score_threshold': 0.5, 'nms_max_boxes': 10, 'nms_iou_threshold': 0.5, 'rescore_confidence': False, 'priors': Y2.PRIORS, 'verbose': False,
               'compute_dtype': 'f32', 'device': 'cpu'}
        return odtk.YOLOv2(cfg, _prov([64, 64, 3], 1)), (1, 64, 64, 3)
    assert kind == 'LHRCNN'
    cfg = {'data_shape': [320, 416, 3], 'mode': 'train', 'is_pretraining': False, 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4,
           'keep_prob': 0.5, 'batch_size': 1, 'rpn_first_step': 60000, 'rcnn_first_step': 100000, 'rpn_second_step': 160000, 'nms_score_threshold': 0.5,
           'nms_max_boxes': 20, 'nms_iou_threshold': 0.45, 'post_nms_proposal': 500, 'verbose': False, 'device': 'cpu'}
    return odtk.LHRCNN(cfg, _prov([320, 416, 3], 1)), (1, 320, 416, 3)


def _gt(P):
    gt = torch.full((1, P, 5), -1.0)
    gt[0, 0] = torch.tensor([30., 30., 20., 20., 1.])
    return gt


@pytest.mark.parametrize('kind,limit', [('SSD300', 1024), ('SSD512', 1024), ('RetinaNet', 1024), ('RefineDet320', 1024), ('PFPNetR', 1024), ('FCOS', 1024),
                                        ('CenterNet', 1024), ('YOLOv3', 1024), ('YOLOv2', 128), ('LHRCNN', 128)])
def test_set_batch_checks_the_ground_truth_rows(kind, limit):
    """P up to the class's limit is staged; one row more raises a ValueError that names the class, the row count and the limit -- in set_batch, before
    any launch, and the batch staged before stays"""
    from odtk import _lib
    torch.set_num_threads(8)
    with mock_ops.installed():
        m, shape = _make(kind)
        imgs = torch.zeros(shape)
        ok = 300 if limit == 1024 else 128
        m.set_batch(imgs, _gt(ok))
        assert tuple(m.gt.shape) == (1, ok, 5)
        held = m.gt
        try:
            m.set_batch(imgs, _gt(limit + 1))
        except ValueError as e:
            msg = str(e)
            assert kind in msg and str(limit + 1) in msg and str(limit) in msg, msg
        except _lib.OdtkError as e:                                   # noqa: F841
            raise AssertionError(f'{kind}: the library error surfaced instead of a ValueError')
        else:
            raise AssertionError(f'{kind}: P = {limit + 1} was not refused')
        assert m.gt is held and tuple(m.gt.shape) == (1, ok, 5)
