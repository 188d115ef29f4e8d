"""GPU tier of the crowded-image ground truth (tests/many_gt_cases.py): every (family, case) of its table through libodtk.so on the device, and one training
step per class in scope at P = 300 (200 boxes in image 0, 3 in image 1)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_gt_cases as EG               # noqa: E402
import many_gt_cases as MG               # noqa: E402


@pytest.mark.parametrize('family,case', MG.PARAMS, ids=[f'{f}-{c}' for f, c in MG.PARAMS])
def test_many_ground_truth_rows(family, case, dev):
    MG.check(family, case, dev)


# ---- model level: one training step per class at P = 300
def _grid_gt(H, W, pad):
    """[2, pad, 5]: image 0 200 boxes of one size (a fifth of the picture) whose centres are the 20 x 10 points of a grid, so that no two of them share a
    best anchor or a centre cell of the finer maps -- gradient words that three or more boxes add into by float atomics depend on the order of arrival,
    at any P; image 1 three boxes"""
    gt = torch.full((2, pad, 5), -1.0)
    k = torch.arange(200)
    iy, ix = (k // 10).float(), (k % 10).float()
    yc, xc = (iy + 0.5) * (H / 20.0), (ix + 0.5) * (W / 10.0)
    h, w = torch.full((200,), 0.2 * H), torch.full((200,), 0.2 * W)
    gt[0, :200] = torch.stack([yc, xc, h, w, (k % 20).float()], 1)
    gt[1, :3] = torch.tensor([[0.3 * H, 0.4 * W, 0.3 * H, 0.25 * W, 1.], [0.6 * H, 0.55 * W, 0.5 * H, 0.6 * W, 7.], [0.75 * H, 0.2 * W, 0.2 * H, 0.3 * W, 12.]])
    return gt


def _classes():
    import test_gpu_centernet_model as TC
    import test_gpu_fcos_model as TF
    import test_gpu_pfpnet_model as TP
    import test_gpu_refinedet_model as TR
    import test_gpu_retinanet_model as TN
    import test_gpu_ssd300 as T3
    import test_gpu_ssd512 as T5
    import test_gpu_yolov3 as TY
    prov = lambda shape: {'data_shape': shape, 'num_train': 2, 'num_val': 0, 'train_generator': [], 'val_generator': None}      # noqa: E731
    return {
        'SSD300': (lambda: T3._model('train', 'f32', 2, prov([300, 300, 3])), (300, 300), 'ssd'),
        'SSD512': (lambda: T5._model('train', 'f32', 2), (512, 512), 'ssd'),
        'RetinaNet': (lambda: TN._model('train', 'f32', 2, 160, prov([160, 160, 3])), (160, 160), 'retinanet'),
        'RefineDet320': (lambda: TR._model('train', 2, prov([320, 320, 3])), (320, 320), 'refinedet'),
        'PFPNetR': (lambda: TP._model('train', 2, prov([320, 320, 3])), (320, 320), 'refinedet'),
        'FCOS': (lambda: TF._model('train', 2, prov([128, 160, 3])), (128, 160), 'fcos'),
        'CenterNet': (lambda: TC._model('train', 2, prov([128, 128, 3])), (128, 128), 'centernet'),
        'YOLOv3': (lambda: TY._model('train', 'f32', 2, 64, prov([64, 64, 3])), (64, 64), 'yolov3'),
    }


@pytest.mark.parametrize('kind', ['SSD300', 'SSD512', 'RetinaNet', 'RefineDet320', 'PFPNetR', 'FCOS', 'CenterNet', 'YOLOv3'])
def test_training_step_at_300_rows(kind, dev):
    """One training step of the class's smallest test model (the helpers of its tests/test_gpu_*_model.py, f32 engine) with 200 boxes in image 0 and 3 in
    image 1.  The loss is finite; it equals, to the family's loss tolerance, what the same rows give when the pad behind them is longer (P = 1024 instead
    of 300: everything behind the first pad row is ignored); and a second model built from the same seed gives the same loss and the same parameters
    after the step, bit for bit."""
    make, (H, W), family = _classes()[kind]
    rel, ab = next(iter(EG.FAMILIES[family].loss_tol.values()))
    g = torch.Generator().manual_seed(7)
    imgs = (torch.rand(2, H, W, 3, generator=g) * 255).round()

    def step(pad):
        torch.manual_seed(1234)
        m = make()
        m.set_batch(imgs, _grid_gt(H, W, pad))
        loss = float(m.train_step(0.001))
        torch.cuda.synchronize()
        return loss, m.P.detach().clone()
    l300, p300 = step(300)
    l300b, p300b = step(300)
    l1024, _ = step(1024)
    print(kind, 'loss at P = 300:', l300, l300b, 'at P = 1024:', l1024)
    assert l300 == l300 and abs(l300) != float('inf'), l300
    assert abs(l300 - l1024) <= rel * max(1.0, abs(l300)) + ab, (l300, l1024)
    print(kind, 'largest parameter difference between the two identical steps:', float((p300 - p300b).abs().max()))
    assert l300 == l300b and torch.equal(p300, p300b), (l300, l300b)
