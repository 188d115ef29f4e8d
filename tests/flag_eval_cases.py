"""The sets that tests/test_cpu_flag_eval.py (restatement, emulated kernels) and tests/test_gpu_flag_eval.py (MI355X) share: hand-worked ones whose
answers are written next to them, and random ones against tests/flag_eval_ref.py, whose results are computed once per process and never modified.

A set is (dets, gts, flags, C): dets / gts as the evaluators' add() takes them per image, flags per image an int array [pad]."""
import functools

import numpy as np

import flag_eval_ref as F

ALL = [[0, 1e10]]


def _gt(*rows):
    return np.array(rows, np.float32).reshape(-1, 5)


def _det(scores, boxes, cls):
    return (np.array(scores, np.float32), np.array(boxes, np.float32).reshape(-1, 4), np.array(cls, np.int32))


# ---------------------------------------------------------------- VOC, by hand
def voc_difficult():
    """one image, one class: A = (0, 0, 10, 10) ordinary, B = (20, 20, 30, 30) difficult, disjoint.  By descending score: a detection on nothing, one on
    B, one on A, a second on A, a second on B -> codes 0, 2, 1, 0, 2 and npos = 1.  Counted: FP, TP, FP -> recall 0, 1, 1, precision 0, 1/2, 1/3:
    AP = 1/2 in both metrics.  Without the flags: codes 0, 1, 1, 0, 0, npos = 2, precision 0, 1/2, 2/3, 1/2, 2/5 at recall 0, 1/2, 1, 1, 1: AP = 2/3."""
    d = _det([0.9, 0.8, 0.7, 0.6, 0.5], [[50, 50, 60, 60], [20, 20, 30, 30], [0, 0, 10, 10], [0, 0, 10, 9], [20, 20, 30, 29]], [0] * 5)
    return [d], [_gt([5, 5, 10, 10, 0], [25, 25, 10, 10, 0])], [np.array([0, 1])], 1


def voc_all_rows_flagged():
    """class 1 has only flagged rows (one difficult, one crowd): its detections on them get code 2, the one elsewhere code 0; npos[1] = 0, AP[1] NaN,
    left out of the mAP, which is class 0's AP = 1"""
    d = _det([0.9, 0.8, 0.7, 0.6], [[0, 0, 10, 10], [20, 20, 30, 30], [40, 40, 50, 50], [70, 70, 80, 80]], [0, 1, 1, 1])
    g = _gt([5, 5, 10, 10, 0], [25, 25, 10, 10, 1], [45, 45, 10, 10, 1], [-1, -1, -1, -1, -1])
    return [d], [g], [np.array([0, 1, 2, 0])], 2


# ---------------------------------------------------------------- COCO, by hand: (dets, gts, C, kw) and a function flag -> flags
def coco_crowd_box(flag):
    """a 100 x 100 row with two 10 x 10 detections inside it: IoU 100 / 10 000, intersection / detection area = 1.  Crowd (2): both code 2 at every
    threshold.  Ignore (1): IoU decides, both unmatched -> code 0.  Ordinary (0): both code 0 and npos = 1."""
    d = _det([0.9, 0.8], [[10, 10, 20, 20], [30, 30, 40, 40]], [0, 0])
    return [d], [_gt([50, 50, 100, 100, 0])], [np.array([flag])], 1, dict(area_ranges=ALL)


def coco_ignore_row_matches_once(flag):
    """two detections on one flagged row (IoU 1 and 0.9): flag 1 -> the first is ignored (2), the row is matched, the second a false positive (0);
    flag 2 -> the row stays available, both are ignored (2)"""
    d = _det([0.9, 0.8], [[0, 0, 10, 10], [0, 0, 10, 9]], [0, 0])
    return [d], [_gt([5, 5, 10, 10, 0])], [np.array([flag])], 1, dict(iou_thresholds=[0.5], area_ranges=ALL)


def coco_ordinary_row_beats_crowd():
    """a detection (0, 0, 10, 12) on an ordinary row (0, 0, 10, 10) -- IoU 100 / 120 -- and inside a crowd row (0, 0, 40, 40) -- overlap 1: the
    non-ignored row is visited first and the walk stops at the crowd row: code 1 (at 0.5 and 0.75; at 0.9 the IoU is too low and the crowd takes it: 2)"""
    d = _det([0.9], [[0, 0, 10, 12]], [0])
    return [d], [_gt([20, 20, 40, 40, 0], [5, 5, 10, 10, 0])], [np.array([2, 0])], 1, dict(iou_thresholds=[0.5, 0.75, 0.9], area_ranges=ALL)


# ---------------------------------------------------------------- random sets
def random_case(seed, n_img, C, D=2000, G=300):
    """40 images x 5 classes (or 1 x 1), 2 000 detections, 300 GT rows: about a quarter of the rows flagged 1 and a tenth flagged 2; crowd rows are large
    (150 - 300 px) and a fifth of the detections are small boxes inside one of them; 60 % are jittered copies of a row; scores on 8 levels (ties);
    the first 90 detections belong to one (image, class) whose rows carry every flag -- a segment of more than 64 positions -- and its three best
    are two boxes inside a crowd row and one on an ordinary row, so the crowd rule shows even under a detection cap of 3."""
    rng = np.random.default_rng(seed)
    big = min(1, n_img - 1)
    gimg = rng.integers(0, n_img, G)
    gcls = rng.integers(0, C, G)
    gflag = rng.choice([0, 1, 2], G, p=[0.65, 0.25, 0.10])
    gimg[:8], gcls[:8], gflag[:8] = big, 0, [0, 1, 2, 0, 0, 1, 2, 0]
    side = np.where(gflag[:, None] == 2, rng.uniform(150, 300, (G, 2)), rng.uniform(10, 120, (G, 2)))
    yc, xc = rng.uniform(60, 440, G), rng.uniform(60, 440, G)
    rows = np.stack([yc, xc, side[:, 0], side[:, 1], gcls], 1).astype(np.float32)
    dimg = rng.integers(0, n_img, D)
    dimg[:90] = big
    boxes = np.zeros((D, 4))
    dcls = rng.integers(0, C, D)
    for i in range(D):
        mine = np.nonzero(gimg == dimg[i])[0] if i >= 90 else np.arange(8)
        crowds = mine[gflag[mine] == 2]
        u = rng.random()
        if mine.size and u < 0.6:
            j = int(rng.choice(mine))
            h, w = side[j]
            boxes[i] = [yc[j] - h / 2, xc[j] - w / 2, yc[j] + h / 2, xc[j] + w / 2] + rng.normal(0, 0.08, 4) * [h, w, h, w]
            dcls[i] = gcls[j] if rng.random() < 0.9 else dcls[i]
        elif crowds.size and u < 0.8:
            j = int(rng.choice(crowds))
            h, w = rng.uniform(8, 40, 2)
            y = rng.uniform(yc[j] - side[j, 0] / 2, yc[j] + side[j, 0] / 2 - h)
            x = rng.uniform(xc[j] - side[j, 1] / 2, xc[j] + side[j, 1] / 2 - w)
            boxes[i], dcls[i] = [y, x, y + h, x + w], gcls[j]
        else:
            y, x = rng.uniform(0, 400, 2)
            boxes[i] = [y, x, y + rng.uniform(5, 150), x + rng.uniform(5, 150)]
        if i < 90:
            dcls[i] = 0
    scores = (rng.integers(1, 9, D) / 8).astype(np.float32)
    # the head of the big segment at any detection cap: two 10 x 10 boxes at the centre of its first crowd row (row 2), then that segment's row 0 itself
    for i in (0, 1):                                                        # (the same box twice: whichever crowd row the tie rule picks, it picks twice)
        boxes[i] = [yc[2] - 5, xc[2] - 5, yc[2] + 5, xc[2] + 5]
    boxes[2] = [yc[0] - side[0, 0] / 2, xc[0] - side[0, 1] / 2, yc[0] + side[0, 0] / 2, xc[0] + side[0, 1] / 2]
    scores[:3] = 1.0
    dets, gts, flags = [], [], []
    for m in range(n_img):
        k = dimg == m
        dets.append((scores[k], boxes[k].astype(np.float32), dcls[k].astype(np.int32)))
        g = gimg == m
        gts.append(np.concatenate([rows[g], -np.ones((1, 5), np.float32)]))             # one padding row
        flags.append(np.concatenate([gflag[g], [0]]).astype(np.int64))
    return dets, gts, flags, C


SHAPES = {'40img-5cls': (21, 40, 5), '1img-1cls': (22, 1, 1)}                      # the two shapes of the GPU tier
MAX_DETS = (3, 100)


@functools.lru_cache(maxsize=None)
def case(name):
    return random_case(*SHAPES[name])


@functools.lru_cache(maxsize=None)
def voc_reference(name, metric, flagged=True):
    dets, gts, flags, C = case(name)
    return F.voc_evaluate(dets, gts, C, flags if flagged else None, metric=metric)


@functools.lru_cache(maxsize=None)
def coco_reference(name, max_dets, flagged=True):
    dets, gts, flags, C = case(name)
    return F.coco_evaluate(dets, gts, C, flags if flagged else None, max_dets=max_dets)


def big_segment(name):
    """(first position, length) of the forced segment in the (image, class)-segmented order of the detections"""
    dets, _, _, C = case(name)
    key = np.concatenate([np.full(len(d[0]), m) * (C + 1) + d[2] for m, d in enumerate(dets)])
    mine = min(1, len(dets) - 1) * (C + 1)
    return int((key < mine).sum()), int((key == mine).sum())


def with_flag_column(gts, flags):
    """the [pad, 6] form of add(): the flag in column 5, -1 in padding rows"""
    out = []
    for g, f in zip(gts, flags):
        col = np.where(g[:, 4] >= 0, f, -1).astype(np.float32)
        out.append(np.concatenate([g, col[:, None]], 1))
    return out
