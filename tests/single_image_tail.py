"""The single-image inference tails, kept on the test side as the independent statement the batched path (odtk.heads.BatchedInference) is compared against:
the single-image decode entry point of the C-ABI -> heads._per_class_nms (odtk_nms_batched, one image; torch.nonzero + gathers above 32 768 rows) -> device
tensors (scores f32[K], bbox f32[K, 4], class_id i32[K]).  Until the classes shared one path these were odtk.heads.*_detect and the bodies of their
test_one_image.  Inputs are the head outputs of ONE image as device tensors."""
import torch


def ssd_detect(pred0, num_classes, priors_yx, priors_hw, score_thr, max_boxes, iou_thr):
    """SSD300.py:190-226.  pred0 [A, num_classes + 4] (last class = background)."""
    from odtk import heads, ops
    A, nc, dev = pred0.shape[0], num_classes - 1, pred0.device
    conf, boxes = torch.zeros(A, nc, device=dev), torch.zeros(A, 4, device=dev)
    keep, cand = torch.zeros(A, dtype=torch.uint8, device=dev), torch.zeros(A, nc, dtype=torch.uint8, device=dev)
    ops.ssd_decode(pred0, num_classes, priors_yx, priors_hw, score_thr, conf, boxes, keep, cand)
    return heads._per_class_nms(conf, boxes, cand, nc, max_boxes, iou_thr)


def retina_detect(pconf, pbox, anchors_yx, anchors_hw, score_thr, max_boxes, iou_thr):
    """RetinaNet.py:224-256.  pconf [A, C] logits (last class = background), pbox [A, 4] = (dy, dx, log h, log w)."""
    from odtk import heads, ops
    conf, boxes, _, cand = ops.retina_decode(pconf, pbox, anchors_yx, anchors_hw, score_thr)
    return heads._per_class_nms(conf, boxes, cand, pconf.shape[1] - 1, max_boxes, iou_thr)


def refinedet_detect(arm_loc, arm_conf, odm_loc, odm_conf, anchors_yx, anchors_hw, score_thr, max_boxes, iou_thr):
    """RefineDet.py:189-230 for one image: arm_loc / odm_loc [A, 4], arm_conf [A, 2], odm_conf [A, C] (last class = background)."""
    from odtk import heads, ops
    conf, boxes, _, cand = ops.refinedet_decode(arm_loc, arm_conf, odm_loc, odm_conf, anchors_yx, anchors_hw, score_thr)
    return heads._per_class_nms(conf, boxes, cand, odm_conf.shape[1] - 1, max_boxes, iou_thr)


def yolov3_detect(preds, priors_flat, score_thr, max_boxes, iou_thr, decode_scale=(32., 32., 16.)):
    """YOLOv3.py:320-368.  preds: three [H, W, P, C + 5] tensors (head 1 = coarsest); decode_scale as in the reference (sic)."""
    from odtk import heads, ops
    conf, bbox = ops.yolov3_decode_candidates(preds, priors_flat, decode_scale)
    cand = (conf >= score_thr).to(torch.uint8)
    return heads._per_class_nms(conf, bbox, cand, conf.shape[1], max_boxes, iou_thr)


def centernet_detect(keypoints, offset, size, score_thr, top_k, stride=4.0, workspace=None):
    """CenterNet.py:159-185 (no NMS: 3x3 peak test + top-k)."""
    from odtk import ops
    H, W, C = keypoints.shape
    ws = workspace if workspace is not None else ops.centernet_workspace(1, H, W, C, keypoints.device)
    return ops.centernet_decode(keypoints, offset, size, stride, score_thr, top_k, ws)


def of_model(m):
    """the single-image tail of a test-mode model of one of the seven classes on ITS OWN head tensors (slot 0) as they stand after a forward pass, with the
    model's thresholds -> [scores, bbox, class_id] as numpy arrays, the form test_one_image returns"""
    import odtk
    if isinstance(m, odtk.SSD300):                       # (SSD512 too)
        out = ssd_detect(m.pred[0], m.num_classes, m.pri[2], m.pri[3], m.nms_score_threshold, m.nms_max_boxes, m.nms_iou_threshold)
    elif isinstance(m, odtk.RetinaNet):
        out = retina_detect(m.pconf[0], m.pbox[0], m.anc[2], m.anc[3], m.nms_score_threshold, m.nms_max_boxes, m.nms_iou_threshold)
    elif isinstance(m, odtk.YOLOv3):
        from odtk.yolov3 import STRIDE
        out = yolov3_detect([p[0] for p in m.preds], m.priors_flat, m.nms_score_threshold, m.nms_max_boxes, m.nms_iou_threshold,
                            decode_scale=(STRIDE[2], STRIDE[2], STRIDE[1]))
    elif isinstance(m, odtk.CenterNet):
        from odtk.centernet import STRIDE
        out = centernet_detect(m.keypoints[0], m.offset[0], m.size[0], m.score_threshold, m.top_k_results_output, STRIDE, m.loss_ws)
    else:                                                # RefineDet320, PFPNetR
        out = refinedet_detect(m.arm_loc[0], m.arm_conf[0], m.odm_loc[0], m.odm_conf[0], m.anc[2], m.anc[3], m.nms_score_threshold, m.nms_max_boxes,
                               m.nms_iou_threshold)
    s, b, c = out
    return [s.cpu().numpy(), b.cpu().numpy().reshape(-1, 4), c.cpu().numpy()]
