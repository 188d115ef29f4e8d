"""Test bodies shared by the GPU tier (tests/test_gpu_batched_inference_dense.py) and the CPU tier (tests/test_cpu_batched_inference_dense.py, where the same
kernels run from source under the emulation): odtk_centernet_decode_batched and odtk_refinedet_decode_batched against the single-image entry points."""
import numpy as np
import torch

from single_image_tail import centernet_detect, refinedet_detect

STRIDE = 4.0
THR = 0.3             # score threshold of the CenterNet cases: sigmoid(-2) = 0.12 < THR < sigmoid(1) = 0.73


def _same(a, b):
    return len(a) == 3 and len(b) == 3 and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _sync(dev):
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()


def centernet_logits(H, W, C, seed):
    """[3, H, W, C] logits.  Image 0: nothing above the threshold.  Image 1: one isolated peak with its own value on every (even y, even x) pixel:
    ceil(H / 2) * ceil(W / 2) peaks.  Image 2: a 2 x 3 plateau of equal logits (each of its pixels equals its 3x3 maximum: six peaks of one score, ordered by
    pixel index) under one higher peak in the far corner."""
    g = torch.Generator().manual_seed(seed)
    kp = -2.0 - 2.0 * torch.rand(3, H, W, C, generator=g)
    ny, nx = (H + 1) // 2, (W + 1) // 2
    vals = 1.0 + 2.0 * (torch.randperm(ny * nx, generator=g).float() + 1.0) / (ny * nx)          # distinct
    cls = torch.randint(0, C, (ny, nx), generator=g)
    ys, xs = torch.meshgrid(torch.arange(0, H, 2), torch.arange(0, W, 2), indexing='ij')
    kp[1, ys, xs, cls] = vals.view(ny, nx)
    kp[2, 1:3, 1:4, C - 1] = 2.0
    kp[2, H - 1, W - 1, 0] = 3.0
    off = torch.rand(3, H, W, 2, generator=g)
    size = 1.0 + 8.0 * torch.rand(3, H, W, 2, generator=g)
    return kp, off, size


def check_centernet(H, W, C, top_k, dev):
    from odtk import ops
    N = 3
    kp, off, size = (t.to(dev) for t in centernet_logits(H, W, C, 100 + H + top_k))
    ws1 = ops.centernet_workspace(1, H, W, C, dev)
    # the three situations, on the single-image results with room for every peak
    full = [ops.centernet_decode(kp[n], off[n], size[n], STRIDE, THR, H * W, ws1) for n in range(N)]
    assert full[0][0].numel() == 0
    assert full[1][0].numel() == ((H + 1) // 2) * ((W + 1) // 2) > top_k
    s2 = full[2][0].cpu()
    assert s2.numel() == 7 and float(s2[0]) > float(s2[1]) and bool((s2[1:] == s2[1]).all())           # the corner peak, then the plateau's six ties
    # ties: the lower pixel index first -- the plateau's pixels in row-major order, read back from the boxes' centres
    p2 = [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3)]
    b2 = full[2][1].cpu()
    for j, (y, x) in enumerate(p2):
        cy, cx = float(b2[1 + j, 0] + b2[1 + j, 2]) / (2 * STRIDE), float(b2[1 + j, 1] + b2[1 + j, 3]) / (2 * STRIDE)
        assert abs(cy - (y + float(off[2, y, x, 0]))) < 1e-4 and abs(cx - (x + float(off[2, y, x, 1]))) < 1e-4, (j, y, x, cy, cx)
    want = [ops.centernet_decode(kp[n], off[n], size[n], STRIDE, THR, top_k, ws1) for n in range(N)]
    assert [w[0].numel() for w in want] == [0, top_k, min(7, top_k)]
    scores = torch.full((N, top_k), -7.0, device=dev)
    bbox = torch.full((N, top_k, 4), -7.0, device=dev)
    cid = torch.full((N, top_k), -7, dtype=torch.int32, device=dev)
    counts = torch.full((N,), -7, dtype=torch.int32, device=dev)
    ws = ops.centernet_decode_workspace(N, H, W, dev)
    assert ws.numel() >= N * H * W * 8
    ops.centernet_decode_batched(kp, off, size, STRIDE, THR, top_k, scores, bbox, cid, counts, ws)
    _sync(dev)
    assert counts.tolist() == [w[0].numel() for w in want]
    for n in range(N):
        k = want[n][0].numel()
        assert torch.equal(scores[n, :k], want[n][0]) and torch.equal(bbox[n, :k], want[n][1]) and torch.equal(cid[n, :k], want[n][2]), n
        assert bool((scores[n, k:] == -7.0).all()) and bool((bbox[n, k:] == -7.0).all()) and bool((cid[n, k:] == -7).all()), n      # nothing written past the count
    # the same images in other slots: a workgroup reads its own image only
    ops.centernet_decode_batched(kp.flip(0).contiguous(), off.flip(0).contiguous(), size.flip(0).contiguous(), STRIDE, THR, top_k, scores, bbox, cid, counts, ws)
    _sync(dev)
    assert counts.tolist() == [w[0].numel() for w in want][::-1]
    for n in range(N):
        k = want[n][0].numel()
        assert torch.equal(scores[N - 1 - n, :k], want[n][0]) and torch.equal(bbox[N - 1 - n, :k], want[n][1]) and torch.equal(cid[N - 1 - n, :k], want[n][2]), n


def check_centernet_read_back(dev):
    from odtk import heads
    H, W, C, top_k = 16, 16, 20, 10
    kp, off, size = (t.to(dev) for t in centernet_logits(H, W, C, 7))
    tail = heads.CenterNetBatched(3, H, W, top_k, dev)
    got = tail(kp, off, size, THR, STRIDE)
    part = tail(kp, off, size, THR, STRIDE, n_images=2)
    assert len(got) == 3 and len(part) == 2 and [len(d[0]) for d in got] == [0, top_k, 7]
    for n in range(3):
        s, b, c = centernet_detect(kp[n], off[n], size[n], THR, top_k, STRIDE)
        assert _same(got[n], [s.cpu().numpy(), b.cpu().numpy().reshape(-1, 4), c.cpu().numpy()]), n
        assert n == 2 or _same(part[n], got[n])
    return tail, kp, off, size


def check_refinedet(N, A, C, dev):
    from odtk import heads, ops
    g = torch.Generator().manual_seed(A)
    arm_loc = (0.3 * torch.randn(N, A, 4, generator=g)).to(dev)
    arm_conf = (3.0 * torch.randn(N, A, 2, generator=g)).to(dev)               # softmax(arm)[1] >= 0.99 on some rows: the ARM filter is exercised
    odm_loc = (0.3 * torch.randn(N, A, 4, generator=g)).to(dev)
    odm_conf = (2.0 * torch.randn(N, A, C, generator=g)).to(dev)
    if A == 6375:
        anc = heads.refinedet_anchors(320, dev)
        yx, hw = anc[2], anc[3]
    else:
        yx = (320.0 * torch.rand(A, 2, generator=g)).to(dev)
        hw = (16.0 + 112.0 * torch.rand(A, 2, generator=g)).to(dev)
    thr, max_boxes, iou = 0.3, 20, 0.45
    conf = torch.full((N, A, C - 1), -7.0, device=dev)
    boxes = torch.full((N, A, 4), -7.0, device=dev)
    keep = torch.full((N, A), 7, dtype=torch.uint8, device=dev)
    cand = torch.full((N, A, C - 1), 7, dtype=torch.uint8, device=dev)
    ops.refinedet_decode_batched(arm_loc, arm_conf, odm_loc, odm_conf, yx, hw, thr, conf, boxes, keep, cand)
    _sync(dev)
    for n in range(N):
        w = ops.refinedet_decode(arm_loc[n], arm_conf[n], odm_loc[n], odm_conf[n], yx, hw, thr)
        assert torch.equal(conf[n], w[0]) and torch.equal(boxes[n], w[1]) and torch.equal(keep[n], w[2]) and torch.equal(cand[n], w[3]), n
        assert 0 < int(w[2].sum()) < A and int(w[3].sum()) > 0                  # rows kept and rows dropped, candidates for the NMS
    tail = heads.BatchedTail(N, A, C - 1, max_boxes, dev)
    assert not tail.compact
    got = tail(conf, boxes, cand, iou)
    for n in range(N):
        s, b, c = refinedet_detect(arm_loc[n], arm_conf[n], odm_loc[n], odm_conf[n], yx, hw, thr, max_boxes, iou)
        assert s.numel() > 0 and _same(got[n], [s.cpu().numpy(), b.cpu().numpy().reshape(-1, 4), c.cpu().numpy()]), n
