"""Bodies shared by tests/test_gpu_batched_inference.py (the kernels on the GPU) and tests/test_cpu_batched_inference.py (the same kernels compiled from
source for the CPU emulation, the NMS standing in as tests/hip_cpu_backend.py does): the batched inference tail against the single-image tail, and the
row compaction against torch.nonzero.  Everything goes through odtk.ops / odtk.heads, i.e. through the C-ABI."""
import numpy as np
import torch

NMS_MAX_BOXES, SCORE_THR, IOU_THR = 10, 0.5, 0.5
N_IMAGES = 5
SHAPES = {'ssd': (8828, 21), 'retina': (40000, 21)}          # (rows per image, classes incl. background); 40 000 > the NMS capacity of 32 768 rows


def make_heads(kind, seed):
    """seeded head tensors of N_IMAGES images with distinct scores: background wins everywhere except on 400 chosen rows per image, which carry one of the
    image's 3 + n foreground classes well above the threshold; the LAST image has no such row (zero detections); classes >= 8 never occur"""
    A, C = SHAPES[kind]
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N_IMAGES, A, C, generator=g)
    logits[..., C - 1] += 12.0
    for n in range(N_IMAGES - 1):
        rows = torch.randperm(A, generator=g)[:400]
        cls = torch.randint(0, 3 + n, (400,), generator=g)
        logits[n, rows, cls] += 15.0
    box = 0.1 * torch.randn(N_IMAGES, A, 4, generator=g)
    return logits, box


def _priors(kind, dev):
    from odtk import ops
    if kind == 'ssd':
        from odtk.ssd300 import prior_spec
        fs, nas, hw = prior_spec()
        pri = ops.ssd_priors(300, fs, nas, hw, dev)
        return pri[2], pri[3]
    g = torch.Generator().manual_seed(77)
    A = SHAPES[kind][0]
    return (800.0 * torch.rand(A, 2, generator=g)).to(dev), (20.0 + 200.0 * torch.rand(A, 2, generator=g)).to(dev)


def single_image_tail(kind, logits, box, yx, hw, n, dev):
    """the existing single-image tail on image n alone: odtk_ssd_decode / odtk_retina_decode -> odtk_nms_batched -> host gather"""
    from odtk import ops
    from single_image_tail import retina_detect
    A, C = SHAPES[kind]
    nc = C - 1
    if kind == 'ssd':
        pred0 = torch.cat([logits[n], box[n]], 1).contiguous().to(dev)
        conf = torch.zeros(A, nc, device=dev); boxes = torch.zeros(A, 4, device=dev)
        keep = torch.zeros(A, dtype=torch.uint8, device=dev); cand = torch.zeros(A, nc, dtype=torch.uint8, device=dev)
        ops.ssd_decode(pred0, C, yx, hw, SCORE_THR, conf, boxes, keep, cand)
        cap = NMS_MAX_BOXES
        out_idx = torch.zeros(nc, cap, dtype=torch.int32, device=dev); out_cnt = torch.zeros(nc, dtype=torch.int32, device=dev)
        ops.nms_batched(boxes, 0, conf, 1, nc, cand, 1, nc, 1, A, nc, None, 0, NMS_MAX_BOXES, IOU_THR, out_idx, cap, out_cnt)
        cnt, idx, conf_h, boxes_h = out_cnt.cpu().tolist(), out_idx.cpu(), conf.cpu(), boxes.cpu()
        s, b, c = [], [], []
        for k in range(nc):
            ids = idx[k, : cnt[k]].long()
            s.append(conf_h[ids, k]); b.append(boxes_h[ids]); c.append(torch.full((cnt[k],), k, dtype=torch.int32))
        return [torch.cat(s).numpy(), torch.cat(b, 0).numpy().reshape(-1, 4), torch.cat(c).numpy()], (conf, boxes, keep, cand)
    pconf, pbox = logits[n].contiguous().to(dev), box[n].contiguous().to(dev)
    dec = ops.retina_decode(pconf, pbox, yx, hw, SCORE_THR)
    s, b, c = retina_detect(pconf, pbox, yx, hw, SCORE_THR, NMS_MAX_BOXES, IOU_THR)                         # (torch.nonzero above 32 768 rows)
    return [s.cpu().numpy(), b.cpu().numpy().reshape(-1, 4), c.cpu().numpy()], dec


def batched_tail(kind, logits, box, yx, hw, dev):
    from odtk import heads, ops
    A, C = SHAPES[kind]
    N, nc = logits.shape[0], C - 1
    conf = torch.zeros(N, A, nc, device=dev); boxes = torch.zeros(N, A, 4, device=dev)
    keep = torch.zeros(N, A, dtype=torch.uint8, device=dev); cand = torch.zeros(N, A, nc, dtype=torch.uint8, device=dev)
    if kind == 'ssd':
        ops.ssd_decode_batched(torch.cat([logits, box], 2).contiguous().to(dev), C, yx, hw, SCORE_THR, conf, boxes, keep, cand)
    else:
        ops.retina_decode_batched(logits.contiguous().to(dev), box.contiguous().to(dev), yx, hw, SCORE_THR, conf, boxes, keep, cand)
    tail = heads.BatchedTail(N, A, nc, NMS_MAX_BOXES, dev)
    assert tail.compact == (A > 32768)
    return tail(conf, boxes, cand, IOU_THR), (conf, boxes, keep, cand)


def check_tail(kind, dev, seed=11):
    """GPU case 1: the batched tail's triple of image n equals (==, every array, in order) the single-image tail run on image n alone"""
    dev = torch.device(dev)
    logits, box = make_heads(kind, seed)
    yx, hw = _priors(kind, dev)
    nc = SHAPES[kind][1] - 1
    singles = [single_image_tail(kind, logits, box, yx, hw, n, dev) for n in range(N_IMAGES)]
    # the inputs are not vacuous (asserted on the single-image results)
    per = np.stack([np.bincount(s[0][2], minlength=nc) for s in singles])                          # detections per (image, class)
    assert all((per[n] > 0).sum() >= 3 for n in range(N_IMAGES - 1)), per
    assert (per[: N_IMAGES - 1] == 0).any() and (per == NMS_MAX_BOXES).any() and per.max() == NMS_MAX_BOXES, per
    assert per[N_IMAGES - 1].sum() == 0 and sum(len(s[0][0]) == 0 for s in singles) == 1, per
    for s in singles:                                                                             # distinct scores inside every class
        for k in range(nc):
            v = s[0][0][s[0][2] == k]
            assert len(np.unique(v)) == len(v)
    got, dec = batched_tail(kind, logits, box, yx, hw, dev)
    assert len(got) == N_IMAGES
    for n in range(N_IMAGES):
        for name, a, b in zip(('conf', 'boxes', 'keep', 'cand'), dec, singles[n][1]):
            assert torch.equal(a[n].cpu(), b.cpu()), (kind, n, name)
        want = singles[n][0]
        for name, a, b in zip(('scores', 'bbox', 'class_id'), got[n], want):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (kind, n, name, a.shape, b.shape)
    return per


def check_default_model(m, imgs, thresholds, cap):
    """a model built WITHOUT test_batch_size (one image slot), two pictures x two thresholds: test_one_image == (every array, dtype and shape) the single-image
    tail (tests/single_image_tail.py) on the head tensors that very forward pass left in the model, and == test_images of that picture [0]; not vacuous:
    detections, and somewhere a class (CenterNet: an image) that fills its `cap` = nms_max_boxes (top_k_results_output)"""
    import single_image_tail as ST
    assert m.batch_size == 1 and m.images.shape[0] == 1 and 'test_batch_size' not in m.config and m.NATIVE_TEST_IMAGES and len(thresholds) == 2
    key = 'nms_score_threshold' if hasattr(m, 'nms_score_threshold') else 'score_threshold'
    same = lambda a, b: len(a) == 3 and len(b) == 3 and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))
    old, counts, fullest = getattr(m, key), [], 0
    try:
        for thr in thresholds:
            setattr(m, key, thr)
            for n in range(2):
                x = np.ascontiguousarray(imgs[n: n + 1])
                got = m.test_one_image(x)
                want = ST.of_model(m)
                assert same(got, want), (thr, n, [a.shape for a in got], [a.shape for a in want])
                again = m.test_images(x)
                assert len(again) == 1 and same(got, again[0]), (thr, n)
                counts.append(len(got[0]))
                fullest = max(fullest, len(got[0]) if key == 'score_threshold' else int(np.bincount(got[2], minlength=1).max(initial=0)))
    finally:
        setattr(m, key, old)
    print(f'{type(m).__name__}: detections per (threshold, picture) {counts}, fullest class {fullest} of {cap}')
    assert sum(counts) > 0 and fullest == cap, (counts, fullest, cap)
    for bad in (np.concatenate([imgs[:1], imgs[:1]]), imgs[:1, :-1]):              # one slot: two images, or another size, are refused by the staging
        for f in (m.test_one_image, m.test_images):
            try:
                f(bad)
            except ValueError as e:
                assert 'test_images' in str(e)
            else:
                raise AssertionError('a bad input was accepted')
    return counts


def check_compaction(dev):
    """GPU case 2: odtk_compact_rows == torch.nonzero(cand.any(1)) per image (incl. an image with no candidate and one where every row is one), twice with
    identical bytes; the capacity clamp; odtk_gather_rows moves the rows' operands"""
    from odtk import ops
    dev = torch.device(dev)
    g = torch.Generator().manual_seed(5)
    for A, nc, ld in ((5000, 20, 20), (3001, 21, 25), (40000, 4, 4), (1024, 3, 3)):
        cand = (torch.rand(4, A, ld, generator=g) < 0.02).to(torch.uint8)
        cand[1] = 0
        cand[2] = 1
        if ld > nc:
            cand[1, :, nc:] = 1                                  # columns behind num_classes do not count
        ref = [torch.nonzero(cand[n, :, :nc].any(1)).flatten() for n in range(4)]
        assert len(ref[1]) == 0 and len(ref[2]) == A and 0 < len(ref[0]) < A
        cd = cand.to(dev)
        runs = []
        for _ in range(2):
            rows = torch.full((4, A), -1, dtype=torch.int32, device=dev)
            counts = torch.full((4,), -1, dtype=torch.int32, device=dev)
            ops.compact_rows(cd, nc, A, rows, counts)
            runs.append((rows.cpu(), counts.cpu()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        rows_h, counts_h = runs[0]
        for n in range(4):
            assert int(counts_h[n]) == len(ref[n]), (A, nc, n)
            assert torch.equal(rows_h[n, : len(ref[n])].long(), ref[n]), (A, nc, n)
            assert bool((rows_h[n, len(ref[n]):] == -1).all())
        # a capacity below the count: the first cap_rows indices, the TRUE count
        capr = 100
        rows = torch.full((4, capr), -1, dtype=torch.int32, device=dev)
        counts = torch.zeros(4, dtype=torch.int32, device=dev)
        ops.compact_rows(cd, nc, capr, rows, counts)
        for n in range(4):
            k = min(len(ref[n]), capr)
            assert int(counts[n]) == len(ref[n]) and torch.equal(rows[n, :k].cpu().long(), ref[n][:k]) and bool((rows[n, k:] == -1).all())
        # gather
        conf = torch.rand(4, A, ld, generator=g); boxes = torch.rand(4, A, 4, generator=g)
        co = torch.full((4, capr, nc), -1.0, device=dev); bo = torch.full((4, capr, 4), -1.0, device=dev)
        ko = torch.full((4, capr, nc), 7, dtype=torch.uint8, device=dev)
        ops.gather_rows(rows, counts, nc, conf.to(dev), boxes.to(dev), cd, co, bo, ko)
        for n in range(4):
            k = min(len(ref[n]), capr)
            assert torch.equal(co[n, :k].cpu(), conf[n, ref[n][:k], :nc]) and torch.equal(bo[n, :k].cpu(), boxes[n, ref[n][:k]])
            assert torch.equal(ko[n, :k].cpu(), cand[n, ref[n][:k], :nc])
            assert bool((co[n, k:] == -1).all()) and bool((ko[n, k:] == 7).all())
