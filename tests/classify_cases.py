"""Case bodies shared by tests/test_cpu_classify.py (csrc/classify.hip from source under the fiber emulation) and tests/test_gpu_classify.py (libodtk.so on
the device): odtk_classify_eval against the float64 NumPy restatement below of the contract in include/odtk.h ("Classification metrics").

Integers (rank, totals, class_seen, class_hit) must be EQUAL to the restatement: comparisons of f32 values are exact.

Bound on loss[n] against float64 (derived from the kernel's summation, not measured; u = 2^-24, one f32 rounding; a 3-ulp function result is within
6 u relative -- the OpenCL full-profile bounds for exp and log the ROCm device library is written to; glibc's expf / logf on the CPU tier are within 1 ulp):
    d_j = z_j - m is one rounding: exp sees d_j (1 + e), |e| <= u, so each term is off by a factor exp(d_j e): relative |d_j| u,
    expf adds 6 u per term, and the sum of the C <= 1024 positive terms is 3 sequential adds per thread (4 columns), 6 butterfly steps and 3 adds over
    the waves: depth 12, taken as 13 u to cover the second-order terms.  So S' = S (1 + r), |r| <= (19 + D) u with D = sum |d_j| exp(d_j) / S.
    logf(S') = log S + r (first order) with 3 ulp of its own: 6 u |log S|.  t = z_label - m is one rounding, u |t|; the final subtraction one more, u |loss|.
    bound(n) = u * (19 + D + 6 |log S| + |z_label - m| + |loss|), evaluated per row in float64 from the row's own logits
(about 4e-6 for a 224-way row of unit-scale logits).  loss_sum is a float64 sum of those f32 values in row order: the restatement adds the kernel's own f32
losses the same way and must be equal to the last bit; against the float64 losses it is held to the sum of the rows' bounds."""
import contextlib

import numpy as np
import torch

U = 2.0 ** -24
GUARD = 8
SHAPES = [(1, 1, 1, 1), (3, 5, 8, 2), (4, 64, 64, 5), (5, 65, 80, 5), (2, 224, 224, 5), (3, 1024, 1024, 5), (2, 7, 7, 7)]       # (N, C, ldl, top_k)
PAD_VALUE = 1e30


# ---------------------------------------------------------------- the float64 restatement
def reference(logits, C, labels, top_k):
    """logits f32 [N, >= C] (numpy), labels int [N] -> rank i64[N], loss f64[N], totals i64[4], seen i64[C], hit i64[C], bound f64[N] (NaN where the loss
    is not finite), counted bool[N]"""
    N = logits.shape[0]
    rank, loss, bound = np.zeros(N, np.int64), np.full(N, np.nan), np.full(N, np.nan)
    totals, seen, hit, counted = np.zeros(4, np.int64), np.zeros(C, np.int64), np.zeros(C, np.int64), np.zeros(N, bool)
    with np.errstate(all='ignore'):
        for n in range(N):
            lab = int(labels[n])
            if not 0 <= lab < C:
                rank[n] = -1
                totals[3] += 1
                continue
            z = logits[n, :C].astype(np.float64)
            zl = z[lab]
            rank[n] = C if not np.isfinite(zl) else int((z > zl).sum() + (z[:lab] == zl).sum())
            m = z.max()
            d = z - m
            S = np.exp(d).sum()
            loss[n] = np.log(S) - (zl - m)
            if np.isfinite(loss[n]):
                D = np.where(np.isfinite(d), np.abs(d) * np.exp(d), 0.0).sum() / S
                bound[n] = U * (19 + D + 6 * abs(np.log(S)) + abs(zl - m) + abs(loss[n]))
            counted[n] = True
            totals[0] += 1
            totals[1] += rank[n] == 0
            totals[2] += rank[n] < top_k
            seen[lab] += 1
            hit[lab] += rank[n] == 0
    return dict(rank=rank, loss=loss, totals=totals, seen=seen, hit=hit, bound=bound, counted=counted)


# ---------------------------------------------------------------- running the entry point between guard words
def _guarded(n, dtype, fill, dev, init=None):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype)
    if init is not None:
        buf[GUARD: GUARD + n] = torch.as_tensor(init, dtype=dtype)
    buf = buf.to(dev)
    return buf, buf[GUARD: GUARD + n]


class Run:
    """the outputs of odtk_classify_eval, each between GUARD sentinel words on both sides; launch() may be called again: the accumulators accumulate"""

    def __init__(self, N, C, dev, init=None):
        self.N, self.C, self.dev = N, C, dev
        init = init or {}
        self.bufs = {}
        for name, n, dt, fill, start in (('rank', N, torch.int32, -77, -5), ('loss', N, torch.float32, -77.0, -5.0), ('totals', 4, torch.int64, -77, 0),
                                         ('loss_sum', 1, torch.float64, -77.0, 0.0), ('seen', C, torch.int32, -77, 0), ('hit', C, torch.int32, -77, 0)):
            self.bufs[name] = _guarded(n, dt, fill, dev, init.get(name, torch.full((n,), start, dtype=dt)))

    def launch(self, logits_dev, ldl, labels_dev, top_k):
        from odtk import ops
        b = self.bufs
        ops.classify_eval(logits_dev, ldl, self.N, self.C, labels_dev, top_k, b['rank'][1], b['loss'][1], b['totals'][1], b['loss_sum'][1], b['seen'][1],
                          b['hit'][1])
        if torch.device(self.dev).type == 'cuda':
            torch.cuda.synchronize()
        out = {}
        for name, (buf, view) in b.items():
            h = buf.cpu().numpy()
            fill = -77
            assert (h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all(), f'{name}: guard words overwritten {h[:GUARD]} {h[-GUARD:]}'
            out[name] = h[GUARD:-GUARD].copy()
        return out


def run_once(logits, C, labels, top_k, dev, init=None):
    """logits f32 numpy [N, ldl], labels int numpy [N] -> outputs (numpy) of one launch into fresh (or `init`) accumulators"""
    N, ldl = logits.shape
    r = Run(N, C, dev, init)
    return r.launch(torch.from_numpy(np.ascontiguousarray(logits)).to(dev), ldl, torch.from_numpy(np.asarray(labels, np.int32)).to(dev), top_k)


def row_order_sum(loss_f32, counted, start=0.0):
    acc = np.float64(start)
    for v, c in zip(loss_f32, counted):
        if c:
            acc = acc + np.float64(v)
    return acc


def compare(got, ref, what=''):
    """integers equal; loss within bound(n) where float64 is finite and non-finite where it is not; the loss sum as documented above.  Returns the largest
    |loss - float64| / bound and the largest |loss - float64| over the finite rows (printed by the callers)"""
    assert np.array_equal(got['rank'], ref['rank']), (what, got['rank'], ref['rank'])
    assert np.array_equal(got['totals'], ref['totals']), (what, got['totals'], ref['totals'])
    assert np.array_equal(got['seen'], ref['seen']) and np.array_equal(got['hit'], ref['hit']), what
    fin = np.isfinite(ref['loss'])
    assert not np.isfinite(got['loss'][~fin]).any(), (what, got['loss'], ref['loss'])
    bad = ~ref['counted']
    assert np.isnan(got['loss'][bad]).all(), what
    err = np.abs(got['loss'][fin].astype(np.float64) - ref['loss'][fin])
    worst = float((err / ref['bound'][fin]).max()) if fin.any() else 0.0
    print(f'{what}: max |loss - f64| {float(err.max()) if fin.any() else 0.0:.3e}, {worst:.3f} of the bound')
    assert (err <= ref['bound'][fin]).all(), (what, err, ref['bound'][fin])
    want = row_order_sum(got['loss'], ref['counted'])
    if np.isfinite(want):
        assert got['loss_sum'][0] == want, (what, got['loss_sum'][0], want)
        assert abs(got['loss_sum'][0] - ref['loss'][ref['counted']].sum()) <= ref['bound'][ref['counted']].sum() * (1 + 1e-9), what
    else:
        assert not np.isfinite(got['loss_sum'][0]), what
    return worst, float(err.max()) if fin.any() else 0.0


def make_case(N, C, ldl, seed, pad=PAD_VALUE):
    """logits with natural ties (a quarter of the rows on a 0.5 grid), labels of which about half are the arg-max; pad columns hold `pad`"""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((N, C)) * 3).astype(np.float32)
    z[::4] = np.round(z[::4] * 2) / 2
    labels = rng.integers(0, C, N)
    for n in range(0, N, 2):
        labels[n] = int(np.argmax(z[n]))
    logits = np.full((N, ldl), pad, np.float32)
    logits[:, :C] = z
    return logits, labels.astype(np.int32)


# ---------------------------------------------------------------- the cases
def check_shape(N, C, ldl, top_k, dev):
    """one launch at the shape: everything against float64; pad columns of 1e30 change nothing; twice the same bits"""
    logits, labels = make_case(N, C, ldl, 100 + N + C)
    ref = reference(logits, C, labels, top_k)
    got = run_once(logits, C, labels, top_k, dev)
    w = compare(got, ref, f'N={N} C={C} ldl={ldl} top_k={top_k}')
    again = run_once(logits, C, labels, top_k, dev)
    zero_pad, _ = make_case(N, C, ldl, 100 + N + C, pad=0.0)
    other = run_once(zero_pad, C, labels, top_k, dev)
    for k in got:
        assert np.array_equal(got[k], again[k], equal_nan=True), (k, 'run to run')
        assert np.array_equal(got[k], other[k], equal_nan=True), (k, 'pad columns')
    assert got['loss_sum'].tobytes() == again['loss_sum'].tobytes()
    if C > 1 and N > 1:
        assert ref['totals'][1] > 0, ref['totals']                 # not vacuous: some row is a hit
    return w


def gap_pred(logits, C, dev):
    """the pred (and loss) of odtk_gap_softmax_ce_fwd for the same logits: a [N * 1][ldl] input with HW = 1"""
    from odtk import ops
    N, ldl = logits.shape
    x = torch.from_numpy(np.ascontiguousarray(logits)).to(dev)
    out = torch.zeros(N, C).to(dev)
    pred = torch.zeros(N, dtype=torch.int32).to(dev)
    ops.gap_softmax_ce_fwd(x, ldl, N, 1, C, None, 0., out, None, pred, None, None)
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), logits[:, :C])
    return pred.cpu().numpy()


def check_ties(dev):
    C, top_k = 8, 3
    rows, labels, want = [], [], []
    for lab in range(C):                                       # an all-equal row: rank = label
        rows.append(np.full(C, 1.25)); labels.append(lab); want.append(lab)
    straddle = np.asarray([5, 3, 3, 3, 3, 1, 1, 1.])           # a tie group over positions 1 .. 4 straddles top_k = 3
    for lab in range(1, 5):
        rows.append(straddle); labels.append(lab); want.append(lab)
    tie = np.asarray([0, 7, 2, 7, 2, 7, -1, 3.])               # the label first (1), in the middle (3) and last (5) of the maximal tie; 2: first / last of a lower tie
    for lab, r in ((1, 0), (3, 1), (5, 2), (2, 4), (4, 5)):
        rows.append(tie); labels.append(lab); want.append(r)
    logits = np.full((len(rows), 11), PAD_VALUE, np.float32)
    logits[:, :C] = np.asarray(rows, np.float32)
    labels = np.asarray(labels, np.int32)
    ref = reference(logits, C, labels, top_k)
    assert ref['rank'].tolist() == want
    got = run_once(logits, C, labels, top_k, dev)
    compare(got, ref, 'ties')
    hits_k = got['rank'] < top_k
    assert hits_k[8:12].tolist() == [True, True, False, False]
    pred = gap_pred(logits, C, dev)
    assert np.array_equal(got['rank'] == 0, labels == pred), (got['rank'], labels, pred)
    # and on random rows with natural ties
    lg, lb = make_case(16, 12, 12, 7)
    lg = np.round(lg)
    g2 = run_once(lg, 12, lb, 3, dev)
    compare(g2, reference(lg, 12, lb, 3), 'rounded rows')
    assert np.array_equal(g2['rank'] == 0, lb == gap_pred(lg, 12, dev))


def check_non_finite(dev):
    C, top_k = 6, 2
    nan, inf = np.nan, np.inf
    cases = [([1, nan, 0, 2, 3, 4.], 1, C),                    # NaN at the label: a miss, rank = C
             ([1, nan, 0, 2, nan, 4.], 3, 1),                  # NaN elsewhere compares false: only 4 > 2 counts
             ([1, 2, inf, 0, 3, 4.], 2, C),                    # +inf at the label, the others finite: a miss
             ([-inf, -inf, -inf, 0.5, -inf, -inf], 3, 0),      # -inf everywhere but one: the finite one wins ...
             ([-inf, -inf, -inf, 0.5, -inf, -inf], 0, C),      # ... and a -inf label is a miss
             ([-inf, -inf, -inf, -inf, -inf, -inf], 2, C),
             ([inf, 1, 2, 3, 4, 5.], 1, 5)]                    # +inf elsewhere is simply greater
    logits = np.asarray([c[0] for c in cases], np.float32)
    labels = np.asarray([c[1] for c in cases], np.int32)
    ref = reference(logits, C, labels, top_k)
    assert ref['rank'].tolist() == [c[2] for c in cases]
    assert np.isfinite(ref['loss']).tolist() == [False, False, False, True, False, False, False] and ref['loss'][3] == 0.0
    got = run_once(logits, C, labels, top_k, dev)
    compare(got, ref, 'non-finite')
    assert got['totals'].tolist() == [7, 1, 2, 0]


def check_bad_labels(dev):
    C = 5
    logits, labels = make_case(6, C, 8, 3)
    labels[1], labels[4] = -1, C
    start = dict(seen=torch.arange(C, dtype=torch.int32) + 3, hit=torch.arange(C, dtype=torch.int32), totals=torch.tensor([10, 20, 30, 40]),
                 loss_sum=torch.tensor([1.5], dtype=torch.float64))
    ref = reference(logits, C, labels, 2)
    got = run_once(logits, C, labels, 2, dev, init=start)
    assert got['rank'][1] == -1 and got['rank'][4] == -1 and np.isnan(got['loss'][[1, 4]]).all()
    assert np.array_equal(got['rank'], ref['rank'])
    assert (got['totals'] - np.asarray([10, 20, 30, 40])).tolist() == ref['totals'].tolist() and ref['totals'][3] == 2 and ref['totals'][0] == 4
    assert np.array_equal(got['seen'] - (np.arange(C) + 3), ref['seen']) and np.array_equal(got['hit'] - np.arange(C), ref['hit'])
    assert got['loss_sum'][0] == row_order_sum(got['loss'], ref['counted'], 1.5)
    only_bad = run_once(logits[:2], C, np.asarray([-1, C], np.int32), 2, dev, init=start)
    assert only_bad['totals'].tolist() == [10, 20, 30, 42] and np.array_equal(only_bad['seen'], np.arange(C) + 3)
    assert np.array_equal(only_bad['hit'], np.arange(C)) and only_bad['loss_sum'][0] == 1.5


def check_accumulation(dev):
    """two launches into the same accumulators == the sum of two single launches (the float64 sum: continued in row order); more rows than one chunk of
    the accumulating workgroup (256)"""
    C, top_k = 37, 5
    a_l, a_y = make_case(300, C, 40, 21)
    b_l, b_y = make_case(300, C, 40, 22)
    one_a, one_b = run_once(a_l, C, a_y, top_k, dev), run_once(b_l, C, b_y, top_k, dev)
    compare(one_a, reference(a_l, C, a_y, top_k), 'N=300 a')
    compare(one_b, reference(b_l, C, b_y, top_k), 'N=300 b')
    r = Run(300, C, dev)
    r.launch(torch.from_numpy(a_l).to(dev), 40, torch.from_numpy(a_y).to(dev), top_k)
    both = r.launch(torch.from_numpy(b_l).to(dev), 40, torch.from_numpy(b_y).to(dev), top_k)
    for k in ('totals', 'seen', 'hit'):
        assert np.array_equal(both[k], one_a[k] + one_b[k]), k
    assert np.array_equal(both['rank'], one_b['rank']) and np.array_equal(both['loss'], one_b['loss'])          # overwritten
    assert both['loss_sum'][0] == row_order_sum(one_b['loss'], np.ones(300, bool), one_a['loss_sum'][0])
    assert abs(both['loss_sum'][0] - (one_a['loss_sum'][0] + one_b['loss_sum'][0])) <= 1e-12 * abs(both['loss_sum'][0])
    r2 = Run(300, C, dev)
    r2.launch(torch.from_numpy(a_l).to(dev), 40, torch.from_numpy(a_y).to(dev), top_k)
    again = r2.launch(torch.from_numpy(b_l).to(dev), 40, torch.from_numpy(b_y).to(dev), top_k)
    assert again['loss_sum'].tobytes() == both['loss_sum'].tobytes()


REFUSALS = [(dict(C=0), r'C=0 outside'), (dict(C=1025, ldl=1025), r'C=1025 outside'), (dict(top_k=0), r'top_k=0 outside'),
            (dict(top_k=9), r'top_k=9 outside \[1, C=8\]'), (dict(N=0), r'N=0 outside'), (dict(N=65536), r'N=65536 outside'), (dict(ldl=7), r'ldl=7 is less than C=8')]
POINTERS = ['logits', 'labels', 'rank', 'loss', 'totals', 'loss_sum', 'class_seen', 'class_hit']


def check_refusals(dev):
    """every limit of the contract, matched on its message; nothing is launched (the buffers are far smaller than the refused sizes)"""
    import pytest
    from odtk import _lib, ops
    t = dict(logits=torch.zeros(2, 8).to(dev), labels=torch.zeros(2, dtype=torch.int32).to(dev), rank=torch.zeros(2, dtype=torch.int32).to(dev),
             loss=torch.zeros(2).to(dev), totals=torch.zeros(4, dtype=torch.int64).to(dev), loss_sum=torch.zeros(1, dtype=torch.float64).to(dev),
             class_seen=torch.zeros(8, dtype=torch.int32).to(dev), class_hit=torch.zeros(8, dtype=torch.int32).to(dev))

    def call(ptrs, ldl=8, N=2, C=8, top_k=3):
        ops.classify_eval(ptrs['logits'], ldl, N, C, ptrs['labels'], top_k, ptrs['rank'], ptrs['loss'], ptrs['totals'], ptrs['loss_sum'],
                          ptrs['class_seen'], ptrs['class_hit'])
    for kw, msg in REFUSALS:
        with pytest.raises(_lib.OdtkError, match='classify_eval: ' + msg):
            call(t, **kw)
    for name in POINTERS:
        with pytest.raises(_lib.OdtkError, match='classify_eval: null pointer'):
            call(dict(t, **{name: None}))
    call(t)                                                        # and the same arguments, unbroken, are accepted
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()
    assert int(t['totals'][0]) == 2


@contextlib.contextmanager
def count_device_to_host():
    """counts the device-to-host transfers torch is asked for (copy_ into a host tensor, .cpu(), .to(host), .item(), .tolist(), .numpy() of a device tensor)"""
    n = [0]
    T = torch.Tensor
    orig = {k: getattr(T, k) for k in ('copy_', 'cpu', 'to', 'item', 'tolist')}

    def copy_(self, src, *a, **k):
        if isinstance(src, T) and src.is_cuda and not self.is_cuda:
            n[0] += 1
        return orig['copy_'](self, src, *a, **k)

    def to(self, *a, **k):
        r = orig['to'](self, *a, **k)
        if self.is_cuda and not r.is_cuda:
            n[0] += 1
        return r

    def wrap(name):
        def f(self, *a, **k):
            if self.is_cuda:
                n[0] += 1
            return orig[name](self, *a, **k)
        return f
    T.copy_, T.to = copy_, to
    for name in ('cpu', 'item', 'tolist'):
        setattr(T, name, wrap(name))
    try:
        yield n
    finally:
        for k, v in orig.items():
            setattr(T, k, v)


def check_evaluator(dev):
    """ClassificationEvaluator over three batches (int64 labels, pitched logits) == the restatement over all rows; result() is ONE device-to-host copy;
    reset() clears"""
    import odtk
    C, top_k, B = 224, 5, 4
    ev = odtk.ClassificationEvaluator(C, top_k, device=dev)
    rows, labs = [], []
    for s in range(3):
        lg, lb = make_case(B, C, 232, 50 + s)
        if s == 1:
            lb[2] = C                                              # one invalid label
        rows.append(lg); labs.append(lb)
        ev.update(torch.from_numpy(lg).to(dev)[:, :C], torch.from_numpy(lb.astype(np.int64)).to(dev))
    with count_device_to_host() as copies:
        r = ev.result()
    if torch.device(dev).type == 'cuda':
        assert copies[0] == 1, copies
    ref = reference(np.concatenate(rows), C, np.concatenate(labs), top_k)
    assert r['num_images'] == 11 and r['invalid_labels'] == 1 and r['top_k'] == top_k
    assert r['top1'] == ref['totals'][1] / 11 and r['topk'] == ref['totals'][2] / 11
    assert np.array_equal(r['class_seen'], ref['seen'])
    want = np.where(ref['seen'] > 0, ref['hit'] / np.maximum(ref['seen'], 1), np.nan)
    assert np.array_equal(r['class_accuracy'], want, equal_nan=True) and np.isnan(r['class_accuracy']).any()
    c = ref['counted']
    assert abs(r['loss'] - ref['loss'][c].mean()) <= ref['bound'][c].mean()
    ev.reset()
    z = ev.result()
    assert z['num_images'] == 0 and z['invalid_labels'] == 0 and np.isnan(z['top1']) and np.isnan(z['loss']) and not z['class_seen'].any()
    import pytest
    for bad in (torch.zeros(B, C + 1), torch.zeros(B, C, dtype=torch.float64)):
        with pytest.raises(ValueError, match='update'):
            ev.update(bad.to(dev), torch.zeros(B, dtype=torch.int64).to(dev))
    with pytest.raises(ValueError, match='top_k'):
        odtk.ClassificationEvaluator(4, 5, device=dev)
