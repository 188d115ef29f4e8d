"""Bit-level fingerprint of what every detector class computes and stores, for refactors of the host code that must change neither.

    python tools/state_fingerprint.py --out fp.json                          # all cases on cuda:0, in one process
    python tools/state_fingerprint.py --case fcos --out fp.json              # one case; an existing --out file is merged into (one process per class on the GPU)
    python tools/state_fingerprint.py --device cpu --threads 8 --out fp.json # the CPU stand-in of the library (tests/mock_ops.py)
    python tools/state_fingerprint.py --diff a.json b.json                   # exit status 1 and the differing fields if the two differ
    python tools/state_fingerprint.py --full ...                             # keep the per-array hashes (to find WHICH variable differs)

It touches only the surface every revision of the package has -- bench_configs.make, set_batch, train_step, export_params, export_tf_variables,
save_weight / load_weight, test_one_image and the flat buffers -- so the same file runs in a checkout of an older commit.  Per case (the ten classes at
batch 2 and the smallest input their tests build them at, with an explicit engine; `<class>_warmup`: FCOS and CenterNet on bf16 with f32_warmup_steps=1,
so the second step crosses the hand-over from the f32 twin):
  steps ........ after each of two optimizer steps: the loss as a hex float, SHA-256 of P, G, every optimizer buffer and S
  tf_variables . SHA-256 of every array of export_tf_variables()
  checkpoint ... key set and tensor hashes of the torch file save_weight wrote, re-read
  loaded ....... SHA-256 of P and the optimizer buffers of a FRESH model after load_weight of that file, and its global_step
  detections ... SHA-256 of the three arrays test_one_image returns from a test-mode model (f32 engine) loaded with those parameters
  tf_loaded .... the same model saved with checkpoint_format='tf' (tf.train.Saver files) and load_weight of that prefix into a FRESH model: SHA-256 of P,
                 the optimizer buffers and S, and its global_step
  backbone_loaded  a FRESH model restored from that prefix through load_pretraining_weight / load_pretrained_weight (the classes that have one): SHA-256
                 of P and of the optimizer buffers, which must be the fresh model's own, and global_step
  graph_steps .. yolov3 and refinedet on the GPU: a model built with use_graph=True after FIVE steps (two eager, the capture, two replays): loss and state
  launches ..... every call of a plain function of odtk.ops during the two optimizer steps and the test-mode test_one_image, in order: the count and a
                 SHA-256 over the canonical calls (`canon`: a tensor is the ordinal of the first appearance of its data_ptr -- counted per model, the
                 trained one and the test-mode one --, dtype, shape and strides: independent of where the allocator put it; 'sha_without_ordinals': the same with the
                 ordinals taken out); --full keeps the list itself ('calls'), to locate a difference
The file keeps the first 64 bits of every hash.  Without --full the long tables -- the hashes of every array of export_tf_variables() and of every
entry of the checkpoint's 'params' and 'layout' -- are folded into {'n': count, 'sha': SHA-256 over the sorted 'name:hash' lines}, so that a file stays a page long.
"""
import argparse
import contextlib
import ctypes
import hashlib
import inspect
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# case -> (bench_configs name or 'lhrcnn', input size, engine)
CASES = {
    'ssd300': ('ssd300', 300, 'bf16'), 'ssd512': ('ssd512', 512, 'bf16'), 'yolov3': ('yolov3', 64, 'f32x3'), 'retinanet': ('retinanet', 128, 'f32x3'),
    'fcos': ('fcos', 128, 'bf16'), 'centernet': ('centernet', 64, 'bf16'), 'refinedet': ('refinedet', 320, 'f32'), 'pfpnet': ('pfpnet', 320, 'f32'),
    'yolov2': ('yolov2', 192, 'bf16'), 'lhrcnn': ('lhrcnn', (320, 416), 'f32'),
    'fcos_warmup': ('fcos', 128, 'bf16'), 'centernet_warmup': ('centernet', 64, 'bf16'),
}
BATCH, DATA_SEED = 2, 1000
HEX = 16           # hex digits kept of every SHA-256 (64 bits: the files hold some 10 000 hashes and stay small enough to commit)


def sha(t):
    import numpy as np
    import torch
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous()
        data = t.view(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b''
        return hashlib.sha256(str(t.dtype).encode() + str(tuple(t.shape)).encode() + data).hexdigest()[:HEX]
    a = np.ascontiguousarray(t)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()[:HEX]


TRACE = None        # while a list: every call through a plain function of odtk.ops is appended to it (trace_ops)
ORDINALS = {}       # data_ptr -> ordinal of its first appearance in the trace of the model that is running (cleared when the test-mode model takes over)


def canon(a):
    """an argument of a traced call as JSON-able data that does not depend on addresses"""
    import torch
    if isinstance(a, torch.Tensor):
        return ['T', ORDINALS.setdefault(a.data_ptr(), len(ORDINALS)), str(a.dtype), list(a.shape), list(a.stride())]
    if isinstance(a, ctypes.Array) and a._type_ is ctypes.c_void_p:          # a table of addresses (the per-level tensors of a loss): its elements read back as ints
        return [canon(ctypes.c_void_p(x)) for x in a]
    if isinstance(a, (list, tuple, ctypes.Array)):
        return [canon(x) for x in a]
    if isinstance(a, dict):
        return {str(k): canon(v) for k, v in sorted(a.items(), key=lambda kv: str(kv[0]))}
    if isinstance(a, ctypes.Structure):
        return {'struct': type(a).__name__, 'fields': [canon(getattr(a, f[0])) for f in a._fields_]}
    if isinstance(a, ctypes.c_void_p):                         # the real library's call layer gets raw addresses: numbered like the tensors they point into
        return ['P', None if a.value is None else ORDINALS.setdefault(a.value, len(ORDINALS))]
    if type(a).__name__ == 'CArgObject':                       # ctypes.byref(structure)
        return canon(a._obj)
    if isinstance(a, float):
        return a.hex()
    r = repr(a)
    if ' at 0x' in r and hasattr(a, '__dict__'):          # a plain object (a workspace holder): its type and what it holds
        return {'object': type(a).__name__, 'vars': canon(vars(a))}
    return r


def without_ordinals(x):
    """the trace with the tensor / address ordinals taken out: what is left to compare where two runs of ONE revision number them differently"""
    if isinstance(x, list):
        if len(x) == 5 and x[0] == 'T':
            return ['T'] + x[2:]
        if len(x) == 2 and x[0] == 'P':
            return ['P']
        return [without_ordinals(v) for v in x]
    return {k: without_ordinals(v) for k, v in x.items()} if isinstance(x, dict) else x


def trace_ops():
    """wrap the plain functions of odtk.ops (the real launches, or the CPU stand-in's once mock_ops.installed() has swapped them in): the classes call
    `ops.name(...)` through the module, so every call lands in TRACE while it is a list"""
    from odtk import ops

    def traced(name, fn):
        def w(*a, **k):
            if TRACE is not None:
                TRACE.append([name] + [canon(x) for x in a] + [[n, canon(v)] for n, v in sorted(k.items())])
            return fn(*a, **k)
        w.__name__ = name
        return w
    for name, fn in list(vars(ops).items()):
        if inspect.isfunction(fn) and not name.startswith('_'):
            setattr(ops, name, traced(name, fn))


@contextlib.contextmanager
def tracing(calls):
    global TRACE
    TRACE = calls
    try:
        yield
    finally:
        TRACE = None


def build(kind, size, engine, device, mode='train', **extra):
    """-> (model, images, gt, lr)"""
    import torch
    import bench_configs
    import odtk
    batch = BATCH if mode == 'train' else 1
    if kind != 'lhrcnn':
        if mode == 'test':           # a low threshold: a twice-stepped random initialisation should still give detections to hash
            extra.update(score_threshold=0.05) if kind == 'centernet' else extra.update(nms_score_threshold=0.05)
        r = bench_configs.make(kind, batch=batch, size=size, dtype=engine, seed=DATA_SEED, mode=mode, device=device, **extra)
        if kind == 'retinanet' and mode == 'train' and 'mock_ops' in sys.modules:
            sys.modules['mock_ops'].retina_loss.anchors = r['model'].anc          # the CPU stand-in's loss matches internally, on the model's anchors
        return r['model'], r['images'], r['gt'], r['lr']
    h, w = size
    g = torch.Generator().manual_seed(DATA_SEED)
    images = (torch.rand(batch, h, w, 3, generator=g) * 255).round()
    gt = bench_configs.synthetic_gt(batch, h, DATA_SEED + 1, lo=0.1, hi=0.7)
    cfg = {'data_shape': [h, w, 3], 'mode': mode, 'is_pretraining': False, 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4,
           'keep_prob': 0.5, 'batch_size': batch, 'rpn_first_step': 1, 'rcnn_first_step': 100000, 'rpn_second_step': 160000,
           'nms_score_threshold': 0.05 if mode == 'test' else 0.5, 'nms_max_boxes': 20, 'nms_iou_threshold': 0.45, 'post_nms_proposal': 500, 'verbose': False,
           'device': device, 'compute_dtype': engine}
    cfg.update(extra)
    prov = {'data_shape': [h, w, 3], 'num_train': batch, 'num_val': 0, 'train_generator': [(images, gt)], 'val_generator': None}
    return odtk.LHRCNN(cfg, prov if mode == 'train' else None), images, gt, 0.003


def opt_buffers(m):
    return tuple(getattr(m, 'OPT_BUFFERS', ('Mom',)))


def state(m):
    out = {'P': sha(m.P), 'G': sha(m.G)}
    for name in opt_buffers(m):
        out[name] = sha(getattr(m, name))
    if hasattr(m, 'S'):
        out['S'] = sha(m.S)
    return out


def loaded_state(m):
    out = {n: sha(getattr(m, n)) for n in ('P',) + opt_buffers(m)}
    if hasattr(m, 'S'):
        out['S'] = sha(m.S)
    return out


def hash_tree(v):
    import torch
    if isinstance(v, torch.Tensor):
        return sha(v)
    if isinstance(v, dict):
        return {str(k): hash_tree(x) for k, x in v.items()}
    return hashlib.sha256(repr(v).encode()).hexdigest()[:HEX]


def fingerprint(case, device):
    import torch
    kind, size, engine = CASES[case]
    extra = {'f32_warmup_steps': 1} if case.endswith('_warmup') else {}
    m, images, gt, lr = build(kind, size, engine, device, **extra)
    rec = {'class': type(m).__name__, 'engine': engine, 'size': size, 'steps': []}
    m.set_batch(images, gt)
    calls = []
    ORDINALS.clear()
    for _ in range(2):
        with tracing(calls):
            loss = float(torch.as_tensor(m.train_step(lr)).reshape(-1)[0].item())
        rec['steps'].append(dict(state(m), loss=loss.hex()))
    rec['tf_variables'] = {k: sha(v) for k, v in m.export_tf_variables().items()}
    params = m.export_params()
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, 'ckpt')
        m.save_weight('latest', prefix)
        path = prefix + '-' + str(m.global_step)
        blob = torch.load(path, map_location='cpu', weights_only=True)
        rec['checkpoint'] = {'keys': sorted(blob), 'hashes': hash_tree(blob)}
        fresh = build(kind, size, engine, device)[0]
        fresh.load_weight(path)
        rec['loaded'] = dict({n: sha(getattr(fresh, n)) for n in ('P',) + opt_buffers(fresh)}, global_step=int(fresh.global_step))
        m.config['checkpoint_format'] = 'tf'
        tf_prefix = os.path.join(tmp, 'saver')
        m.save_weight('latest', tf_prefix)
        tf_path = tf_prefix + '-' + str(m.global_step)
        fresh = build(kind, size, engine, device)[0]
        fresh.load_weight(tf_path)
        rec['tf_loaded'] = dict(loaded_state(fresh), global_step=int(fresh.global_step))
        fresh = build(kind, size, engine, device)[0]
        restore = getattr(fresh, 'load_pretraining_weight', None) or getattr(fresh, 'load_pretrained_weight', None)
        if restore is not None:
            untouched = {n: sha(getattr(fresh, n)) for n in opt_buffers(fresh)}
            restore(tf_path)
            rec['backbone_loaded'] = dict(loaded_state(fresh), global_step=int(fresh.global_step), untouched=untouched)
    del m, fresh
    if kind in ('yolov3', 'refinedet') and torch.device(device).type != 'cpu':
        g, images, gt, lr = build(kind, size, engine, device, use_graph=True)
        g.set_batch(images, gt)
        for _ in range(5):
            loss = float(torch.as_tensor(g.train_step(lr)).reshape(-1)[0].item())
        rec['graph_steps'] = dict(state(g), loss=loss.hex(), captured=g._graph is not None)
        del g
    t, images, _, _ = build(kind, size, 'f32', device, mode='test')
    t.load_oracle_params(params)
    ORDINALS.clear()                     # a new model: its buffers may sit where freed ones of the trained model sat, ordinals count from here again
    try:
        with tracing(calls):
            scores, bbox, cid = t.test_one_image(images[:1].numpy())
        rec['detections'] = {'n': int(len(scores)), 'scores': sha(scores), 'bbox': sha(bbox), 'class_id': sha(cid)}
    except AssertionError as e:          # the CPU stand-in has no decode / NMS launch for some classes: 'libodtk takes device pointers'
        if torch.device(device).type != 'cpu':
            raise
        rec['detections'] = {'n': -1, 'unavailable': str(e)}
    rec['launches'] = {'n': len(calls), 'sha': hashlib.sha256(json.dumps(calls).encode()).hexdigest()[:HEX], 'calls': calls,
                       'sha_without_ordinals': hashlib.sha256(json.dumps(without_ordinals(calls)).encode()).hexdigest()[:HEX]}
    return rec


def fold(table):
    lines = ''.join(f'{k}:{v}\n' for k, v in sorted(table.items()))
    return {'n': len(table), 'sha': hashlib.sha256(lines.encode()).hexdigest()[:HEX]}


def compact(rec):
    rec = dict(rec, tf_variables=fold(rec['tf_variables']), checkpoint=dict(rec['checkpoint'], hashes=dict(rec['checkpoint']['hashes'])))
    rec['launches'] = {k: v for k, v in rec['launches'].items() if k != 'calls'}
    for k in ('params', 'layout'):
        if isinstance(rec['checkpoint']['hashes'].get(k), dict) and 'sha' not in rec['checkpoint']['hashes'][k]:
            rec['checkpoint']['hashes'][k] = fold(rec['checkpoint']['hashes'][k])
    return rec


def diff(a, b, path=''):
    if isinstance(a, dict) and isinstance(b, dict):
        out = []
        for k in sorted(set(a) | set(b)):
            out += diff(a.get(k), b.get(k), f'{path}/{k}')
        return out
    if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in diff(x, y, f'{path}[{i}]')]
    return [] if a == b else [path]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--case', action='append', choices=sorted(CASES), help='default: all')
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--threads', type=int, default=8, help='torch threads (fixed: the CPU stand-in reduces in thread-count-dependent order)')
    ap.add_argument('--out')
    ap.add_argument('--full', action='store_true', help='keep the per-array hashes of the TF variables and of the checkpoint parameters')
    ap.add_argument('--diff', nargs=2, metavar=('A', 'B'))
    args = ap.parse_args()
    if args.diff:
        a, b = (json.load(open(p)) for p in args.diff)
        a.pop('_meta', None); b.pop('_meta', None)
        d = diff(a, b)
        print(f'{len(d)} differing fields' + ''.join('\n  ' + p for p in d[:40]))
        sys.exit(1 if d else 0)
    import torch
    torch.set_num_threads(args.threads)
    out = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
    cpu = torch.device(args.device).type == 'cpu'
    if cpu:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import mock_ops
    with (mock_ops.installed() if cpu else contextlib.nullcontext()):
        trace_ops()
        for case in args.case or list(CASES):
            tables = contextlib.nullcontext()
            if cpu and case == 'ssd512':         # the mocked box-side launches call the oracle, which reads the swapped tables
                from oracle import ssd512_ref
                tables = ssd512_ref.tables()
            with tables:
                rec = fingerprint(case, args.device)
                out[case] = rec if args.full else compact(rec)
            print(case, 'loss', [float.fromhex(s['loss']) for s in out[case]['steps']], 'P', out[case]['steps'][-1]['P'][:12],
                  'detections', out[case]['detections']['n'], flush=True)
    out['_meta'] = {'device': torch.cuda.get_device_name(0) if not cpu else 'cpu mock', 'torch': torch.__version__, 'threads': args.threads}
    if args.out:
        with open(args.out, 'w') as f:
            f.write('{\n' + ',\n'.join(f' {json.dumps(k)}: {json.dumps(out[k], sort_keys=True)}' for k in sorted(out)) + '\n}\n')      # one line per case


if __name__ == '__main__':
    main()
