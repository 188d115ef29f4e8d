"""CPU: `python bench.py --gpus N` must start its own ranks when no launcher did (round-1 verdict: the bare command died
on an assert before RCCL was touched), keep the ONE-JSON-line contract on rank 0, and still work under torchrun."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, env=None):
    e = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run(cmd, cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def _one_json_line(stdout):
    lines = [l for l in stdout.splitlines() if l.strip().startswith('{')]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def test_self_launch_two_ranks_gloo():
    r = _run([sys.executable, 'bench.py', '--gpus', '2', '--launch-check', '--steps', '4', '--warmup', '1'])
    assert r.returncode == 0, r.stderr[-2000:]
    out = _one_json_line(r.stdout)
    assert out['metric'] == 'launch-check' and out['n_gpus'] == 2 and out['steps'] == 4 and out['warmup'] == 1
    assert out['comm'] == {'backend': 'gloo', 'world_size': 2, 'launcher': 'self', 'allreduce_ok': True}
    for key in ('value', 'unit', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data', 'config'):
        assert key in out


def test_torchrun_launch_two_ranks_gloo():
    r = _run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
              '--master-port', '29731', 'bench.py', '--gpus', '2', '--launch-check', '--steps', '3', '--warmup', '1'])
    assert r.returncode == 0, r.stderr[-2000:]
    out = _one_json_line(r.stdout)
    assert out['n_gpus'] == 2 and out['comm']['world_size'] == 2 and out['comm']['launcher'] == 'external'


def test_mismatched_world_size_is_an_error_message_not_an_assert():
    r = _run([sys.executable, 'bench.py', '--gpus', '2', '--launch-check'], env={'WORLD_SIZE': '4', 'RANK': '0'})
    assert r.returncode != 0 and 'WORLD_SIZE=4' in r.stderr and 'Traceback' not in r.stderr


def test_dump_outputs_of_a_training_step(tmp_path):
    """`bench.py --dump-outputs DIR` writes what the last timed step computed: the loss, the loss terms, every variable after the update and its gradient,
    float32, large tensors as a sample whose indices depend only on the tensor's name (the same in every run, for a parameter and its gradient alike).
    Here on one SSD300 step through tests/mock_ops.py's launches."""
    import zlib
    import numpy as np
    import torch
    import bench
    import mock_ops
    import odtk
    from oracle import ssd300_ref as R
    torch.set_num_threads(8)
    cfg = {'mode': 'train', 'data_format': 'channels_last', 'num_classes': 20, 'weight_decay': 1e-4, 'keep_prob': 0.5, 'batch_size': 2,
           'nms_score_threshold': 0.5, 'nms_max_boxes': 20, 'nms_iou_threshold': 0.5, 'pretraining_weight': '', 'verbose': False,
           'compute_dtype': 'f32', 'seed': 0, 'use_graph': False, 'device': 'cpu'}
    imgs, gt = R.synthetic_batch(2, 31)
    with mock_ops.installed():
        m = odtk.SSD300(cfg, {'data_shape': [300, 300, 3], 'num_train': 2, 'num_val': 0, 'train_generator': [], 'val_generator': None})
        m.set_batch(imgs, gt)
        loss = m.train_step(0.01)
        bench.dump_outputs(m, loss, str(tmp_path / 'a'))
        bench.dump_outputs(m, loss, str(tmp_path / 'b'))
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted(os.listdir(tmp_path / 'b'))
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= bench.DUMP_LIMIT
    load = {f[:-4]: np.load(tmp_path / 'a' / f) for f in files}
    for f in files:
        assert load[f[:-4]].dtype == np.float32 and np.array_equal(load[f[:-4]], np.load(tmp_path / 'b' / f)), f
    assert load['loss'].tolist() == [np.float32(float(loss))]
    assert np.array_equal(load['loss_parts'], m.loss_parts.numpy())
    params = m.export_params()
    assert {k for k in load if k.startswith('param.')} == {'param.' + k for k in params}
    assert {k for k in load if k.startswith('grad.')} == {'grad.' + k for k in m.pinfo}
    sampled = 0
    for k, v in params.items():
        p = v.numpy().reshape(-1)
        g = m.get_param(k, m.G).numpy().reshape(-1) if k in m.pinfo else None
        if p.size <= bench.DUMP_SAMPLE:
            assert np.array_equal(load['param.' + k], v.numpy()), k
            assert g is None or np.array_equal(load['grad.' + k].reshape(-1), g), k
        else:
            sampled += 1
            idx = np.sort(np.random.default_rng(zlib.crc32(k.encode())).choice(p.size, bench.DUMP_SAMPLE, replace=False))
            assert np.array_equal(load['param.' + k], p[idx]), k
            assert np.array_equal(load['grad.' + k], g[idx]), k                 # the gradient at the same indices
    assert sampled > 0


def test_real_run_without_gpus_fails_loudly():
    r = _run([sys.executable, 'bench.py', '--gpus', '2', '--steps', '1'])
    assert r.returncode == 2 and 'GPU(s) visible' in r.stderr
    r = _run([sys.executable, 'bench.py', '--steps', '1'])
    assert r.returncode != 0 and 'no CPU fallback' in r.stderr
