#!/usr/bin/env python
"""Loader benchmark (needs an MI355X and PIL): 64 pictures of 500 x 375, 4:2:0, quality 90, made from a seeded smooth-plus-noise image.  Prints ONE JSON line:
entropy decode images/s at 1 / 4 / 16 threads, odtk_jpeg_reconstruct time by HIP events and its GB/s against the achievable HBM rate (6.3 TB/s),
JpegBatchDecoder and get_generator (SSD300's augmentor config) images/s end to end, and PIL's Image.open(..).convert('RGB') on the same thread counts.
Every figure: warm-up first, then `--reps` repetitions, median with min and max."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from make_jpeg_fixtures import picture          # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def spread(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--pictures', type=int, default=64)
    a = ap.parse_args()
    from PIL import Image
    import odtk  # noqa: F401
    from odtk.voc_data import JpegBatchDecoder, TFRecordWriter, encode_example, get_generator
    assert torch.cuda.is_available(), 'jpeg_bench needs an MI355X'
    dev = torch.device('cuda:0')
    datas = []
    for k in range(a.pictures):
        buf = io.BytesIO()
        Image.fromarray(picture(500, 375, 1000 + k), 'RGB').save(buf, 'JPEG', quality=90, subsampling=2)
        datas.append(buf.getvalue())
    N = len(datas)
    res = {'pictures': N, 'jpeg_bytes_mean': sum(map(len, datas)) / N, 'reps': a.reps}
    for th in (1, 4, 16):
        dec = JpegBatchDecoder(dev, threads=th)
        dec.entropy(datas)
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); dec.entropy(datas); t.append(N / (time.perf_counter() - t0))
        res[f'entropy_images_per_s_{th}t'] = spread(t)
        with ThreadPoolExecutor(th) as pool:
            f = lambda d: np.asarray(Image.open(io.BytesIO(d)).convert('RGB'))      # noqa: E731
            list(pool.map(f, datas))
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); list(pool.map(f, datas)); t.append(N / (time.perf_counter() - t0))
        res[f'pil_images_per_s_{th}t'] = spread(t)
    dec = JpegBatchDecoder(dev, threads=16)
    hb = dec.entropy(datas)
    dec.reconstruct(hb); torch.cuda.synchronize()
    # the reconstruct launches alone: re-run them on the uploaded batch
    from odtk import ops
    qt_at, plan_at, nbytes = dec._sizes(hb.infos, hb.coef_elems)
    ms = []
    for _ in range(a.reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); ops.jpeg_reconstruct(dec._dev_in[plan_at:], N); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[2:]
    coef_bytes = sum(int(i.coef_count) for i in hb.infos)
    moved = 2 * coef_bytes + 2 * coef_bytes + sum(i.width * i.height * 3 for i in hb.infos)      # coefficients in, planes out and in again, RGB out
    res['reconstruct_ms'] = spread(ms)
    res['reconstruct_bytes'] = moved
    res['reconstruct_GBps'] = moved / (statistics.median(ms) * 1e-3) / 1e9
    res['reconstruct_share_of_achievable_hbm'] = moved / (statistics.median(ms) * 1e-3) / HBM_ACHIEVABLE
    dec(datas); torch.cuda.synchronize()
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter(); dec(datas); torch.cuda.synchronize(); t.append(N / (time.perf_counter() - t0))
    res['decoder_images_per_s'] = spread(t)
    cfg = {'data_format': 'channels_last', 'output_shape': [300, 300], 'crop_method': 'random', 'flip_prob': [0., 0.5], 'fill_mode': 'BILINEAR',
           'keep_aspect_ratios': False, 'constant_values': 0., 'color_jitter_prob': 0.5, 'rotate': [0.5, -5., -5.], 'pad_truth_to': 60}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'bench.tfrecord')
        with TFRecordWriter(path) as w:
            for k, data in enumerate(datas):
                w.write(encode_example(data, [375, 500, 3], [[50, 300, 60, 400, k % 20]]))
        it = iter(get_generator([path], 32, N, cfg, device=dev, seed=0, prefetch=2))
        for _ in range(4):
            next(it)
        torch.cuda.synchronize()
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(8):
                next(it)
            torch.cuda.synchronize(); t.append(8 * 32 / (time.perf_counter() - t0))
        it.close()
    res['generator_images_per_s'] = spread(t)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
