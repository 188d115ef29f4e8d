"""Case bodies shared by tests/test_cpu_jpeg.py (csrc/jpeg.hip from source under the fiber emulation) and tests/test_gpu_jpeg.py (libodtk.so on the device).
Fixtures: tests/golden/jpeg/ (tools/make_jpeg_fixtures.py): JPEG files next to PIL's decode of each.

Bounds against PIL (libjpeg-turbo: integer IDCT, integer triangle filter), derived, not measured: both inverse DCTs are within 1 of the exact result, so Y,
Cb and Cr differ by at most 1 each before conversion; after the triangle filter and its rounding chroma differs by at most 2; the conversion and the two
roundings then give max |diff| <= 1 for grayscale, <= 3 for 4:4:4, <= 5 for subsampled pictures, borders included.  The mean |diff| is bounded at twice the
largest value the CPU emulation gave on any fixture (0.4247 on s420_40x24_q16bit): a half-level bias would show there and not in the max."""
import contextlib
import json
import os
import tempfile

import numpy as np
import torch

import hip_cpu_backend as HC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'jpeg')
MANIFEST = json.load(open(os.path.join(GOLDEN, 'manifest.json')))
DECODABLE = sorted(n for n, e in MANIFEST.items() if not e['refused'])
REFUSED = sorted(n for n, e in MANIFEST.items() if e['refused'])
MIXED = ['s420_1x1', 'gray_19x23', 's420_37x51', 's420_64x48_rst']
MEAN_BOUND = 2 * 0.4247


def fixture_bytes(name):
    return open(os.path.join(GOLDEN, name + '.jpg'), 'rb').read()


def fixture_rgb(name):
    return np.load(os.path.join(GOLDEN, name + '.npy'))


def max_bound(name):
    e = MANIFEST[name]
    return 1 if e['mode'] == 'L' else (3 if e['sampling'] == [1, 1] else 5)


@contextlib.contextmanager
def emulated():
    """the emulation with csrc/jpeg.hip in the build (a build of its own, cached in a directory of its own); hip_cpu_backend's module state is put back"""
    files, lib, tmp = list(HC.KERNEL_FILES), HC._LIB, tempfile.tempdir
    HC.KERNEL_FILES = files + ['jpeg.hip']
    HC._LIB = None
    tempfile.tempdir = os.path.join(tempfile.gettempdir(), f'odtk_cpu_jpeg_{os.getuid()}')
    os.makedirs(tempfile.tempdir, exist_ok=True)
    try:
        with HC.installed() as names:
            assert 'odtk_jpeg_reconstruct' in names
            yield
    finally:
        HC.KERNEL_FILES, HC._LIB, tempfile.tempdir = files, lib, tmp


def decode_batch(datas, dev, decoder=None):
    """list of JPEG byte strings -> list of u8 [h, w, 3] numpy arrays through JpegBatchDecoder (one odtk_jpeg_reconstruct for the whole list)"""
    from odtk.voc_data import JpegBatchDecoder
    dec = decoder if decoder is not None else JpegBatchDecoder(dev, threads=2)
    outs = dec(datas)
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()
    return [o.cpu().numpy().copy() for o in outs]


def check_fixture(name, dev, report=None):
    got = decode_batch([fixture_bytes(name)], dev)[0]
    want = fixture_rgb(name)
    assert got.shape == want.shape and got.dtype == np.uint8
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f'{name}: max |diff| {int(diff.max())} (bound {max_bound(name)}), mean |diff| {float(diff.mean()):.4f} (bound {MEAN_BOUND})')
    if report is not None:
        report[name] = (int(diff.max()), float(diff.mean()))
    assert int(diff.max()) <= max_bound(name), (name, int(diff.max()), np.argwhere(diff == diff.max())[:4].tolist())
    assert float(diff.mean()) <= MEAN_BOUND, (name, float(diff.mean()))


def check_mixed_batch(dev, order):
    names = [MIXED[i] for i in order]
    alone = [decode_batch([fixture_bytes(n)], dev)[0] for n in names]
    together = decode_batch([fixture_bytes(n) for n in names], dev)
    for n, a, b in zip(names, alone, together):
        assert a.shape == b.shape and np.array_equal(a, b), n


def check_many_copies(dev, copies=33, name='s420_37x51'):
    one = decode_batch([fixture_bytes(name)], dev)[0]
    outs = decode_batch([fixture_bytes(name)] * copies, dev)
    assert len(outs) == copies
    for k, o in enumerate(outs):
        assert np.array_equal(o, one), k


def check_decoder_reuse(dev):
    """a large batch, then a smaller one of other pictures through the same decoder: nothing of the first may show in the second"""
    from odtk.voc_data import JpegBatchDecoder
    dec = JpegBatchDecoder(dev, threads=2)
    first = ['s420_64x48_rst', 's422_37x51', 's444_24x40', 's420_37x51']
    second = ['gray_19x23', 's420_8x8']
    decode_batch([fixture_bytes(n) for n in first], dev, dec)
    stage = dec._stage.numel()
    got = decode_batch([fixture_bytes(n) for n in second], dev, dec)
    assert dec._stage.numel() == stage          # grown once, not shrunk
    for n, g in zip(second, got):
        assert np.array_equal(g, decode_batch([fixture_bytes(n)], dev)[0]), n


SHARD_PICTURES = ['s444_24x40', 's422_37x51', 's420_37x51', 'gray_19x23', 's420_64x48_rst', 's420_40x24_q30', 's420_40x24_q100', 's420_40x24_q16bit',
                  's420_40x24_opt', 's420_8x8', 's444_24x40', 's420_37x51']


def fixture_boxes(name, k):
    """two boxes well inside the picture: [ymin, ymax, xmin, xmax, class]"""
    e = MANIFEST[name]
    h, w = float(e['height']), float(e['width'])
    return np.asarray([[0.1 * h, 0.6 * h, 0.2 * w, 0.7 * w, k % 20], [0.3 * h, 0.9 * h, 0.4 * w, 0.95 * w, (k + 7) % 20]], np.float32)


def write_fixture_shards(directory, shards=2):
    """the twelve SHARD_PICTURES with their boxes as `.tfrecord` shards; returns (paths, [(name, boxes)] in record order)"""
    from odtk.voc_data import TFRecordWriter, encode_example
    paths, records = [], []
    per = -(-len(SHARD_PICTURES) // shards)
    for s in range(shards):
        paths.append(os.path.join(str(directory), 'fix_%05d-of-%05d.tfrecord' % (s + 1, shards)))
        with TFRecordWriter(paths[-1]) as w:
            for k in range(s * per, min((s + 1) * per, len(SHARD_PICTURES))):
                name = SHARD_PICTURES[k]
                e = MANIFEST[name]
                w.write(encode_example(fixture_bytes(name), [e['height'], e['width'], 1 if e['mode'] == 'L' else 3], fixture_boxes(name, k)))
                records.append((name, fixture_boxes(name, k)))
    return paths, records
