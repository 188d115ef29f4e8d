#!/usr/bin/env python
"""Writes tests/golden/jpeg/: small JPEG files (PIL's encoder = libjpeg-turbo) next to PIL's own decode of each as <name>.npy (u8 [h, w, 3]), the
expected output the decoder tests hold libodtk to, plus three files the decoder must refuse.  Pictures are a smooth gradient plus seeded noise, so AC
coefficients, both Huffman table classes and long codes occur.  Needs PIL; the tests read the outputs only.
    python tools/make_jpeg_fixtures.py              the JPEG files, PIL's decodes, manifest.json
    python tools/make_jpeg_fixtures.py --emulated   <name>.emu.npy for two pictures: this project's decode under the CPU emulation of csrc/jpeg.hip, which
                                                    the device result must equal byte for byte (tests/test_gpu_jpeg.py)
"""
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'jpeg')
EMULATED = ('s444_24x40', 's420_37x51')


def picture(w, h, seed, channels=3):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    for c in range(channels):
        g = 128 + 90 * np.sin((x * (0.11 + 0.05 * c) + y * (0.07 + 0.03 * c)) + c) + rng.normal(0, 14, (h, w))
        planes.append(g)
    a = np.clip(np.stack(planes, -1), 0, 255).astype(np.uint8)
    return a[..., 0] if channels == 1 else a


# name, width, height, mode, PIL save options
CASES = [
    ('s444_24x40', 24, 40, 'RGB', dict(quality=90, subsampling=0)),
    ('s422_37x51', 37, 51, 'RGB', dict(quality=90, subsampling=1)),
    ('s420_37x51', 37, 51, 'RGB', dict(quality=90, subsampling=2)),
    ('s420_8x8', 8, 8, 'RGB', dict(quality=90, subsampling=2)),
    ('s420_1x1', 1, 1, 'RGB', dict(quality=90, subsampling=2)),
    ('gray_19x23', 19, 23, 'L', dict(quality=90)),
    ('s420_64x48_rst', 64, 48, 'RGB', dict(quality=90, subsampling=2, restart_marker_blocks=2)),
    ('s420_40x24_q30', 40, 24, 'RGB', dict(quality=30, subsampling=2)),
    ('s420_40x24_q100', 40, 24, 'RGB', dict(quality=100, subsampling=2)),
    ('s420_40x24_q16bit', 40, 24, 'RGB', dict(subsampling=2, qtables=[[min(16 + 40 * i, 1000) for i in range(64)], [min(17 + 60 * i, 2000) for i in range(64)]])),
    ('s420_40x24_opt', 40, 24, 'RGB', dict(quality=90, subsampling=2, optimize=True)),
]
REFUSED = [
    ('progressive_24x24', 24, 24, 'RGB', dict(quality=90, progressive=True)),
    ('cmyk_16x16', 16, 16, 'CMYK', dict(quality=90)),
    ('rgb_16x16', 16, 16, 'RGB', dict(quality=90, keep_rgb=True)),
]


def main():
    from PIL import Image
    os.makedirs(OUT, exist_ok=True)
    manifest = {}
    for k, (name, w, h, mode, opts) in enumerate(CASES + REFUSED):
        if mode == 'CMYK':
            arr = np.concatenate([picture(w, h, 100 + k), picture(w, h, 200 + k, 1)[..., None]], -1)
        else:
            arr = picture(w, h, 100 + k, 1 if mode == 'L' else 3)
        buf = io.BytesIO()
        Image.fromarray(arr, mode).save(buf, 'JPEG', **opts)
        data = buf.getvalue()
        open(os.path.join(OUT, name + '.jpg'), 'wb').write(data)
        entry = {'width': w, 'height': h, 'mode': mode, 'bytes': len(data), 'refused': (name, w, h, mode, opts) in REFUSED}
        if not entry['refused']:
            dec = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
            assert dec.shape == (h, w, 3)
            np.save(os.path.join(OUT, name + '.npy'), dec)
            sub = opts.get('subsampling')
            entry['sampling'] = [1, 1] if mode == 'L' else {0: [1, 1], 1: [2, 1], 2: [2, 2]}[sub]
        manifest[name] = entry
    json.dump(manifest, open(os.path.join(OUT, 'manifest.json'), 'w'), indent=1, sort_keys=True)
    print('wrote', len(manifest), 'fixtures to', OUT)


def emulated():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, ROOT)
    import jpeg_cases as JC
    with JC.emulated():
        for name in EMULATED:
            out = JC.decode_batch([JC.fixture_bytes(name)], 'cpu')[0]
            np.save(os.path.join(OUT, name + '.emu.npy'), out)
            print(name, out.shape)


if __name__ == '__main__':
    emulated() if '--emulated' in sys.argv[1:] else main()
