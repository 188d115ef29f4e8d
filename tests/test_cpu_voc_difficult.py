"""The `<difficult>` flag from the VOC annotation to the generator's sixth ground-truth column, on the CPU tier: the XML parser, the record feature
(absent unless asked for: the default records stay byte-identical), parse_example, and get_generator(with_difficult=True) through the real worker and
the augmentor's box kernel (csrc/augment.hip from source, tests/hip_cpu) with scripted draws that crop boxes out of the picture."""
import os

import numpy as np
import pytest
import torch

import hip_cpu_backend as HC
import jpeg_cases as JC

PICTURES = ['s420_64x48_rst', 's420_37x51']
# (class name, corner fractions of the picture (y0, x0, y1, x1), <difficult> text or None = no tag).  The augmentor below zooms to 32 x 32 and cuts a
# 16 x 16 window: a box over (0.6 .. 0.9) of both sides has its centre at 24 of 32, one over (0.1 .. 0.4) at 8 of 32.
OBJECTS = [('dog', (0.6, 0.6, 0.9, 0.9), '1'), ('cat', (0.1, 0.1, 0.4, 0.4), '0'), ('car', (0.6, 0.6, 0.9, 0.9), None),
           ('bus', (0.1, 0.1, 0.4, 0.4), '1'), ('cow', (0.6, 0.6, 0.9, 0.9), '0')]
CONFIG = {'data_format': 'channels_last', 'output_shape': [16, 16], 'zoom_size': [32, 32], 'crop_method': 'random', 'fill_mode': 'BILINEAR',
          'keep_aspect_ratios': False, 'constant_values': 0., 'pad_truth_to': 6}
DRAWS = [[16, 16], [0, 0]]               # picture 0: the lower right window (dog, car, cow stay); picture 1: the upper left one (cat, bus stay)


def _vd():
    import odtk  # noqa: F401
    from odtk import voc_data
    return voc_data


def expected_columns():
    """class and flag columns [2, 6] of the batch of the two pictures under DRAWS"""
    vd = _vd()
    ids = vd.classname_to_ids
    cls = np.full((2, 6), -1.0, np.float32)
    flag = np.full((2, 6), -1.0, np.float32)
    cls[0, :3], flag[0, :3] = [ids['dog'], ids['car'], ids['cow']], [1, 0, 0]
    cls[1, :2], flag[1, :2] = [ids['cat'], ids['bus']], [0, 1]
    return cls, flag


def voc_dir(tmp_path, difficult_text=None):
    xml_dir, img_dir = tmp_path / 'Annotations', tmp_path / 'JPEGImages'
    xml_dir.mkdir(), img_dir.mkdir()
    for k, name in enumerate(PICTURES):
        e = JC.MANIFEST[name]
        w, h = e['width'], e['height']
        objs = ''
        for n, (cname, (y0, x0, y1, x1), diff) in enumerate(OBJECTS):
            if difficult_text is not None and n == 0:
                diff = difficult_text
            tag = '' if diff is None else f'<difficult>{diff}</difficult>'
            objs += (f'<object><name>{cname}</name>{tag}<bndbox><xmin>{x0 * w}</xmin><ymin>{y0 * h}</ymin><xmax>{x1 * w}</xmax><ymax>{y1 * h}</ymax>'
                     f'</bndbox></object>\n')
        (img_dir / f'{k:06d}.jpg').write_bytes(JC.fixture_bytes(name))
        (xml_dir / f'{k:06d}.xml').write_text(f'<annotation><filename>{k:06d}.jpg</filename><size><width>{w}</width><height>{h}</height><depth>3</depth>'
                                              f'</size>\n{objs}</annotation>')
    return str(xml_dir), str(img_dir)


def test_xml_difficult_and_the_record_feature(tmp_path):
    vd = _vd()
    xml_dir, img_dir = voc_dir(tmp_path)
    xml = os.path.join(xml_dir, '000000.xml')
    plain = vd.xml_to_example(xml, img_dir)
    ex = vd.parse_example(plain)
    assert 'difficult' not in ex and ex['ground_truth'].shape == (5, 5)
    assert plain == vd.encode_example(ex['image'], ex['shape'], ex['ground_truth'])        # the parent's writer on the same inputs: byte-identical
    flagged = vd.parse_example(vd.xml_to_example(xml, img_dir, with_difficult=True))
    assert flagged['difficult'].dtype == np.uint8 and flagged['difficult'].tolist() == [1, 0, 0, 1, 0]           # 1, 0, absent, 1, 0
    assert np.array_equal(flagged['ground_truth'], ex['ground_truth']) and flagged['image'] == ex['image']
    assert vd.xml_to_example(xml, img_dir, with_difficult=True) == vd.encode_example(ex['image'], ex['shape'], ex['ground_truth'], [1, 0, 0, 1, 0])
    # the shards: default = the parent's records, with_difficult = the same plus the feature
    a = vd.dataset2tfrecord(xml_dir, img_dir, str(tmp_path / 'a'), 'voc', total_shards=1)
    b = vd.dataset2tfrecord(xml_dir, img_dir, str(tmp_path / 'b'), 'voc', total_shards=1, with_difficult=True)
    ra, rb = list(vd.tf_record_iterator(a[0])), list(vd.tf_record_iterator(b[0]))
    assert len(ra) == len(rb) == 2
    for k, (x, y) in enumerate(zip(ra, rb)):
        px = vd.parse_example(x)
        assert x == vd.encode_example(px['image'], px['shape'], px['ground_truth']) and 'difficult' not in px
        py = vd.parse_example(y)
        assert py['difficult'].tolist() == [1, 0, 0, 1, 0] and np.array_equal(py['ground_truth'], px['ground_truth']) and py['image'] == px['image']


def test_xml_difficult_refusals(tmp_path):
    vd = _vd()
    xml_dir, img_dir = voc_dir(tmp_path, difficult_text='2')
    xml = os.path.join(xml_dir, '000001.xml')
    with pytest.raises(ValueError, match=r'000001\.xml: <difficult>2</difficult> of object 0'):
        vd.xml_to_example(xml, img_dir, with_difficult=True)
    assert vd.parse_example(vd.xml_to_example(xml, img_dir))['ground_truth'].shape == (5, 5)          # not read unless asked for
    with pytest.raises(ValueError, match='3 flags for 2 ground-truth rows'):
        vd.encode_example(b'x', [1, 1, 3], np.zeros((2, 5)), [0, 1, 0])
    from odtk.tf_checkpoint import _pb_bytes
    entries = [vd._feature('image', b'x'), vd._feature('shape', np.array([1, 1, 3], np.int32).tobytes()),
               vd._feature('ground_truth', np.zeros((2, 5), np.float32).tobytes()), vd._feature('difficult', bytes([0]))]
    with pytest.raises(ValueError, match='1 difficult flags for 2 ground-truth rows'):
        vd.parse_example(_pb_bytes(1, b''.join(_pb_bytes(1, e) for e in entries)))


class _AsDevice(torch.Tensor):
    """a CPU tensor that answers `is_cuda` like a device tensor (the Augmentor insists on device tensors; the emulated kernels take host pointers)"""
    @property
    def is_cuda(self):
        return True


@pytest.fixture()
def augment_on_cpu(monkeypatch):
    import odtk  # noqa: F401
    from odtk import _lib, augment
    lib = HC.build()
    for n in ('odtk_augment_workspace_bytes', 'odtk_augment_boxes', 'odtk_augment_images'):
        f = getattr(lib, n)
        f.restype, f.argtypes = _lib.SIGNATURES[n]

    def call(name, *args):
        rc = getattr(lib, name)(*args)
        assert rc == 0, lib.odtk_last_error().decode()
    monkeypatch.setattr(augment, 'call', call)
    monkeypatch.setattr(augment, 'call_ll', lambda name, *args: int(getattr(lib, name)(*args)))
    monkeypatch.setattr(augment._lib, 'load', lambda: lib)
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a, **k: type('S', (), {'cuda_stream': 0})())
    monkeypatch.setattr(torch.Tensor, 'record_stream', lambda self, s: None)
    return lambda t: torch.Tensor._make_subclass(_AsDevice, t.contiguous())


class _FixtureDecoder:
    """the two device stages' first: the fixture's decoded picture looked up by its JPEG bytes (the decoder itself: tests/test_cpu_jpeg.py)"""

    def __init__(self, wrap):
        self.wrap, self.by_bytes = wrap, {JC.fixture_bytes(n): n for n in PICTURES}

    def entropy(self, datas):
        return [self.by_bytes[bytes(d)] for d in datas]

    def reconstruct(self, names):
        return [self.wrap(torch.from_numpy(JC.fixture_rgb(n).copy())) for n in names]


def scripted(augmentor):
    return lambda images, gts: augmentor(images, gts, draws=[list(d) for d in DRAWS])


def check_batch(gt, with_flags):
    cls, flag = expected_columns()
    g = gt.cpu().numpy()
    assert g.shape == (2, 6, 6 if with_flags else 5) and np.array_equal(g[..., 4], cls)
    if with_flags:
        assert np.array_equal(g[..., 5], flag)
    real = cls >= 0
    assert np.all(g[..., :4][real] > 0) and np.all(g[..., :4][~real] == -1)


def test_generator_sixth_column_follows_the_boxes_through_the_crop(tmp_path, augment_on_cpu):
    vd = _vd()
    from odtk.augment import Augmentor
    xml_dir, img_dir = voc_dir(tmp_path)
    flagged = vd.dataset2tfrecord(xml_dir, img_dir, str(tmp_path / 'f'), 'voc', total_shards=1, with_difficult=True)
    plain = vd.dataset2tfrecord(xml_dir, img_dir, str(tmp_path / 'p'), 'voc', total_shards=1)
    aug = Augmentor(**CONFIG)

    def first(paths, **kw):
        it = iter(vd.get_generator(paths, 2, 1, CONFIG, device='cpu', seed=0, decoder=_FixtureDecoder(augment_on_cpu), augmentor=scripted(aug), **kw))
        try:
            return next(it)
        finally:
            it.close()
    img, gt = first(flagged, with_difficult=True)
    assert tuple(img.shape) == (2, 16, 16, 3)
    check_batch(gt, True)
    _, gt5 = first(flagged)                                                   # new records, old reader: five columns, the feature is skipped
    check_batch(gt5, False)
    assert np.array_equal(gt.cpu().numpy()[..., :5], gt5.cpu().numpy())
    _, gt0 = first(plain, with_difficult=True)                                # old records, new reader: flag 0 wherever there is a box
    g0 = gt0.cpu().numpy()
    assert np.array_equal(g0[..., :5], gt5.cpu().numpy()) and np.array_equal(g0[..., 5], np.where(g0[..., 4] >= 0, 0, -1))
