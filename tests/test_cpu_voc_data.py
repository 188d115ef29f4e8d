"""CPU tier of odtk.voc_data: record framing, Example layout, VOC annotations, shard writing, and the generator's host logic with both device stages mocked."""
import json
import os
import re
import struct
import threading

import numpy as np
import pytest
import torch

import jpeg_cases as JC


def _vd():
    import odtk  # noqa: F401
    from odtk import voc_data
    return voc_data


def test_class_table_is_pinned():
    vd = _vd()
    want = json.load(open(os.path.join(JC.GOLDEN, 'voc_classes.json')))
    assert vd.classname_to_ids == want and len(vd.VOC_CLASSES) == 20 and sorted(want.values()) == list(range(20))
    import odtk
    assert odtk.VOC_CLASSES is vd.VOC_CLASSES and odtk.get_generator is vd.get_generator


# ---------------------------------------------------------------- framing
def test_tfrecord_round_trip_and_hand_written_framing(tmp_path):
    vd = _vd()
    from odtk.tf_checkpoint import crc32c
    recs = [b'', b'x', bytes(range(256)) * 5]
    p = str(tmp_path / 'a.tfrecord')
    with vd.TFRecordWriter(p) as w:
        for r in recs:
            w.write(r)
    assert list(vd.tf_record_iterator(p)) == recs and list(vd.tf_record_iterator(p, verify=False)) == recs

    def masked(b):
        c = crc32c(b)
        return ((((c >> 15) | (c << 17)) & 0xffffffff) + 0xa282ead8) & 0xffffffff
    one = str(tmp_path / 'one.tfrecord')
    with vd.TFRecordWriter(one) as w:
        w.write(b'hello')
    head = struct.pack('<Q', 5)
    assert open(one, 'rb').read() == head + struct.pack('<I', masked(head)) + b'hello' + struct.pack('<I', masked(b'hello'))
    assert crc32c(b'123456789') == 0xe3069283            # the CRC32C check value


def test_tfrecord_errors_name_the_offset(tmp_path):
    vd = _vd()
    p = str(tmp_path / 'a.tfrecord')
    with vd.TFRecordWriter(p) as w:
        w.write(b'first record')
        w.write(b'second record!')
    raw = bytearray(open(p, 'rb').read())
    second = 16 + len(b'first record')
    bad = bytearray(raw)
    bad[second + 12 + 3] ^= 0x40
    open(p, 'wb').write(bad)
    it = vd.tf_record_iterator(p)
    assert next(it) == b'first record'
    with pytest.raises(vd.TFRecordError, match=f'offset {second} '):
        next(it)
    assert len(list(vd.tf_record_iterator(p, verify=False))) == 2
    open(p, 'wb').write(raw[:-3])
    with pytest.raises(vd.TFRecordError, match=f'truncated record at byte offset {second} '):
        list(vd.tf_record_iterator(p))
    open(p, 'wb').write(raw[:second + 5])
    with pytest.raises(vd.TFRecordError, match=f'header at byte offset {second} '):
        list(vd.tf_record_iterator(p))


# ---------------------------------------------------------------- Example
def _varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7f) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def _ld(field, payload):
    return _varint((field << 3) | 2) + _varint(len(payload)) + payload


def test_example_round_trip_and_foreign_order():
    vd = _vd()
    gt = np.asarray([[1, 2, 3, 4, 5], [6.5, 7.5, 8.5, 9.5, 19]], np.float32)
    ex = vd.parse_example(vd.encode_example(b'\xff\xd8jpeg', [375, 500, 3], gt))
    assert ex['image'] == b'\xff\xd8jpeg' and ex['shape'].tolist() == [375, 500, 3] and ex['shape'].dtype == np.int32
    assert np.array_equal(ex['ground_truth'], gt) and ex['ground_truth'].dtype == np.float32
    assert vd.parse_example(vd.encode_example(b'i', [1, 1, 3], np.zeros((0, 5))))['ground_truth'].shape == (0, 5)

    def entry(key, feature):
        return _ld(1, _ld(1, key.encode()) + _ld(2, feature))

    def bytes_feature(v):
        return _ld(1, _ld(1, v))
    int64_feature = _ld(3, _ld(1, _varint(7)))                  # Feature.int64_list: an extra feature of another kind
    features = (entry('ground_truth', bytes_feature(gt.tobytes())) + entry('extra', int64_feature) + entry('shape', bytes_feature(np.asarray([2, 3, 1], np.int32).tobytes()))
                + entry('image', bytes_feature(b'abc')))
    ex = vd.parse_example(_ld(1, features))
    assert ex['image'] == b'abc' and ex['shape'].tolist() == [2, 3, 1] and np.array_equal(ex['ground_truth'], gt)
    with pytest.raises(ValueError, match='image'):
        vd.parse_example(_ld(1, entry('shape', bytes_feature(b'\0' * 12)) + entry('ground_truth', bytes_feature(b''))))


# ---------------------------------------------------------------- annotations
XML = """<annotation><folder>VOC2007</folder><filename>{name}.jpg</filename>
<size><width>{w}</width><height>{h}</height><depth>3</depth></size>
<object><name>dog</name><bndbox><xmin>4</xmin><ymin>2</ymin><xmax>20</xmax><ymax>30</ymax></bndbox>
  <part><name>head</name><bndbox><xmin>1</xmin><ymin>1</ymin><xmax>2</xmax><ymax>2</ymax></bndbox></part></object>
<group><object><name>tvmonitor</name><pose>Left</pose><bndbox><xmin>5.5</xmin><ymin>6</ymin><xmax>7</xmax><ymax>8</ymax></bndbox></object></group>
</annotation>"""


def _voc_dir(tmp_path, n):
    xml_dir, img_dir = tmp_path / 'Annotations', tmp_path / 'JPEGImages'
    xml_dir.mkdir(), img_dir.mkdir()
    for k in range(n):
        name = JC.DECODABLE[k % len(JC.DECODABLE)]
        e = JC.MANIFEST[name]
        (img_dir / f'{k:06d}.jpg').write_bytes(JC.fixture_bytes(name))
        (xml_dir / f'{k:06d}.xml').write_text(XML.format(name=f'{k:06d}', w=e['width'], h=e['height']))
    return str(xml_dir), str(img_dir)


def test_xml_to_example_takes_objects_at_any_depth(tmp_path):
    vd = _vd()
    xml_dir, img_dir = _voc_dir(tmp_path, 1)
    ex = vd.parse_example(vd.xml_to_example(os.path.join(xml_dir, '000000.xml'), img_dir))
    e = JC.MANIFEST[JC.DECODABLE[0]]
    assert ex['image'] == JC.fixture_bytes(JC.DECODABLE[0]) and ex['shape'].tolist() == [e['height'], e['width'], 3]
    assert ex['ground_truth'].tolist() == [[2, 30, 4, 20, 11], [6, 8, 5.5, 7, 19]]          # the `part` is not an object; the nested object is


def test_dataset2tfrecord_writes_all_7_annotations_into_3_shards(tmp_path):
    vd = _vd()
    xml_dir, img_dir = _voc_dir(tmp_path, 7)
    files = vd.dataset2tfrecord(xml_dir, img_dir, str(tmp_path / 'out'), 'voc', total_shards=3)
    assert [os.path.basename(f) for f in files] == ['voc_%05d-of-00003.tfrecord' % k for k in (1, 2, 3)]
    counts = [len(list(vd.tf_record_iterator(f))) for f in files]
    assert sum(counts) == 7 and counts == [3, 3, 1]
    images = [vd.parse_example(r)['image'] for f in files for r in vd.tf_record_iterator(f)]
    assert images == [JC.fixture_bytes(JC.DECODABLE[k % len(JC.DECODABLE)]) for k in range(7)]


# ---------------------------------------------------------------- generator (host logic; decode and augmentor mocked)
class MockDecoder:
    """entropy(): the worker's half -- remembers the thread it ran on; 'BAD' payloads are refused like an unsupported JPEG"""

    def __init__(self):
        self.entropy_threads, self.reconstruct_threads = set(), set()

    def entropy(self, datas):
        vd = _vd()
        self.entropy_threads.add(threading.get_ident())
        for i, d in enumerate(datas):
            if d.startswith(b'BAD'):
                raise vd.JpegError(f'picture {i}: jpeg: progressive JPEG (SOF2) is not supported')
        return [int(d) for d in datas]

    def reconstruct(self, hb):
        self.reconstruct_threads.add(threading.get_ident())
        return hb


def _mock_augmentor(images, gts):
    return list(images), [float(g[0, 4]) for g in gts]


def _shards(tmp_path, n, bad=()):
    vd = _vd()
    paths = []
    for s in range(2):
        paths.append(str(tmp_path / f's{s}.tfrecord'))
        with vd.TFRecordWriter(paths[-1]) as w:
            for k in range(s * (n // 2), n if s else n // 2):
                image = b'BAD' if k in bad else str(k).encode()
                w.write(vd.encode_example(image, [1, 1, 3], [[0, 1, 0, 1, k % 20]]))
    return paths


def _restated_shuffle(n, buffer_size, rng):
    """the rule in ten lines: a buffer filled from the input; each output is a uniformly drawn slot, refilled from the input, or with the last slot once
    the input has ended"""
    buf, nxt, out = list(range(min(buffer_size, n))), min(buffer_size, n), []
    while buf:
        i = int(rng.integers(len(buf)))
        out.append(buf[i])
        if nxt < n:
            buf[i] = nxt
            nxt += 1
        else:
            buf[i] = buf[-1]
            buf.pop()
    return out


def test_generator_order_remainder_repeat_restart_and_threads(tmp_path):
    vd = _vd()
    n, B, buf = 11, 4, 5
    dec = MockDecoder()
    gen = vd.get_generator(_shards(tmp_path, n), B, buf, {}, seed=42, prefetch=2, decoder=dec, augmentor=_mock_augmentor)
    rng = np.random.default_rng(42)
    want = []
    for _ in range(3):                                       # three passes: each drops its remainder of 11 % 4 = 3 and reshuffles with the running generator
        order = _restated_shuffle(n, buf, rng)
        want += [order[i: i + B] for i in range(0, n - n % B, B)]
    it = iter(gen)
    got = [next(it) for _ in range(6)]
    assert [g[0] for g in got] == want[:6]
    assert all(g[1] == [float(k % 20) for k in g[0]] for g in got)
    it2 = iter(gen)                                          # restart: the same stream from its beginning; the first iterator is ended
    assert [next(it2)[0] for _ in range(2)] == want[:2]
    assert not it._thread.is_alive()
    with pytest.raises(StopIteration):
        next(it)
    worker = it2._thread
    it2.close()
    assert not worker.is_alive()
    assert threading.get_ident() not in dec.entropy_threads and dec.reconstruct_threads == {threading.get_ident()}


def test_generator_bad_record_raises_in_the_consumer(tmp_path):
    vd = _vd()
    gen = vd.get_generator(_shards(tmp_path, 8, bad={5}), 2, 1, {}, seed=0, decoder=MockDecoder(), augmentor=_mock_augmentor)
    it = iter(gen)
    assert [next(it)[0] for _ in range(2)] == [[0, 1], [2, 3]]
    got = []

    def consume():                                           # on a helper thread: a consumer that hung would fail the join below, not hang the test
        try:
            got.append(next(it))
        except BaseException as e:                           # noqa: BLE001
            got.append(e)
    t = threading.Thread(target=consume, daemon=True)
    t.start()
    t.join(5.0)
    assert not t.is_alive(), 'next() did not return within 5 s of the bad record'
    assert isinstance(got[0], vd.JpegError) and re.search(r'record 5: jpeg: progressive JPEG \(SOF2\) is not supported', str(got[0]))
    it._thread.join(5.0)
    assert not it._thread.is_alive()


def test_generator_worker_ends_when_the_iterator_is_dropped(tmp_path):
    vd = _vd()
    gen = vd.get_generator(_shards(tmp_path, 8), 2, 4, {}, seed=0, prefetch=1, decoder=MockDecoder(), augmentor=_mock_augmentor)
    it = iter(gen)
    next(it)
    worker = it._thread
    assert worker.daemon and worker.is_alive()
    del it
    worker.join(5.0)
    assert not worker.is_alive()
    small = vd.get_generator(_shards(tmp_path, 2), 4, 4, {}, decoder=MockDecoder(), augmentor=_mock_augmentor)
    with pytest.raises(ValueError, match='fewer than batch_size'):
        next(iter(small))


def test_generator_with_real_decode_under_the_emulation(tmp_path):
    """shards of fixture pictures through the real worker, entropy decoder and (emulated) kernels into the augmentor: shapes, and pixels against PIL"""
    vd = _vd()
    paths, records = JC.write_fixture_shards(tmp_path)
    cfg = {'data_format': 'channels_last', 'output_shape': [16, 16], 'fill_mode': 'BILINEAR', 'keep_aspect_ratios': False, 'constant_values': 0., 'pad_truth_to': 6}
    seen = {}

    def augmentor(images, gts):
        seen['images'], seen['gts'] = images, gts
        return len(images), len(gts)
    with JC.emulated():
        it = iter(vd.get_generator(paths, 4, 1, cfg, device='cpu', seed=0, decoder=vd.JpegBatchDecoder('cpu', threads=2), augmentor=augmentor))
        assert next(it) == (4, 4)
        it.close()
    for (name, boxes), img, gt in zip(records[:4], seen['images'], seen['gts']):
        d = np.abs(img.numpy().astype(np.int32) - JC.fixture_rgb(name).astype(np.int32))
        assert d.max() <= JC.max_bound(name) and np.array_equal(gt.numpy(), boxes)


def test_sizes_declared_by_the_stream_are_bounded_before_they_are_allocated(tmp_path):
    vd = _vd()
    p = str(tmp_path / 'huge.tfrecord')
    with vd.TFRecordWriter(p) as w:
        w.write(b'payload')
    raw = bytearray(open(p, 'rb').read())
    raw[:8] = struct.pack('<Q', (1 << 40) - 1)               # a length of a terabyte in a file of 23 bytes
    open(p, 'wb').write(raw)
    with pytest.raises(vd.TFRecordError, match='truncated record at byte offset 0 '):
        list(vd.tf_record_iterator(p, verify=False))
    data = bytearray(JC.fixture_bytes('s420_8x8'))
    sof = data.index(b'\xff\xc0')
    data[sof + 5: sof + 9] = b'\xff\xff\xff\xff'            # the frame header declares 65535 x 65535
    dec = vd.JpegBatchDecoder('cpu', threads=1)
    with pytest.raises(vd.JpegError, match='picture 0: jpeg: 65535 x 65535 pixels exceed max_pixels'):
        dec.entropy([bytes(data)])
    with pytest.raises(vd.JpegError, match='exceed max_pixels = 63'):
        vd.JpegBatchDecoder('cpu', threads=1, max_pixels=63).entropy([JC.fixture_bytes('s420_8x8')])


def test_evaluate_refuses_an_endless_generator_without_a_count(tmp_path):
    import odtk
    vd = _vd()
    gen = vd.get_generator(_shards(tmp_path, 8), 2, 1, {}, decoder=MockDecoder(), augmentor=_mock_augmentor)

    class Model:
        config = {'num_classes': 20}
    with pytest.raises(ValueError, match='repeats without end'):
        odtk.evaluate(Model(), gen)
