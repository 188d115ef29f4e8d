"""odtk.imagenet_data without a GPU: the record layout, hostile records, dataset2tfrecord over a tree of class folders filled from tests/golden/jpeg, the
generator's host logic with the two device stages replaced through the decoder= / augmentor= hooks (as tests/test_cpu_voc_data.py does), and the host logic
of RetinaNet.evaluate() / test_images() in pre-training mode over mocked launches (tests/mock_ops.py plus the stand-ins here)."""
import contextlib
import json
import os
import shutil
import sys
import threading
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_cases as JC                  # noqa: E402


def _im():
    import odtk  # noqa: F401
    from odtk import imagenet_data
    return imagenet_data


def _pb():
    from odtk.tf_checkpoint import _pb_bytes, _pb_field, _put_varint
    return _pb_bytes, _pb_field, _put_varint


# ---------------------------------------------------------------- records
def test_example_round_trip_and_layout():
    im = _im()
    _pb_bytes, _pb_field, _put_varint = _pb()
    image = bytes(range(256)) * 3
    rec = im.encode_example(image, [375, 500, 3], 217)
    ex = im.parse_example(rec)
    assert ex['image'] == image and ex['shape'].dtype == np.int32 and ex['shape'].tolist() == [375, 500, 3] and ex['label'] == 217 and type(ex['label']) is int
    assert im.encode_example(ex['image'], ex['shape'], ex['label']) == rec                      # byte for byte
    # the reference's layout, spelled out: image / shape bytes_list (Feature field 1), label int64_list (field 3) holding one packed varint
    def entry(key, feature):
        return _pb_bytes(1, _pb_bytes(1, key) + _pb_bytes(2, feature))
    want = _pb_bytes(1, entry(b'image', _pb_bytes(1, _pb_bytes(1, image))) + entry(b'shape', _pb_bytes(1, _pb_bytes(1, np.asarray([375, 500, 3], np.int32).tobytes())))
                     + entry(b'label', _pb_bytes(3, _pb_bytes(1, _put_varint(217)))))
    assert rec == want
    # map entries in any order, unknown features ignored, an unpacked int64 accepted
    other = _pb_bytes(1, entry(b'label', _pb_bytes(3, _pb_field(1, 0, _put_varint(5)))) + entry(b'extra', _pb_bytes(1, _pb_bytes(1, b'x')))
                      + entry(b'shape', _pb_bytes(1, _pb_bytes(1, b'\0' * 12))) + entry(b'image', _pb_bytes(1, _pb_bytes(1, b'jpg'))))
    assert im.parse_example(other)['label'] == 5 and im.parse_example(other)['image'] == b'jpg'
    assert im.parse_example(im.encode_example(b'', [1, 1, 3], 2 ** 40))['label'] == 2 ** 40   # the generator carries any non-negative label


def test_hostile_records_are_refused_by_name():
    im = _im()
    _pb_bytes, _pb_field, _put_varint = _pb()

    def entry(key, feature):
        return _pb_bytes(1, _pb_bytes(1, key) + _pb_bytes(2, feature))
    img = entry(b'image', _pb_bytes(1, _pb_bytes(1, b'jpg')))
    shp = entry(b'shape', _pb_bytes(1, _pb_bytes(1, b'\0' * 12)))
    lab = entry(b'label', _pb_bytes(3, _pb_bytes(1, _put_varint(3))))
    ex = lambda *e: _pb_bytes(1, b''.join(e))                   # noqa: E731
    assert im.parse_example(ex(img, shp, lab))['label'] == 3
    for rec, msg in ((ex(img, shp), r"without the feature\(s\) \['label'\]"),
                     (ex(shp, lab), r"without the feature\(s\) \['image'\]"),
                     (ex(img, entry(b'shape', _pb_bytes(1, _pb_bytes(1, b'\0' * 8))), lab), 'shape of 8 bytes'),
                     (ex(img, shp, entry(b'label', _pb_bytes(3, _pb_bytes(1, _put_varint(3) + _put_varint(4))))), 'label list of 2 values'),
                     (ex(img, shp, entry(b'label', _pb_bytes(3, b''))), 'label list of 0 values'),
                     (ex(img, shp, entry(b'label', _pb_bytes(3, _pb_bytes(1, _put_varint(-1))))), 'negative label -1'),
                     (ex(img, shp, entry(b'label', _pb_bytes(1, _pb_bytes(1, b'3')))), "'label' is not an int64_list"),
                     (ex(entry(b'image', _pb_bytes(3, _pb_bytes(1, _put_varint(1)))), shp, lab), "'image' is not a bytes_list"),
                     (ex(img, shp, entry(b'label', _pb_bytes(3, _pb_field(1, 1, b'\3' + b'\0' * 7)))), 'wire type 1'),
                     (ex(img, shp, entry(b'label', _pb_field(3, 0, _put_varint(3)))), "'label' is not an int64_list"),
                     (ex(img, shp, entry(b'label', _pb_bytes(3, _pb_bytes(1, b'\x80')))), 'malformed protobuf')):
        with pytest.raises(ValueError, match=msg):
            im.parse_example(rec)
    # voc_data keeps its own messages
    from odtk import voc_data
    with pytest.raises(ValueError, match=r"without the bytes_list feature\(s\) \['ground_truth'\]"):
        voc_data.parse_example(ex(img, shp, lab))


# ---------------------------------------------------------------- dataset2tfrecord
def _tree(root, names, per_class=1):
    """class folders n00 .. : folder k holds `per_class` copies of fixture names[k] (one DISTINCT picture per class)"""
    for k, name in enumerate(names):
        d = os.path.join(root, f'n{k:02d}')
        os.makedirs(d)
        for j in range(per_class):
            shutil.copy(os.path.join(JC.GOLDEN, name + '.jpg'), os.path.join(d, f'{name}_{j}.jpg'))
    return root


def _read(files):
    from odtk import voc_data
    im = _im()
    return [im.parse_example(r) for f in files for r in voc_data.tf_record_iterator(f)]


def test_dataset2tfrecord_writes_every_picture_once(tmp_path):
    im = _im()
    names = JC.DECODABLE
    root = _tree(str(tmp_path / 'img'), names, per_class=2)
    open(os.path.join(root, 'README'), 'w').write('not a class folder')
    files = im.dataset2tfrecord(root, str(tmp_path / 'out'), 'train', total_shards=5, seed=4)
    assert [os.path.basename(f) for f in files] == ['train_%05d-of-00005.tfrecord' % k for k in range(1, 6)]
    got = _read(files)
    assert len(got) == 2 * len(names)                            # every picture (the reference's arithmetic would drop 2 * len(names) % 5 ... of them)
    count = {}
    for e in got:
        name = names[e['label']]                                 # default mapping: sorted folder names -> 0 .. K-1
        assert e['image'] == JC.fixture_bytes(name)
        m = JC.MANIFEST[name]
        assert e['shape'].tolist() == [m['height'], m['width'], 3]
        count[name] = count.get(name, 0) + 1
    assert count == {n: 2 for n in names}
    again = _read(im.dataset2tfrecord(root, str(tmp_path / 'out2'), 'train', total_shards=5, seed=4))
    assert [e['label'] for e in again] == [e['label'] for e in got]                      # the seed fixes the shuffle ...
    other = _read(im.dataset2tfrecord(root, str(tmp_path / 'out3'), 'train', total_shards=3, seed=5))
    assert [e['label'] for e in other] != [e['label'] for e in got] and sorted(e['label'] for e in other) == sorted(e['label'] for e in got)
    assert [e['label'] for e in got] != sorted(e['label'] for e in got)                  # ... and it IS shuffled


def test_dataset2tfrecord_mappings(tmp_path):
    im = _im()
    names = JC.DECODABLE[:3]
    root = _tree(str(tmp_path / 'img'), names)
    mapping = {'n00': 7, 'n01': 223, 'n02': 0, 'unused': 1}
    got = _read(im.dataset2tfrecord(root, str(tmp_path / 'a'), 'x', total_shards=2, classname_to_ids=mapping, seed=0))
    assert sorted((e['label'], e['image']) for e in got) == sorted((mapping[f'n{k:02d}'], JC.fixture_bytes(n)) for k, n in enumerate(names))
    path = str(tmp_path / 'map.json')
    json.dump(mapping, open(path, 'w'))
    from_json = _read(im.dataset2tfrecord(root, str(tmp_path / 'b'), 'x', total_shards=2, classname_to_ids=path, seed=0))
    assert [(e['label'], e['image']) for e in from_json] == [(e['label'], e['image']) for e in got]
    with pytest.raises(ValueError, match=r"no entry for the class folder\(s\) \['n02'\]"):
        im.dataset2tfrecord(root, str(tmp_path / 'c'), 'x', classname_to_ids={'n00': 0, 'n01': 1})
    with pytest.raises(ValueError, match='non-negative integer'):
        im.dataset2tfrecord(root, str(tmp_path / 'd'), 'x', classname_to_ids={'n00': 0, 'n01': -1, 'n02': 2})


def test_dataset2tfrecord_unsupported_files(tmp_path):
    im = _im()
    from odtk.voc_data import JpegError
    names = JC.DECODABLE[:4] + JC.REFUSED
    root = _tree(str(tmp_path / 'img'), names)
    progressive = [n for n in JC.REFUSED if 'prog' in n][0]
    only = _tree(str(tmp_path / 'one'), JC.DECODABLE[:2] + [progressive])
    with pytest.raises(JpegError, match=progressive + r'_0\.jpg: jpeg: .*progressive'):
        im.dataset2tfrecord(only, str(tmp_path / 'r'), 'x', total_shards=1)
    with pytest.raises(ValueError, match='on_unsupported'):
        im.dataset2tfrecord(root, str(tmp_path / 'r2'), 'x', on_unsupported='ignore')
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        files = im.dataset2tfrecord(root, str(tmp_path / 's'), 'x', total_shards=3, seed=1, on_unsupported='skip')
    mine = [x for x in w if 'does not support' in str(x.message)]
    assert len(mine) == 1 and f'{len(JC.REFUSED)} file(s)' in str(mine[0].message) and '.jpg' in str(mine[0].message)
    got = _read(files)
    assert sorted(names[e['label']] for e in got) == sorted(JC.DECODABLE[:4])              # exactly the manifest's refused files are left out


# ---------------------------------------------------------------- generator (host logic; decode and augmentor mocked)
class MockDecoder:
    """entropy(): the worker's half, remembers its thread and hands the JPEG bytes on as the 'decoded picture'"""

    def __init__(self):
        self.entropy_threads, self.reconstruct_threads = set(), set()

    def entropy(self, datas):
        self.entropy_threads.add(threading.get_ident())
        return list(datas)

    def reconstruct(self, hb):
        self.reconstruct_threads.add(threading.get_ident())
        return hb


def _mock_augmentor(images, gts):
    assert gts is None                                           # the ImageNet records carry no ground truth
    return list(images)


def _shard(path, names, labels=None):
    """one record per entry of names, label = its index in JC.MANIFEST's sorted names unless given"""
    from odtk import voc_data
    im = _im()
    order = sorted(JC.MANIFEST)
    with voc_data.TFRecordWriter(str(path)) as w:
        for k, n in enumerate(names):
            m = JC.MANIFEST[n]
            w.write(im.encode_example(JC.fixture_bytes(n), [m['height'], m['width'], 3], order.index(n) if labels is None else labels[k]))
    return str(path), order


def _restated_shuffle(n, buf, rng):
    from odtk.voc_data import shuffle_stream
    return list(shuffle_stream(range(n), buf, rng))


def test_generator_order_pairing_remainder_restart_and_threads(tmp_path):
    im = _im()
    names = [JC.DECODABLE[k % len(JC.DECODABLE)] for k in range(11)]
    a, order = _shard(tmp_path / 'a.tfrecord', names[:6])
    b, _ = _shard(tmp_path / 'b.tfrecord', names[6:])
    B, buf = 4, 5
    dec = MockDecoder()
    gen = im.get_generator([a, b], B, buf, {}, seed=42, decoder=dec, augmentor=_mock_augmentor)
    assert gen.endless is True and gen.skipped == 0
    rng = np.random.default_rng(42)
    want = []
    for _ in range(3):                                           # three passes: each drops its remainder of 11 % 4 = 3 and reshuffles with the running generator
        o = _restated_shuffle(11, buf, rng)
        want += [o[i: i + B] for i in range(0, 8, B)]
    it = iter(gen)
    assert it._thread.name == 'odtk-imagenet-loader' and it._thread.daemon
    for k in range(6):
        images, labels = next(it)
        assert isinstance(labels, torch.Tensor) and labels.dtype == torch.int64 and labels.device.type == 'cpu' and tuple(labels.shape) == (B,)
        assert labels.tolist() == [order.index(names[i]) for i in want[k]]
        for img, lab in zip(images, labels.tolist()):            # the label stays with its picture through the shuffle
            assert img == JC.fixture_bytes(order[lab])
    first = iter(im.get_generator([a, b], B, buf, {}, seed=42, decoder=MockDecoder(), augmentor=_mock_augmentor))
    assert next(first)[1].tolist() == [order.index(names[i]) for i in want[0]]             # the same seed, the same order
    first.close()
    worker = it._thread
    it2 = iter(gen)                                              # a new iter() ends the previous stream
    worker.join(5.0)
    assert not worker.is_alive()
    with pytest.raises(StopIteration):
        next(it)
    assert next(it2)[1].tolist() == [order.index(names[i]) for i in want[0]]
    it2.close()
    assert not it2._thread.is_alive()
    assert threading.get_ident() not in dec.entropy_threads and dec.reconstruct_threads == {threading.get_ident()}


def test_generator_fewer_records_than_a_batch_and_config_check(tmp_path):
    im = _im()
    a, _ = _shard(tmp_path / 'a.tfrecord', JC.DECODABLE[:2])
    with pytest.raises(ValueError, match='fewer than batch_size'):
        next(iter(im.get_generator(a, 4, 4, {}, decoder=MockDecoder(), augmentor=_mock_augmentor)))
    with pytest.raises(ValueError, match='pad_truth_to'):
        im.get_generator(a, 2, 4, {'data_format': 'channels_last', 'output_shape': [8, 8], 'pad_truth_to': 60}, device='cpu', decoder=MockDecoder())
    with pytest.raises(ValueError, match='on_unsupported'):
        im.get_generator(a, 2, 4, {}, on_unsupported='drop', decoder=MockDecoder(), augmentor=_mock_augmentor)


def test_generator_skip_fills_batches_and_raise_names_the_record(tmp_path):
    im = _im()
    from odtk import voc_data
    good = JC.DECODABLE[:8]
    names = good[:2] + [JC.REFUSED[0]] + good[2:4] + [JC.REFUSED[-1]] + good[4:]             # refused at records 2 and 5
    a, order = _shard(tmp_path / 'a.tfrecord', names)
    gen = im.get_generator(a, 2, 1, {}, seed=0, on_unsupported='skip', decoder=MockDecoder(), augmentor=_mock_augmentor)
    it = iter(gen)
    got = [next(it)[1].tolist() for _ in range(4)]                # buffer_size 1 keeps file order: the batches are filled from the following records
    it.close()
    assert got == [[order.index(n) for n in good[i: i + 2]] for i in range(0, 8, 2)]
    assert gen.skipped >= 2 and gen.skipped % 2 == 0             # (the worker runs ahead into the next pass)
    real = voc_data.JpegBatchDecoder('cpu', threads=1)

    class RealEntropy(MockDecoder):                               # the worker's half is the real Huffman decoder (host code); no device half
        def entropy(self, datas):
            real.entropy(datas)
            return list(datas)
    strict = im.get_generator(a, 2, 1, {}, seed=0, decoder=RealEntropy(), augmentor=_mock_augmentor)
    with pytest.raises(voc_data.JpegError, match=r'^record 2: jpeg: '):
        it = iter(strict)
        next(it)
        next(it)


# ---------------------------------------------------------------- RetinaNet.evaluate / test_images in pre-training mode, launches mocked
def _classify_eval(logits, ldl, N, C_, labels, top_k, rank, loss, totals, loss_sum, class_seen, class_hit):
    import classify_cases as CC
    r = CC.reference(logits.numpy()[:, :C_], C_, labels.numpy(), top_k)
    rank.copy_(torch.from_numpy(r['rank']).to(rank.dtype))
    loss.copy_(torch.from_numpy(r['loss']).float())
    totals += torch.from_numpy(r['totals'])
    loss_sum += float(np.nansum(np.where(r['counted'], r['loss'], 0.0)))
    class_seen += torch.from_numpy(r['seen']).to(class_seen.dtype)
    class_hit += torch.from_numpy(r['hit']).to(class_hit.dtype)


@contextlib.contextmanager
def mocked(forbidden):
    """mock_ops + the head stand-ins of test_cpu_retinanet_pretrain + odtk_classify_eval's; every name in `forbidden` raises when launched"""
    import mock_ops
    import test_cpu_retinanet_pretrain as TP
    from odtk import ops
    with mock_ops.installed():
        names = ['gap_softmax_ce_fwd', 'gap_softmax_ce_bwd', 'classify_eval'] + list(forbidden)
        old = {n: getattr(ops, n) for n in names}
        ops.gap_softmax_ce_fwd, ops.gap_softmax_ce_bwd, ops.classify_eval = TP._gap_fwd, TP._gap_bwd, _classify_eval

        def refuse(name):
            def f(*a, **k):
                raise AssertionError(f'{name} launched during evaluate()')
            return f
        for n in forbidden:
            setattr(ops, n, refuse(n))
        try:
            yield
        finally:
            for n, v in old.items():
                setattr(ops, n, v)


BACKWARD_AND_OPTIMIZER = ['gap_softmax_ce_bwd', 'conv2d_wgrad', 'conv2d_dgrad', 'bn_bwd', 'maxpool_bwd', 'sgd_momentum', 'sum_f32']


class Finite:
    def __init__(self, batches, endless=False):
        self.batches, self.endless, self.served = batches, endless, 0

    def __iter__(self):
        for b in self.batches:
            self.served += 1
            yield b


def test_pretraining_evaluate_host_logic():
    import odtk
    import test_cpu_retinanet_pretrain as TP
    torch.set_num_threads(8)
    g = torch.Generator().manual_seed(5)
    batches = [((torch.rand(2, 64, 64, 3, generator=g) * 255).round(), torch.tensor([3 + k, 200 - k])) for k in range(4)]
    cfg = TP._cfg(batch_size=2, data_shape=[64, 64, 3])
    with mocked(BACKWARD_AND_OPTIMIZER):
        val = Finite(batches)
        m = odtk.RetinaNet(cfg, {'num_train': 8, 'num_val': 7, 'train_generator': batches, 'val_generator': val})
        before = (m.P.clone(), m.Mom.clone(), m.S.clone(), m.global_step)
        r = m.evaluate()                                          # val_generator / num_val = 7 -> rounded down to 3 batches = 6 images
        assert r['num_images'] == 6 and val.served == 3 and r['top_k'] == 5 and r['invalid_labels'] == 0
        assert torch.equal(m.P, before[0]) and torch.equal(m.Mom, before[1]) and torch.equal(m.S, before[2]) and m.global_step == before[3]
        assert 0.0 <= r['top1'] <= r['topk'] <= 1.0 and np.isfinite(r['loss']) and int(r['class_seen'].sum()) == 6 and r['class_seen'][3] == 1
        assert m.evaluate(num_images=4, top_k=1)['num_images'] == 4
        assert m.evaluate(generator=Finite(batches))['num_images'] == 8                  # a finite generator without a count: one pass
        with pytest.raises(ValueError, match='less than one batch'):
            m.evaluate(num_images=1)
        with pytest.raises(ValueError, match='repeats without end'):
            m.evaluate(generator=Finite(batches, endless=True))
        assert m.evaluate(generator=Finite(batches, endless=True), num_images=5)['num_images'] == 4
        short = batches[:1] + [(batches[1][0][:1], batches[1][1][:1])]
        with pytest.raises(ValueError, match='a batch of 1 images'):
            m.evaluate(generator=Finite(short))
        with pytest.raises(ValueError, match='labels'):
            m.evaluate(generator=Finite([(batches[0][0], torch.tensor([3, 224]))]))
        none = odtk.RetinaNet(cfg, {'num_train': 8, 'num_val': 0, 'train_generator': batches, 'val_generator': None})
        with pytest.raises(ValueError, match='no generator given'):
            none.evaluate()
        with pytest.raises(ValueError, match='moving statistics'):
            odtk.RetinaNet(dict(cfg, mode='test'), None).evaluate(generator=Finite(batches))
    with mocked([]):                                              # the step itself does launch them: the list above is not vacuous
        m = odtk.RetinaNet(cfg, {'num_train': 8, 'num_val': 0, 'train_generator': batches, 'val_generator': None})
        m.set_batch(*batches[0])
        with mocked(['sgd_momentum']), pytest.raises(AssertionError, match='sgd_momentum launched'):
            m.train_step(0.01)


def test_pretraining_test_images_host_logic():
    import odtk
    import test_cpu_retinanet_pretrain as TP
    torch.set_num_threads(8)
    g = torch.Generator().manual_seed(6)
    imgs = (torch.rand(3, 64, 64, 3, generator=g) * 255).round()
    with mocked([]):
        m = odtk.RetinaNet(TP._cfg(mode='test', data_shape=[64, 64, 3], test_batch_size=3), None)
        assert m.batch_size == 3
        full = m.test_images(imgs.numpy())
        assert full.dtype == np.int64 and full.shape == (3,)
        part = m.test_images(imgs[1:].numpy())                    # n < test_batch_size: the tail slot is computed and discarded
        assert part.shape == (2,) and np.array_equal(part, full[1:])
        one = m.test_one_image(imgs[2:].numpy())
        assert one.dtype == np.int64 and one.shape == (1,) and one[0] == full[2]
        for bad in (torch.zeros(4, 64, 64, 3).numpy(), imgs[:0].numpy(), imgs[:, :63].numpy()):
            with pytest.raises(ValueError, match='test_images'):
                m.test_images(bad)
        single = odtk.RetinaNet(TP._cfg(mode='test', data_shape=[64, 64, 3]), None)
        single.load_oracle_params(m.export_params())
        assert np.array_equal(np.concatenate([single.test_one_image(imgs[k: k + 1].numpy()) for k in range(3)]), full)
