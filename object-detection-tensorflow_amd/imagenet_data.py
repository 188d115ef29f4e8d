"""ImageNet-style classification input: the reference's `utils/tfrecord_imagenet_utils.py` behind the same names, without TensorFlow.  The provider of
(images, labels) for RetinaNet's classification pre-training graph (`is_pretraining: True`); the twin of voc_data.py, whose framing, JPEG decoder, shuffle
buffer and loader thread it uses.

    encode_example / parse_example   the reference's tf.train.Example (tfrecord_imagenet_utils.py:87-91): `image` bytes_list (the JPEG file), `shape`
                                     bytes_list holding int32[3] h, w, 3, `label` int64_list with one value
    dataset2tfrecord                 a directory with one sub-directory per class -> `.tfrecord` shards
    get_generator                    shards -> shuffle buffer -> batches -> decode -> odtk.augment.Augmentor without ground truth:
                                     (images f32 [B, H, W, 3] on the device, labels int64 [B] on the host), what RetinaNet.set_batch takes in pre-training mode

Where this differs from the reference, on purpose:
  - dataset2tfrecord writes EVERY picture (the reference's `int(ceil(n)) / shards` rounds down and drops up to total_shards - 1 of them), takes the class
    ids from a mapping the caller gives (default: the sorted directory names -> 0 .. K-1; the reference's 1000-entry table is not restated) and reads
    `shape` from the JPEG header (odtk_jpeg_info) instead of decoding every file.
  - Baseline JPEG only, as in voc_data.py.  ImageNet holds a few progressive and CMYK files: on_unsupported='skip' leaves them out, in dataset2tfrecord
    (with one warning) and in get_generator (counted in generator.skipped); 'raise' (default) names the file / record.
  - get_generator returns ONE re-iterable object, as voc_data.get_generator does."""
from __future__ import annotations

import ctypes as C
import json
import os
import warnings

import numpy as np
import torch

from . import _lib
from ._lib import JpegInfo
from .tf_checkpoint import _get_varint, _pb_bytes, _pb_parse, _put_varint, _signed
from .voc_data import JpegError, TFRecordWriter, VOCGenerator, _example_features

FEATURES = ('image', 'shape', 'label')


# --------------------------------------------------------------------------------------------------- tf.train.Example
def encode_example(image_bytes: bytes, shape, label: int) -> bytes:
    """Feature{bytes_list = 1 -> BytesList{value = 1}} for image and shape, Feature{int64_list = 3 -> Int64List{value = 1, packed}} for the label"""
    shape = np.asarray(shape, np.int32).reshape(3)

    def entry(key, feature):
        return _pb_bytes(1, _pb_bytes(1, key.encode()) + _pb_bytes(2, feature))
    entries = [entry('image', _pb_bytes(1, _pb_bytes(1, bytes(image_bytes)))), entry('shape', _pb_bytes(1, _pb_bytes(1, shape.tobytes()))),
               entry('label', _pb_bytes(3, _pb_bytes(1, _put_varint(int(label)))))]
    return _pb_bytes(1, b''.join(entries))


def _bytes_value(key, feature):
    vals = None
    for f, wt, v in _pb_parse(feature):
        if f == 1 and wt == 2:
            inner = _pb_parse(v)
            if any(g == 1 and wb != 2 for g, wb, _ in inner):
                raise ValueError(f"feature '{key}': a bytes_list value with a wrong wire type")
            vals = (vals or []) + [b for g, wb, b in inner if g == 1]
        elif f in (1, 2, 3):
            raise ValueError(f"feature '{key}' is not a bytes_list (Feature field {f}, wire type {wt})")
    if vals is None:
        raise ValueError(f"feature '{key}' is not a bytes_list")
    if len(vals) != 1:
        raise ValueError(f"feature '{key}': a bytes_list of {len(vals)} values, not 1")
    return vals[0]


def _int64_values(key, feature):
    vals = None
    for f, wt, v in _pb_parse(feature):
        if f == 3 and wt == 2:
            vals = [] if vals is None else vals
            for g, wi, w in _pb_parse(v):
                if g != 1:
                    continue
                if wi == 0:                                       # not packed
                    vals.append(_signed(w))
                elif wi == 2:                                     # packed: varints back to back
                    pos = 0
                    while pos < len(w):
                        x, pos = _get_varint(w, pos)
                        vals.append(_signed(x))
                else:
                    raise ValueError(f"feature '{key}': an int64_list value of wire type {wi} (a varint is expected)")
        elif f in (1, 2, 3):
            raise ValueError(f"feature '{key}' is not an int64_list (Feature field {f}, wire type {wt})")
    if vals is None:
        raise ValueError(f"feature '{key}' is not an int64_list")
    return vals


def parse_example(record: bytes) -> dict:
    """{'image': bytes, 'shape': int32[3], 'label': int}; map entries in any order, unknown features ignored.  ValueError names what is wrong with a
    record: a missing feature, a feature of the wrong kind or wire type, a shape that is not 12 bytes, a label list that is not one non-negative value"""
    feats = {}
    try:
        for key, value in _example_features(record):
            if key in FEATURES and value is not None:
                feats[key] = _int64_values(key, value) if key == 'label' else _bytes_value(key, value)
    except ValueError:
        raise
    except Exception as e:                                        # noqa: BLE001 -- IndexError, struct.error: one exception type for hostile input
        raise ValueError(f'Example: truncated or malformed protobuf ({type(e).__name__})') from None
    missing = [k for k in FEATURES if k not in feats]
    if missing:
        raise ValueError(f'Example without the feature(s) {missing}')
    if len(feats['shape']) != 12:
        raise ValueError(f"Example with a shape of {len(feats['shape'])} bytes (int32[3] = 12 bytes)")
    if len(feats['label']) != 1:
        raise ValueError(f"Example with a label list of {len(feats['label'])} values, not 1")
    if feats['label'][0] < 0:
        raise ValueError(f"Example with the negative label {feats['label'][0]}")
    return {'image': feats['image'], 'shape': np.frombuffer(feats['shape'], np.int32).copy(), 'label': int(feats['label'][0])}


# --------------------------------------------------------------------------------------------------- conversion
def jpeg_refusal(data: bytes):
    """None if the decoder takes this JPEG, else its message (progressive, CMYK, RGB-coded, 12-bit, not a JPEG ...).  Host only: reads the headers."""
    lib = _lib.load()
    info = JpegInfo()
    if lib.odtk_jpeg_info(data, len(data), C.byref(info)) != 0:
        return lib.odtk_last_error().decode()
    return None


def _jpeg_shape(data: bytes):
    lib = _lib.load()
    info = JpegInfo()
    if lib.odtk_jpeg_info(data, len(data), C.byref(info)) != 0:
        return None, lib.odtk_last_error().decode()
    return np.asarray([info.height, info.width, 3], np.int32), None       # channels = 3: what the decoder returns, grayscale included


def _check_policy(on_unsupported):
    if on_unsupported not in ('raise', 'skip'):
        raise ValueError(f"on_unsupported must be 'raise' or 'skip', not {on_unsupported!r}")


def dataset2tfrecord(img_dir, output_dir, name, total_shards=50, classname_to_ids=None, seed=None, on_unsupported='raise'):
    """Converts a directory with one sub-directory per class into total_shards record files `<name>_<k>-of-<n>.tfrecord` (k from 1, both five digits: the
    reference's file names) under output_dir; returns the paths in shard order.  classname_to_ids: a dict, or the path of a JSON file holding one;
    default: the sorted sub-directory names -> 0 .. K-1.  A sub-directory the mapping does not name raises ValueError.  The list of files (sorted, then
    shuffled with `seed`) is written in consecutive runs of ceil(n / total_shards): EVERY picture, the last shards short or empty.  `shape` is h, w, 3
    from the JPEG header.  A file the decoder refuses: on_unsupported='raise' -> JpegError naming the path; 'skip' -> left out, one warning with the count
    and the first path."""
    _check_policy(on_unsupported)
    total_shards = int(total_shards)
    if total_shards < 1:
        raise ValueError(f'total_shards must be >= 1, not {total_shards}')
    classes = sorted(d for d in os.listdir(img_dir) if os.path.isdir(os.path.join(img_dir, d)))
    if classname_to_ids is None:
        mapping = {c: i for i, c in enumerate(classes)}
    elif isinstance(classname_to_ids, (str, os.PathLike)):
        with open(classname_to_ids) as f:
            mapping = json.load(f)
    else:
        mapping = dict(classname_to_ids)
    unknown = [c for c in classes if c not in mapping]
    if unknown:
        raise ValueError(f'dataset2tfrecord: classname_to_ids has no entry for the class folder(s) {unknown[:5]}')
    for c in classes:
        v = mapping[c]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f'dataset2tfrecord: class id of {c!r} must be a non-negative integer, not {v!r}')
    files = [(os.path.join(img_dir, c, f), int(mapping[c])) for c in classes for f in sorted(os.listdir(os.path.join(img_dir, c)))
             if os.path.isfile(os.path.join(img_dir, c, f))]
    np.random.default_rng(seed).shuffle(files)
    os.makedirs(output_dir, exist_ok=True)
    if os.listdir(output_dir):
        warnings.warn(f'dataset2tfrecord: {output_dir} already holds files; the shards are written next to them')
    run = -(-len(files) // total_shards)                               # runs of the FILE list: one pass, no picture kept in memory
    paths = [os.path.join(output_dir, '%s_%05d-of-%05d.tfrecord' % (name, k + 1, total_shards)) for k in range(total_shards)]
    refused = []
    for k, out in enumerate(paths):
        with TFRecordWriter(out) as writer:
            for path, label in files[k * run: (k + 1) * run]:
                with open(path, 'rb') as f:
                    data = f.read()
                shape, why = _jpeg_shape(data)
                if shape is None:
                    if on_unsupported == 'raise':
                        raise JpegError(f'{path}: {why}')
                    refused.append(path)
                    continue
                writer.write(encode_example(data, shape, label))
    if refused:
        warnings.warn(f'dataset2tfrecord: {len(refused)} file(s) the JPEG decoder does not support were left out (first: {refused[0]})')
    return paths


# --------------------------------------------------------------------------------------------------- the generator
def _label_payload(examples):
    return torch.tensor([e['label'] for e in examples], dtype=torch.int64)


class ImageNetGenerator(VOCGenerator):
    """see get_generator.  `skipped`: records left out so far by on_unsupported='skip' (all streams of this generator)"""
    THREAD_NAME = 'odtk-imagenet-loader'

    def __init__(self, tfrecords, batch_size, buffer_size, image_preprocess_config, device='cuda:0', seed=None, prefetch=2, verify=True,
                 on_unsupported='raise', decoder=None, augmentor=None):
        _check_policy(on_unsupported)
        if augmentor is None and image_preprocess_config.get('pad_truth_to') is not None:
            raise ValueError('image_preprocess_config: pad_truth_to belongs to ground truth; the ImageNet records have none')
        super().__init__(tfrecords, batch_size, buffer_size, image_preprocess_config, device, seed, prefetch, verify, decoder, augmentor)
        self.on_unsupported = on_unsupported
        self._skipped = [0]

    @property
    def skipped(self):
        return self._skipped[0]

    def _worker_options(self):
        return dict(parse=parse_example, extra=_label_payload, refusal=jpeg_refusal if self.on_unsupported == 'skip' else None, skipped=self._skipped)

    def _finish(self, images, labels):
        return self._augmentor(images, None), labels


def get_generator(tfrecords, batch_size, buffer_size, image_preprocess_config, device='cuda:0', seed=None, prefetch=2, verify=True,
                  on_unsupported='raise', **hooks):
    """tfrecord_imagenet_utils.get_generator: `.tfrecord` shards -> endless batches (images f32 [B, H, W, 3] on `device` (channels_first per the config),
    labels int64 [B], a CPU tensor): the (images, labels) RetinaNet.set_batch takes in pre-training mode.  image_preprocess_config is the reference's
    image_augmentor_config WITHOUT pad_truth_to.  Stages and threading are voc_data.get_generator's: records in file order -> shuffle buffer of
    buffer_size -> batches of batch_size, the remainder of a pass dropped -> repeated without end (`endless`); a daemon thread reads, parses and
    Huffman-decodes up to `prefetch` batches ahead, upload, reconstruction and augmentation run on the consumer's thread and current stream; each iter()
    restarts the stream and ends the previous one.  The label stays with its picture: both travel through the shuffle in one record.  A record whose JPEG
    the decoder refuses: on_unsupported='raise' -> JpegError('record <index>: jpeg: ...') from next(); 'skip' -> the record is dropped, the batch filled
    from the following records, and counted in `.skipped`.  The generator carries any non-negative label; set_batch checks it against the graph.
    hooks (tests): decoder=, augmentor= replace the two device stages (the augmentor is called as augmentor(images, None))."""
    return ImageNetGenerator(tfrecords, batch_size, buffer_size, image_preprocess_config, device, seed, prefetch, verify, on_unsupported, **hooks)
