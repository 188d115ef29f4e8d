"""PASCAL VOC input: the reference's `utils/tfrecord_voc_utils.py` behind the same names, without TensorFlow.

    dataset2tfrecord / xml_to_example   VOC annotations + JPEG files -> `.tfrecord` shards (the reference's tf.train.Example: three bytes_list features,
                                        `image` the JPEG file, `shape` int32[3] h, w, depth, `ground_truth` float32[G, 5] ymin, ymax, xmin, xmax, class)
    TFRecordWriter / tf_record_iterator the record framing (u64 length, masked CRC32C of it, payload, masked CRC32C of the payload)
    JpegBatchDecoder                    JPEG byte strings -> u8 [h, w, 3] device tensors: Huffman decoding on CPU threads (libodtk, the GIL released),
                                        everything per block and per pixel in one odtk_jpeg_reconstruct on the device (include/odtk.h, "JPEG")
    get_generator                       shards -> shuffle buffer -> batches -> decode -> odtk.augment.Augmentor: the object a model takes as
                                        data_provider['train_generator'] (or 'val_generator', with a config that has no random part)

Beyond the reference: the annotation's `<difficult>` (the PASCAL VOC protocol does not count such objects, voc_eval.py).  With with_difficult=True
dataset2tfrecord writes a fourth bytes_list feature `difficult` (uint8[G], next to `ground_truth`; readers that do not know it skip it) and
get_generator yields [B, pad, 6] ground truth whose last column is the flag of the box in that row.  Without it records and batches are the reference's.

Where this differs from the reference, on purpose:
  - dataset2tfrecord writes EVERY annotation.  The reference's shard size `int(ceil(len(xmllist)) / float(total_shards))` rounds down and silently drops
    up to total_shards - 1 annotations at the end of the list.
  - get_generator returns ONE re-iterable object instead of (init_op, iterator): every iter() restarts the stream, which is what running init_op did.
  - Baseline JPEG only (what VOC's JPEGImages are): progressive files, arithmetic coding, CMYK and 12-bit samples are refused with the record's index
    and the decoder's message.
The ImageNet records of tfrecord_imagenet_utils.py (one label per picture) are imagenet_data.py: it shares the framing, the decoder, the Example map
reader (_example_features) and the loader thread (_worker / _VOCIterator, given its own "parse" and "payload" functions: _worker's parse= / extra=) with this file.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
import queue
import struct
import threading
import warnings
import weakref
import xml.etree.ElementTree as ET
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from ._lib import JpegInfo, JpegPlan, OdtkError
from .tf_checkpoint import _pb_bytes, _pb_parse, crc32c, mask_crc

VOC_CLASSES = ('aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog', 'horse', 'motorbike',
               'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')
classname_to_ids = {name: i for i, name in enumerate(VOC_CLASSES)}


# --------------------------------------------------------------------------------------------------- TFRecord framing
class TFRecordError(ValueError):
    pass


class TFRecordWriter:
    def __init__(self, path):
        self.path = path
        self._f = open(path, 'wb')

    def write(self, record: bytes):
        head = struct.pack('<Q', len(record))
        self._f.write(head + struct.pack('<I', mask_crc(crc32c(head))) + record + struct.pack('<I', mask_crc(crc32c(record))))

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def tf_record_iterator(path, verify=True):
    """the payloads of one `.tfrecord` file in order; a short record or (verify=True) a bad CRC raises TFRecordError naming the record's byte offset"""
    with open(path, 'rb') as f:
        offset, size = 0, os.fstat(f.fileno()).st_size
        while True:
            head = f.read(12)
            if not head:
                return
            if len(head) < 12:
                raise TFRecordError(f'{path}: truncated record header at byte offset {offset} ({len(head)} of 12 bytes)')
            (length,), (lcrc,) = struct.unpack('<Q', head[:8]), struct.unpack('<I', head[8:])
            if verify and mask_crc(crc32c(head[:8])) != lcrc:
                raise TFRecordError(f'{path}: corrupt record at byte offset {offset} (length CRC mismatch)')
            left = max(size - offset - 12, 0)                # (the length is checked against the file before anything of that size is asked for)
            if length + 4 > left:
                raise TFRecordError(f'{path}: truncated record at byte offset {offset} (payload of {length} bytes + CRC, {left} bytes left)')
            body = f.read(length + 4)
            if len(body) < length + 4:
                raise TFRecordError(f'{path}: truncated record at byte offset {offset} (payload of {length} bytes + CRC, {len(body)} bytes read)')
            payload = body[:length]
            if verify and mask_crc(crc32c(payload)) != struct.unpack('<I', body[length:])[0]:
                raise TFRecordError(f'{path}: corrupt record at byte offset {offset} (payload CRC mismatch)')
            yield payload
            offset += 16 + length


# --------------------------------------------------------------------------------------------------- tf.train.Example
def _feature(key: str, value: bytes) -> bytes:
    """one entry of Features.feature (map<string, Feature>): key = 1, value = 2 -> Feature{bytes_list = 1 -> BytesList{value = 1}}"""
    return _pb_bytes(1, key.encode()) + _pb_bytes(2, _pb_bytes(1, _pb_bytes(1, value)))


def encode_example(image: bytes, shape, ground_truth, difficult=None) -> bytes:
    """the reference's Example (tfrecord_voc_utils.xml_to_example): Example{features = 1 -> Features{feature = 1 (repeated map entry)}}; difficult
    (uint8[G], one flag per ground-truth row) adds the feature `difficult` behind them"""
    shape = np.asarray(shape, np.int32).reshape(3)
    gt = np.asarray(ground_truth, np.float32).reshape(-1, 5)
    entries = [_feature('image', bytes(image)), _feature('shape', shape.tobytes()), _feature('ground_truth', gt.tobytes())]
    if difficult is not None:
        flags = np.asarray(difficult, np.uint8).reshape(-1)
        if flags.shape[0] != gt.shape[0]:
            raise ValueError(f'difficult holds {flags.shape[0]} flags for {gt.shape[0]} ground-truth rows')
        entries.append(_feature('difficult', flags.tobytes()))
    return _pb_bytes(1, b''.join(_pb_bytes(1, e) for e in entries))


def _example_features(record: bytes):
    """the (key, serialized Feature) entries of Example{features = 1 -> Features{feature = 1 (repeated map entry: key = 1, value = 2)}}, in record order;
    an entry without a value comes with None.  Shared with imagenet_data.py."""
    for f, wt, features in _pb_parse(record):
        if f != 1 or wt != 2:
            continue
        for f2, wt2, entry in _pb_parse(features):
            if f2 != 1 or wt2 != 2:
                continue
            key = value = None
            for f3, wt3, v in _pb_parse(entry):
                if f3 == 1 and wt3 == 2:
                    key = v.decode('utf-8', 'replace')
                elif f3 == 2 and wt3 == 2:
                    value = v
            yield key, value


def parse_example(record: bytes) -> dict:
    """{'image': bytes, 'shape': int32[3], 'ground_truth': float32[G, 5]} and, when the record has the feature, 'difficult': uint8[G]; map entries in any
    order, unknown features ignored"""
    feats = {}
    for key, value in _example_features(record):
        if key in ('image', 'shape', 'ground_truth', 'difficult') and value is not None:
            for f4, wt4, blist in _pb_parse(value):
                if f4 == 1 and wt4 == 2:                      # bytes_list
                    vals = [v for f5, wt5, v in _pb_parse(blist) if f5 == 1 and wt5 == 2]
                    if vals:
                        feats[key] = vals[0]
    missing = [k for k in ('image', 'shape', 'ground_truth') if k not in feats]
    if missing:
        raise ValueError(f'Example without the bytes_list feature(s) {missing}')
    if len(feats['shape']) != 12 or len(feats['ground_truth']) % 20:
        raise ValueError(f"Example with a shape of {len(feats['shape'])} bytes / ground truth of {len(feats['ground_truth'])} bytes (int32[3] / float32[G, 5])")
    out = {'image': feats['image'], 'shape': np.frombuffer(feats['shape'], np.int32).copy(),
           'ground_truth': np.frombuffer(feats['ground_truth'], np.float32).reshape(-1, 5).copy()}
    if 'difficult' in feats:
        if len(feats['difficult']) != out['ground_truth'].shape[0]:
            raise ValueError(f"Example with {len(feats['difficult'])} difficult flags for {out['ground_truth'].shape[0]} ground-truth rows")
        out['difficult'] = np.frombuffer(feats['difficult'], np.uint8).copy()
    return out


# --------------------------------------------------------------------------------------------------- VOC annotations
def xml_to_example(xmlpath, imgpath, with_difficult=False) -> bytes:
    """one VOC annotation + its JPEG file (read, not decoded) -> serialized Example.  Like the reference's xpath('//object') this takes EVERY `object`
    element of the document, at any depth; the box is the object's own `bndbox` child.  with_difficult: the object's `<difficult>` (absent or 0 -> 0,
    1 -> 1, anything else a ValueError naming the file) goes into the feature `difficult`."""
    root = ET.parse(xmlpath).getroot()
    with open(os.path.join(imgpath, root.find('filename').text), 'rb') as f:
        image = f.read()
    size = root.find('size')
    shape = [int(size.find(k).text) for k in ('height', 'width', 'depth')]
    rows, difficult = [], []
    for obj in root.iter('object'):
        box = obj.find('bndbox')
        rows.append([float(box.find(k).text) for k in ('ymin', 'ymax', 'xmin', 'xmax')] + [classname_to_ids[obj.find('name').text]])
        if with_difficult:
            tag = obj.find('difficult')
            text = '0' if tag is None else (tag.text or '').strip()
            if text not in ('0', '1'):
                raise ValueError(f'{xmlpath}: <difficult>{text}</difficult> of object {len(rows) - 1} is neither 0 nor 1')
            difficult.append(int(text))
    return encode_example(image, shape, np.asarray(rows, np.float32).reshape(-1, 5), np.asarray(difficult, np.uint8) if with_difficult else None)


def dataset2tfrecord(xml_dir, img_dir, output_dir, name, total_shards=5, with_difficult=False):
    """Converts a VOC directory: the `*.xml` annotations of xml_dir, in sorted order, with their pictures from img_dir, into total_shards record files
    `<name>_<k>-of-<n>.tfrecord` (k from 1, both five digits: the reference's file names) under output_dir; returns the paths in shard order.
    ALL annotations are written: consecutive runs of ceil(n / total_shards), so the last shards may be short or empty (the reference's arithmetic rounds
    down and drops up to total_shards - 1 annotations, see the module docstring).  Records are added to a directory that already holds files; a warning
    says so.  with_difficult: every record also carries the objects' `<difficult>` flags (xml_to_example); without it the records are the reference's."""
    total_shards = int(total_shards)
    if total_shards < 1:
        raise ValueError(f'total_shards must be >= 1, not {total_shards}')
    os.makedirs(output_dir, exist_ok=True)
    if os.listdir(output_dir):
        warnings.warn(f'dataset2tfrecord: {output_dir} already holds files; the shards are written next to them')
    annotations = sorted(glob.glob(os.path.join(xml_dir, '*.xml')))
    run = -(-len(annotations) // total_shards)
    paths = [os.path.join(output_dir, f'{name}_{k + 1:05d}-of-{total_shards:05d}.tfrecord') for k in range(total_shards)]
    for k, path in enumerate(paths):
        with TFRecordWriter(path) as writer:
            for annotation in annotations[k * run: (k + 1) * run]:
                writer.write(xml_to_example(annotation, img_dir, with_difficult))
    return paths


# --------------------------------------------------------------------------------------------------- JPEG
class JpegError(OdtkError):
    pass


def _align(n, a=16):
    return (n + a - 1) // a * a


class HostBatch:
    """what the CPU half leaves for the device half: per picture its info and offsets, one int16 coefficient array, one uint16 table array"""
    __slots__ = ('infos', 'coef_off', 'coef', 'qt', 'coef_elems')


class JpegBatchDecoder:
    """decoder(list of JPEG byte strings) -> list of u8 [h, w, 3] tensors on `device`.
    entropy() is the CPU half (no GPU call: safe on a worker thread), reconstruct() the device half on the current stream; __call__ runs both and lets
    the Huffman decoder write straight into the pinned staging buffer.  Staging and device buffers grow and never shrink.
    max_pixels bounds width * height of one picture as its header declares it (default 64 Mi, far above any VOC picture): buffers are sized from the
    header before a byte of entropy data is checked, and a hostile 65535 x 65535 frame header would otherwise ask for 13 GB."""

    def __init__(self, device='cuda:0', threads=None, max_pixels=1 << 26):
        self.device = torch.device(device)
        self.max_pixels = int(max_pixels)
        self.threads = int(threads) if threads else min(16, len(os.sched_getaffinity(0)))
        self._pool = ThreadPoolExecutor(self.threads, thread_name_prefix='odtk-jpeg')
        self._stage = self._dev_in = self._planes = None
        self._copied = None

    # ---- CPU half
    def _layout(self, datas):
        lib = _lib.load()
        infos, offs, total = [], [], 0
        for i, d in enumerate(datas):
            info = JpegInfo()
            if lib.odtk_jpeg_info(d, len(d), C.byref(info)) != 0:
                raise JpegError(f'picture {i}: {lib.odtk_last_error().decode()}')
            if info.width * info.height > self.max_pixels:
                raise JpegError(f'picture {i}: jpeg: {info.width} x {info.height} pixels exceed max_pixels = {self.max_pixels}')
            infos.append(info)
            offs.append(total)
            total += _align(int(info.coef_count), 8)            # in int16 elements: every picture starts 16-byte aligned
        return infos, offs, total

    def _decode_into(self, datas, infos, offs, coef_addr, qt_addr):
        lib = _lib.load()

        def one(i):
            rc = lib.odtk_jpeg_entropy_decode(datas[i], len(datas[i]), coef_addr + 2 * offs[i], int(infos[i].coef_count), qt_addr + 512 * i)
            return None if rc == 0 else lib.odtk_last_error().decode()          # (thread_local message: read on the thread that made the call)
        for i, msg in enumerate(self._pool.map(one, range(len(datas)))):
            if msg is not None:
                raise JpegError(f'picture {i}: {msg}')

    def entropy(self, datas) -> HostBatch:
        datas = [bytes(d) for d in datas]
        hb = HostBatch()
        hb.infos, hb.coef_off, hb.coef_elems = self._layout(datas)
        hb.coef = np.empty(max(hb.coef_elems, 1), np.int16)
        hb.qt = np.empty((len(datas), 4, 64), np.uint16)
        self._decode_into(datas, hb.infos, hb.coef_off, hb.coef.ctypes.data, hb.qt.ctypes.data)
        return hb

    # ---- device half
    def _sizes(self, infos, coef_elems):
        N = len(infos)
        qt_at = _align(2 * coef_elems)
        plan_at = _align(qt_at + 512 * N)
        return qt_at, plan_at, _align(plan_at + C.sizeof(JpegPlan) * N)

    def _grow(self, nbytes, plane_bytes):
        cuda = self.device.type == 'cuda'
        if self._stage is None or self._stage.numel() < nbytes:
            self._wait_copy()
            self._stage = torch.empty(nbytes, dtype=torch.uint8, pin_memory=cuda)
            self._dev_in = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if self._planes is None or self._planes.numel() < plane_bytes:
            self._planes = torch.empty(plane_bytes, dtype=torch.uint8, device=self.device)

    def _wait_copy(self):
        if self._copied is not None:
            self._copied.synchronize()           # the staging buffer is free again once the last upload has left it
            self._copied = None

    def _launch(self, infos, coef_off, coef_elems):
        """staging buffer filled with coefficients and tables -> plans, one upload, one odtk_jpeg_reconstruct"""
        from . import ops
        N = len(infos)
        qt_at, plan_at, nbytes = self._sizes(infos, coef_elems)
        out_off, out_bytes, plane_off, plane_bytes = [], 0, [], 0
        for info in infos:
            out_off.append(out_bytes)
            out_bytes += _align(info.height * info.width * 3)
            plane_off.append(plane_bytes)
            plane_bytes += _align(int(info.coef_count))
        out = torch.empty(out_bytes, dtype=torch.uint8, device=self.device)
        base, planes, outp = self._dev_in.data_ptr(), self._planes.data_ptr(), out.data_ptr()
        plans = (JpegPlan * N)()
        units = tiles = 0
        for i, info in enumerate(infos):
            ops.jpeg_plan_init(plans[i], info, base + 2 * coef_off[i], base + qt_at + 512 * i, planes + plane_off[i], outp + out_off[i], units, tiles)
            units += plans[i].unit_count
            tiles += plans[i].tile_count
        C.memmove(self._stage.data_ptr() + plan_at, C.addressof(plans), C.sizeof(plans))
        self._dev_in[:nbytes].copy_(self._stage[:nbytes], non_blocking=True)
        if self.device.type == 'cuda':
            self._copied = torch.cuda.Event()
            self._copied.record()
        ops.jpeg_reconstruct(self._dev_in[plan_at:], N)
        return [out[o: o + i.height * i.width * 3].view(i.height, i.width, 3) for o, i in zip(out_off, infos)]

    def reconstruct(self, hb: HostBatch):
        qt_at, plan_at, nbytes = self._sizes(hb.infos, hb.coef_elems)
        self._grow(nbytes, sum(_align(int(i.coef_count)) for i in hb.infos))
        self._wait_copy()
        stage = self._stage.numpy()
        stage[:2 * hb.coef_elems] = hb.coef[:hb.coef_elems].view(np.uint8)
        stage[qt_at: qt_at + 512 * len(hb.infos)] = hb.qt.reshape(-1).view(np.uint8)
        return self._launch(hb.infos, hb.coef_off, hb.coef_elems)

    def __call__(self, datas):
        datas = [bytes(d) for d in datas]
        if not datas:
            return []
        infos, offs, elems = self._layout(datas)
        qt_at, plan_at, nbytes = self._sizes(infos, elems)
        self._grow(nbytes, sum(_align(int(i.coef_count)) for i in infos))
        self._wait_copy()
        addr = self._stage.data_ptr()
        self._decode_into(datas, infos, offs, addr, addr + qt_at)
        return self._launch(infos, offs, elems)


# --------------------------------------------------------------------------------------------------- the generator
def shuffle_stream(items, buffer_size, rng):
    """tf.data's shuffle: fill a buffer of buffer_size, then emit a uniformly drawn slot and refill it from the input; when the input ends the drawn
    slot is refilled with the last one until the buffer is empty.  rng.integers(n) is the only draw, one per emitted item."""
    buf = []
    for item in items:
        if len(buf) < buffer_size:
            buf.append(item)
            continue
        i = int(rng.integers(len(buf)))
        out, buf[i] = buf[i], item
        yield out
    while buf:
        i = int(rng.integers(len(buf)))
        out, buf[i] = buf[i], buf[-1]
        buf.pop()
        yield out


def _records(paths, verify):
    index = 0
    for p in paths:
        for payload in tf_record_iterator(p, verify):
            yield index, payload
            index += 1


def _voc_payload(examples):
    return [torch.from_numpy(e['ground_truth']) for e in examples]


FLAG_STRIDE = 1024          # the evaluators' class cap: class + FLAG_STRIDE * flag is exact in f32 and splits again without loss


def _voc_payload_difficult(examples):
    """the ground truths with each row's flag folded into its class column (class + FLAG_STRIDE * flag): odtk_augment_boxes drops and compacts rows and
    carries that column through unchanged, so the flag arrives in whatever row its box ends up in.  A record without the feature: flags 0."""
    out = []
    for e in examples:
        gt = e['ground_truth'].copy()
        if 'difficult' in e:
            gt[:, 4] += np.float32(FLAG_STRIDE) * e['difficult'].astype(np.float32)
        out.append(torch.from_numpy(gt))
    return out


def _split_flag_column(gt):
    """[N, pad, 5] with class + FLAG_STRIDE * flag in column 4 -> [N, pad, 6]: class, flag; padding rows (-1) stay -1 in both"""
    folded = gt[..., 4]
    real = folded >= 0
    flag = torch.where(real, torch.floor(folded / FLAG_STRIDE), torch.full_like(folded, -1))
    cls = torch.where(real, folded - FLAG_STRIDE * flag, folded)
    return torch.cat([gt[..., :4], cls[..., None], flag[..., None]], -1)


def _worker(paths, batch_size, buffer_size, seed, verify, decoder, out_q, stop, parse=parse_example, extra=_voc_payload, refusal=None, skipped=None):
    """CPU work only (file reads, CRCs, protobuf, Huffman decoding): never a GPU call.  Puts (host batch, extra(examples)) or an exception.
    parse / extra: record -> example dict with an 'image', examples of a batch -> what travels with the pictures (VOC: the ground truths).
    refusal (imagenet_data's on_unsupported='skip'): image bytes -> None, or the reason the decoder refuses the picture; such a record is left out before
    batching -- the batch is filled from the records that follow -- and counted in skipped[0]."""
    def put(item):
        while not stop.is_set():
            try:
                out_q.put(item, timeout=0.05)
                return True
            except queue.Full:
                pass
        return False
    try:
        rng = np.random.default_rng(seed)
        while not stop.is_set():                                       # .repeat(): every pass reshuffles with the running generator
            batch, emitted = [], 0
            for index, payload in shuffle_stream(_records(paths, verify), buffer_size, rng):
                if stop.is_set():
                    return
                if refusal is not None:
                    try:
                        example = parse(payload)
                    except Exception as e:                             # noqa: BLE001
                        raise ValueError(f'records {[index]}: {e}') from e
                    if refusal(example['image']) is not None:
                        skipped[0] += 1
                        continue
                    batch.append((index, example))
                else:
                    batch.append((index, payload))
                if len(batch) < batch_size:
                    continue
                try:
                    examples = [p if refusal is not None else parse(p) for _, p in batch]
                except Exception as e:                                 # noqa: BLE001
                    raise ValueError(f'records {[i for i, _ in batch]}: {e}') from e
                try:
                    hb = decoder.entropy([e['image'] for e in examples])
                except JpegError as e:
                    pic, _, msg = str(e).partition(': ')
                    k = int(pic.split()[1]) if pic.startswith('picture ') else 0
                    raise JpegError(f'record {batch[k][0]}: {msg}') from None
                if not put((hb, extra(examples))):
                    return
                batch, emitted = [], emitted + 1
            if emitted == 0:                                           # (drop_remainder with fewer records than a batch: nothing, for ever)
                raise ValueError(f'the tfrecords hold fewer than batch_size = {batch_size} records')
    except BaseException as e:                                          # noqa: BLE001 -- handed to the consumer, which raises it
        put(e)


class _VOCIterator:
    def __init__(self, gen):
        self._decoder, self._augmentor = gen._decoder, gen._augmentor
        self._q = queue.Queue(maxsize=max(1, gen.prefetch))
        self._stop = threading.Event()
        self._thread = threading.Thread(target=_worker, name=gen.THREAD_NAME, daemon=True,
                                        args=(gen.tfrecords, gen.batch_size, gen.buffer_size, gen.seed, gen.verify, gen._decoder, self._q, self._stop),
                                        kwargs=gen._worker_options())
        self._finish = gen._finish
        self._thread.start()

    def __iter__(self):
        return self

    def __next__(self):
        if self._stop.is_set():
            raise StopIteration
        while True:
            try:
                item = self._q.get(timeout=0.1)
                break
            except queue.Empty:
                if not self._thread.is_alive() and self._q.empty():
                    self.close()
                    raise RuntimeError('the loader thread ended without a result') from None
        if isinstance(item, BaseException):
            self.close()
            raise item
        hb, extra = item
        images = self._decoder.reconstruct(hb)             # upload + odtk_jpeg_reconstruct, on the consumer's thread and current stream
        return self._finish(images, extra)

    def close(self):
        self._stop.set()
        if self._thread is not threading.current_thread():
            self._thread.join()

    def __del__(self):
        try:
            self._stop.set()
        except Exception:                                   # noqa: BLE001 -- interpreter shutdown
            pass


class VOCGenerator:
    """see get_generator"""
    endless = True                  # evaluate() asks for num_images (or num_val) before it reads a stream that never ends
    THREAD_NAME = 'odtk-voc-loader'

    def _worker_options(self):
        """keyword arguments of _worker: the record layout of this generator (imagenet_data.ImageNetGenerator has its own)"""
        return {'extra': _voc_payload_difficult} if self.with_difficult else {}

    def _finish(self, images, gts):
        """the consumer's last stage: decoded pictures + what the worker sent with them -> one item of the stream"""
        if not self.with_difficult:
            return self._augmentor(images, gts)
        images, gt = self._augmentor(images, gts)
        return images, _split_flag_column(gt)

    with_difficult = False

    def __init__(self, tfrecords, batch_size, buffer_size, image_preprocess_config, device='cuda:0', seed=None, prefetch=2, verify=True, decoder=None,
                 augmentor=None, with_difficult=False):
        self.with_difficult = bool(with_difficult)
        self.tfrecords = [tfrecords] if isinstance(tfrecords, (str, os.PathLike)) else list(tfrecords)
        self.batch_size, self.buffer_size, self.prefetch, self.verify, self.seed = int(batch_size), max(1, int(buffer_size)), int(prefetch), verify, seed
        assert self.batch_size > 0 and self.tfrecords
        if augmentor is None:
            from .augment import Augmentor
            augmentor = Augmentor(seed=seed, **image_preprocess_config)
        self._augmentor = augmentor
        self._decoder = decoder if decoder is not None else JpegBatchDecoder(device)
        self._last = None

    def __iter__(self):
        last = self._last() if self._last is not None else None
        if last is not None:
            last.close()                                    # one live stream per generator, like the reference's single re-initialised iterator
        it = _VOCIterator(self)
        self._last = weakref.ref(it)
        return it


def get_generator(tfrecords, batch_size, buffer_size, image_preprocess_config, device='cuda:0', seed=None, prefetch=2, verify=True, with_difficult=False,
                  **hooks):
    """tfrecord_voc_utils.get_generator: `.tfrecord` shards -> endless batches ([B, H, W, 3] f32 pictures, [B, pad_truth_to, 5] ground truth), exactly what
    odtk.augment.Augmentor returns with ground truth (image_preprocess_config is the reference's image_augmentor_config and needs pad_truth_to).
    Order of the stages as in the reference: records in file order -> shuffle buffer of buffer_size (shuffle_stream) -> batches of batch_size, the
    remainder of a pass dropped -> repeated without end.  Each iter() of the returned object restarts the stream (and ends the previous one).  A daemon
    thread reads, parses and Huffman-decodes up to `prefetch` batches ahead; upload, reconstruction and augmentation run on the consumer's thread and
    current stream.  A record whose JPEG the decoder refuses raises JpegError('record <index>: <message>') from next().  `seed` fixes the shuffle and
    the augmentor's draws.  with_difficult=True: ground truth [B, pad_truth_to, 6], column 5 the `difficult` flag (0 / 1; 0 for records written without
    it; -1 in padding rows) of the box that the augmentor left in that row -- what odtk.evaluate() takes; training code keeps the default.
    hooks (tests): decoder=, augmentor= replace the two device stages."""
    return VOCGenerator(tfrecords, batch_size, buffer_size, image_preprocess_config, device, seed, prefetch, verify, with_difficult=with_difficult,
                        **hooks)
