"""TFRecord shards without TensorFlow: the container the reference's dataset arrives in (``train-*`` / ``validation-*``,
functions/input_fns.py:33-94, utils/data_util.py:161-265 and :389-473), read into batches that
:func:`assembled_cnn_amd.input_pipeline.preprocess_batch` and ``Trainer.train_step`` take as they are.

  * framing -- :class:`RecordFile`, :func:`write_records`: ``uint64 length | uint32 masked_crc32c(length) | data |
    uint32 masked_crc32c(data)``, little endian, the mask ``((c >> 15) | (c << 17)) + 0xa282ead8`` (tf_bundle.mask_crc);
  * ``tf.train.Example`` in the protobuf wire format -- :func:`parse_example`, :func:`encode_example`;
  * the reference's parsers by name -- :func:`parse_example_proto`, :func:`parse_record_sup`, :func:`parse_record`;
  * the dataset -- :class:`RecordDataset` (``input_fn`` + ``process_record_dataset``), :func:`get_filenames`,
    :func:`batch_size_and_epochs` (``input_fn_cls``'s arithmetic).

TensorFlow's record reader verifies the CRC-32C behind every payload.  Here a batch's payloads are gathered into a pinned
staging buffer of this module's own, copied to the device once and checked there by one launch (``ops.crc32c_spans``):
the host checksum (tf_bundle.crc32c, ~70 MB/s) cannot keep up with a training step.  With ``parse='device'`` the Examples
are walked there too (``ops.example_parse``, ``ops.example_label_rows``).  DESIGN.md section 1.3 has the rules.
"""
from __future__ import annotations

import glob
import os
import struct
from typing import Dict, Iterable, Iterator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import dp, ops, staging
from . import lib as _lib
from .tf_bundle import _crc32c_bytes, _put_varint, crc32c, mask_crc

SPAN_DTYPE = np.dtype(_lib.SpanDesc)
VERIFY_MODES = ('device', 'host', 'none')
PARSE_MODES = ('host', 'device')
ROW_DTYPE = np.dtype(_lib.ExampleRow)
_HEADER, _FOOTER = 12, 4


# ---- framing --------------------------------------------------------------------------------------------------------
def frame_record(payload) -> bytes:
  """one record: length, masked crc of the length, the payload, masked crc of the payload"""
  payload = bytes(payload)
  head = struct.pack('<Q', len(payload))
  return head + struct.pack('<I', mask_crc(crc32c(head))) + payload + struct.pack('<I', mask_crc(crc32c(payload)))


def write_records(path: str, payloads: Iterable) -> int:
  """``payloads`` (bytes-like) as one shard at ``path``; returns the number of records written"""
  n = 0
  with open(path, 'wb') as fh:
    for p in payloads:
      fh.write(frame_record(p))
      n += 1
  return n


class RecordFile(object):
  """A shard, mapped (a path) or wrapped (bytes-like), walked once: ``offsets`` / ``lengths`` (int64) of the payloads,
  ``stored`` (uint32) the masked payload crcs as the file holds them, ``starts`` the byte position of each record.  The
  crc of every length field is verified here, on the host (8 bytes a record); the payload crcs are NOT (RecordDataset's
  ``verify``).  A truncated record or a corrupt length raises ValueError naming the file and the byte position -- TensorFlow's
  DataLossError.  A file that ends exactly behind a record is a complete, shorter file: the format cannot tell."""

  def __init__(self, path_or_bytes, name: Optional[str] = None):
    if isinstance(path_or_bytes, (str, os.PathLike)):
      self.name = name or os.fspath(path_or_bytes)
      size = os.path.getsize(path_or_bytes)
      self.data = np.memmap(path_or_bytes, dtype=np.uint8, mode='r') if size else np.zeros(0, np.uint8)
    else:
      self.name = name or '<bytes>'
      self.data = np.frombuffer(memoryview(path_or_bytes), dtype=np.uint8)
    data, size = self.data, int(self.data.size)
    offsets, lengths, stored = [], [], []
    pos = 0
    while pos < size:
      if size - pos < _HEADER:
        raise ValueError('%s: truncated record header at byte %d' % (self.name, pos))
      head = data[pos:pos + _HEADER].tobytes()
      length, crc = struct.unpack('<QI', head)
      if mask_crc(_crc32c_bytes(head[:8])) != crc:
        raise ValueError('%s: corrupt record length at byte %d' % (self.name, pos))
      if length > size - pos - _HEADER - _FOOTER:
        raise ValueError('%s: truncated record at byte %d (%d payload bytes, %d left in the file)' % (
            self.name, pos, length, max(size - pos - _HEADER - _FOOTER, 0)))
      offsets.append(pos + _HEADER)
      lengths.append(length)
      stored.append(struct.unpack('<I', data[pos + _HEADER + length:pos + _HEADER + length + _FOOTER].tobytes())[0])
      pos += _HEADER + length + _FOOTER
    self.offsets = np.asarray(offsets, dtype=np.int64)
    self.lengths = np.asarray(lengths, dtype=np.int64)
    self.stored = np.asarray(stored, dtype=np.uint32)
    self.starts = self.offsets - _HEADER

  def __len__(self) -> int:
    return int(self.offsets.size)

  def payload(self, i: int) -> np.ndarray:
    """uint8 view of record i's payload (no copy)"""
    o = int(self.offsets[i])
    return self.data[o:o + int(self.lengths[i])]


# ---- tf.train.Example (protobuf wire format) ------------------------------------------------------------------------
def _varint(buf, pos: int, end: int) -> Tuple[int, int]:
  """(value, next position) of the varint at buf[pos:end]; at most ten bytes, the tenth carrying one bit"""
  n = shift = 0
  for k in range(10):
    if pos >= end:
      raise ValueError('truncated varint')
    b = buf[pos]
    pos += 1
    n |= (b & 0x7f) << shift
    if not b & 0x80:
      if k == 9 and b > 1:
        raise ValueError('varint overflows 64 bits')
      return n, pos
    shift += 7
  raise ValueError('overlong varint')


def _fields(buf, pos: int, end: int):
  """(field number, wire type, value, begin, end) of the message at buf[pos:end]: value is the integer of a varint /
  fixed field, begin .. end the bytes of a length-delimited or fixed one.  Never indexes past ``end``."""
  while pos < end:
    key, pos = _varint(buf, pos, end)
    fn, wt = key >> 3, key & 7
    if wt == 0:
      v, nxt = _varint(buf, pos, end)
      yield fn, wt, v, pos, nxt
    elif wt in (1, 5):
      nxt = pos + (8 if wt == 1 else 4)
      if nxt > end:
        raise ValueError('truncated fixed-width field')
      yield fn, wt, None, pos, nxt
    elif wt == 2:
      n, pos = _varint(buf, pos, end)
      nxt = pos + n
      if nxt > end:
        raise ValueError('truncated length-delimited field')
      yield fn, wt, None, pos, nxt
    else:
      raise ValueError('unsupported protobuf wire type %d' % wt)
    pos = nxt


_KINDS = {1: 'bytes', 2: 'float', 3: 'int64'}


def _feature(buf, pos: int, end: int):
  """Feature{oneof 1: BytesList, 2: FloatList, 3: Int64List} -> (kind, value): value a list of (begin, end) spans of buf,
  a float32 array or an int64 array; (None, None) for a Feature with no kind set.  The last kind in the message wins."""
  kind, value = None, None
  for fn, wt, _, b, e in _fields(buf, pos, end):
    if fn not in _KINDS or wt != 2:
      continue
    kind = _KINDS[fn]
    if kind == 'bytes':
      value = [(b2, e2) for f2, w2, _, b2, e2 in _fields(buf, b, e) if f2 == 1 and w2 == 2]
    elif kind == 'float':
      parts = []
      for f2, w2, _, b2, e2 in _fields(buf, b, e):
        if f2 != 1 or w2 not in (2, 5):
          continue
        if (e2 - b2) % 4:
          raise ValueError('packed float list of %d bytes' % (e2 - b2))
        parts.append(np.frombuffer(bytes(buf[b2:e2]), dtype='<f4'))
      value = np.concatenate(parts).astype(np.float32) if parts else np.zeros(0, np.float32)
    else:
      vals = []
      for f2, w2, v2, b2, e2 in _fields(buf, b, e):
        if f2 != 1 or w2 not in (0, 2):
          continue
        if w2 == 0:
          vals.append(v2)
        else:
          while b2 < e2:
            v2, b2 = _varint(buf, b2, e2)
            vals.append(v2)
      value = np.array(vals, dtype=np.uint64).view(np.int64) if vals else np.zeros(0, np.int64)   # ten-byte varints are negative
  return kind, value


def _example(buf) -> Dict[str, tuple]:
  """name -> (kind, value) of a serialised Example, bytes values as spans of buf; the last duplicate key wins"""
  out: Dict[str, tuple] = {}
  end = len(buf)
  for fn, wt, _, b, e in _fields(buf, 0, end):
    if fn != 1 or wt != 2:
      continue                                                     # Example{1: Features}
    for f2, w2, _, b2, e2 in _fields(buf, b, e):
      if f2 != 1 or w2 != 2:
        continue                                                   # Features{1: map entry {1: key, 2: Feature}}
      key, feat = b'', (None, None)
      for f3, w3, _, b3, e3 in _fields(buf, b2, e2):
        if f3 == 1 and w3 == 2:
          key = bytes(buf[b3:e3])
        elif f3 == 2 and w3 == 2:
          feat = _feature(buf, b3, e3)
      try:
        out[key.decode('utf-8')] = feat
      except UnicodeDecodeError:
        raise ValueError('feature name is not UTF-8')
  return out


def _buffer(payload):
  """bytes-like or 1-D uint8 array -> a byte view whose elements are Python ints and whose slices copy nothing"""
  if isinstance(payload, np.ndarray) and (payload.dtype != np.uint8 or payload.ndim != 1):
    raise ValueError('a record payload is a 1-D uint8 array or bytes-like')
  return memoryview(payload).cast('B')


def parse_example(payload) -> Dict[str, object]:
  """A serialised ``tf.train.Example`` -> {name: list of bytes | float32 array | int64 array} (None for a Feature with no
  kind set).  Packed and unpacked lists are accepted, unknown fields skipped, the last duplicate key wins; ValueError on
  any truncation or overlong varint."""
  buf = _buffer(payload)
  return {k: ([bytes(buf[b:e]) for b, e in v] if kind == 'bytes' else v) for k, (kind, v) in _example(buf).items()}


def _len_field(fn: int, body: bytes) -> bytes:
  return _put_varint((fn << 3) | 2) + _put_varint(len(body)) + body


def encode_example(features: Dict[str, object]) -> bytes:
  """The inverse of parse_example, lists packed as TensorFlow writes them: a list / tuple of bytes is a BytesList, a
  floating array a FloatList, an integer array an Int64List, None a Feature with no kind.  Keys in the dict's order."""
  entries = b''
  for name, v in features.items():
    if v is None:
      feat = b''
    elif isinstance(v, (list, tuple)) and all(isinstance(x, (bytes, bytearray)) for x in v):
      feat = _len_field(1, b''.join(_len_field(1, bytes(x)) for x in v))
    else:
      a = np.asarray(v)
      if a.dtype.kind == 'f':
        body = a.astype('<f4').tobytes()
        feat = _len_field(2, _len_field(1, body) if body else b'')
      elif a.dtype.kind in 'iub':
        body = b''.join(_put_varint(int(x) & 0xffffffffffffffff) for x in a.reshape(-1))
        feat = _len_field(3, _len_field(1, body) if body else b'')
      else:
        raise ValueError('feature %r: bytes, floats or integers' % name)
    entries += _len_field(1, _len_field(1, name.encode('utf-8')) + _len_field(2, feat))
  return _len_field(1, entries)


# ---- the reference's parsers ----------------------------------------------------------------------------------------
_BBOX = ('image/object/bbox/ymin', 'image/object/bbox/xmin', 'image/object/bbox/ymax', 'image/object/bbox/xmax')


def _fixed(ex, name, kind, default):
  """tf.FixedLenFeature([], default_value): missing, or no kind set -> the default; another kind, or a value count
  other than one -> ValueError"""
  got, v = ex.get(name, (None, None))
  if got is None:
    return default
  if got != kind:
    raise ValueError('feature %s: expected %s, the record holds %s' % (name, kind, got))
  if len(v) != 1:
    raise ValueError('feature %s: %d values where exactly one is expected' % (name, len(v)))
  return v[0]


def _var(ex, name, kind):
  """tf.VarLenFeature: the values; empty when missing or unset; another kind -> ValueError"""
  got, v = ex.get(name, (None, None))
  if got is None:
    return np.zeros(0, np.float32)
  if got != kind:
    raise ValueError('feature %s: expected %s, the record holds %s' % (name, kind, got))
  return v


def _proto(buf):
  """parse_example_proto on a buffer, the encoded image as a span of it"""
  ex = _example(buf)
  enc = _fixed(ex, 'image/encoded', 'bytes', (0, 0))
  name = _fixed(ex, 'image/filename', 'bytes', (0, 0))
  label = int(_fixed(ex, 'image/class/label', 'int64', -1))
  coords = [_var(ex, k, 'float') for k in _BBOX]
  if len({c.size for c in coords}) != 1:
    raise ValueError('bounding-box coordinate lists of different lengths: %s' % [int(c.size) for c in coords])
  bbox = np.stack(coords, axis=1).reshape(1, -1, 4).astype(np.float32)      # [1, nboxes, (ymin, xmin, ymax, xmax)]
  return enc, np.int32(np.int64(label).astype(np.int32)), bbox, bytes(buf[name[0]:name[1]]), _var(ex, 'image/logit', 'float')


def parse_example_proto(payload, ret_dict: bool = False):
  """data_util.parse_example_proto (:173-208): (encoded image bytes, label int32, bbox float32 [1, nboxes, 4] in (ymin,
  xmin, ymax, xmax) order, filename bytes, logit float32 values); defaults b'' and -1, empty sparse features.  With
  ``ret_dict`` the features by name instead (the sparse ones as their value arrays)."""
  buf = _buffer(payload)
  enc, label, bbox, filename, logit = _proto(buf)
  encoded = bytes(buf[enc[0]:enc[1]])
  if ret_dict:
    out = {'image/encoded': encoded, 'image/filename': filename, 'image/class/label': np.int64(label), 'image/logit': logit}
    out.update({k: bbox[0, :, i] for i, k in enumerate(_BBOX)})
    return out
  return encoded, label, bbox, filename, logit


def _kd_label(label, logit, num_classes: int) -> np.ndarray:
  """concat(one_hot(label, num_classes), reshape(logit, [num_classes])), float32: a row Trainer.split_labels takes"""
  if logit.size != num_classes:
    raise ValueError('image/logit holds %d values, num_classes is %d' % (logit.size, num_classes))
  row = np.zeros(2 * num_classes, np.float32)
  if 0 <= int(label) < num_classes:                 # tf.one_hot: an index outside the depth gives a row of zeros
    row[int(label)] = 1.0
  row[num_classes:] = logit
  return row


def proto_row(buf, base: int = 0):
  """_proto's result as the row asm_example_parse writes for a class-0 record whose first byte lies at ``base`` (one
  ROW_DTYPE record), and the logit values.  The values need not lie packed in the payload, so ``logit_offset`` is ``base``:
  the caller has the values.  Raises what _proto raises."""
  (b, e), label, bbox, _, logit = _proto(buf)
  nb, ne = _fixed(_example(buf), 'image/filename', 'bytes', (0, 0))
  row = np.zeros((), dtype=ROW_DTYPE)
  row['label'], row['logit_count'], row['n_boxes'] = label, logit.size, bbox.shape[1]
  row['enc_offset'], row['enc_length'] = base + b, e - b
  row['name_offset'], row['name_length'] = base + nb, ne - nb
  row['logit_offset'] = base
  return row, logit


def parse_record_sup(payload, return_logits: bool = False, num_classes: int = 1001) -> dict:
  """data_util.parse_record_sup (:210-235) up to the image preprocessing, which runs on the device for a whole batch
  (preprocess_batch): {'image': the encoded bytes, 'label': int32, or with return_logits the float32 [2 * num_classes]
  row}.  As in the reference the bounding box is parsed and not passed on."""
  encoded, label, _, _, logit = parse_example_proto(payload)
  return {'image': encoded, 'label': _kd_label(label, logit, num_classes) if return_logits else label}


def parse_record(payload, return_logits: bool = False, num_classes: int = 1001, return_filename: bool = False):
  """data_util.parse_record (:237-265) up to the image preprocessing: (encoded bytes, label[, filename])"""
  encoded, label, _, filename, logit = parse_example_proto(payload)
  if return_logits:
    assert num_classes == 1001, 'Only support ImageNet for Knowledge Distillation yet'
    label = _kd_label(label, logit, num_classes)
  return (encoded, label, filename) if return_filename else (encoded, label)


def get_filenames(is_training: bool, data_dir: str, train_regex: str = 'train-*', val_regex: str = 'validation-*') -> List[str]:
  """data_util.get_filenames (:161-170): the shards matching the pattern, sorted"""
  return sorted(glob.glob(os.path.join(data_dir, train_regex if is_training else val_regex)))


def batch_size_and_epochs(batch_size: int, num_epochs: int, mixup_type: int, is_training: bool, num_gpus: int = 1):
  """input_fn_cls's arithmetic (functions/input_fns.py:97-104): mixup type 1 in training reads two batches for one, so
  batch and epochs double; then the per-device batch.  -> (batch_size, num_epochs) for RecordDataset"""
  if mixup_type == 1 and is_training:
    batch_size, num_epochs = batch_size * 2, num_epochs * 2
  return dp.per_device_batch_size(batch_size, num_gpus), num_epochs


# ---- the dataset ----------------------------------------------------------------------------------------------------
class Batch(NamedTuple):
  encoded: List[np.ndarray]             # uint8 views into the mapped shards: preprocess_batch(batch.encoded, ...)
  labels: torch.Tensor                  # int32 [B], or float32 [B, 2 * num_classes] with return_logits
  filenames: List[bytes]
  origins: List[Tuple[str, int]]        # (shard, byte position of the record in it)
  # keep_payloads: (the dataset's uint8 device staging buffer, int64 [B, 2] offset and length of each record's image/encoded
  # bytes in it), valid until the next batch is drawn: preprocess_batch(..., jpeg_parse='device', jpeg_resident=payloads)
  payloads: Optional[Tuple[torch.Tensor, np.ndarray]] = None


def _shuffled(items: Iterator, buffer_size: int, rng: np.random.Generator) -> Iterator:
  """tf.data's shuffle: fill a buffer, then emit a uniformly drawn slot and refill it; drain at the end"""
  buf = []
  for it in items:
    if len(buf) < buffer_size:
      buf.append(it)
      continue
    k = int(rng.integers(len(buf)))
    out, buf[k] = buf[k], it
    yield out
  while buf:
    k = int(rng.integers(len(buf)))
    buf[k], buf[-1] = buf[-1], buf[k]
    yield buf.pop()


def _interleaved(files: Iterator[str], cycle_length: int) -> Iterator[Tuple[RecordFile, int]]:
  """tf.data's interleave with block_length 1: cycle_length shards open, one record from each in turn; an exhausted
  shard's slot takes the next file at once; with no file left the slot closes"""
  def opened():
    for name in files:
      f = RecordFile(name)
      if len(f):
        return [f, 0]
    return None
  slots = []
  while len(slots) < cycle_length:
    s = opened()
    if s is None:
      break
    slots.append(s)
  k = 0
  while slots:
    f, i = slots[k]
    if i == len(f):
      s = opened()
      if s is None:
        del slots[k]
        k = k % len(slots) if slots else 0
        continue
      slots[k] = s
      f, i = s
    slots[k][1] = i + 1
    yield f, i
    k = (k + 1) % len(slots)


class RecordDataset(object):
  """``input_fn`` + ``process_record_dataset`` (functions/input_fns.py:33-94, utils/data_util.py:389-473) as an iterator
  of :class:`Batch`:

    1. in training the file list is shuffled (a shuffle buffer of ``num_train_files``, default all of them);
    2. ``cycle_length`` shards are interleaved one record at a time, an exhausted shard replaced by the next file;
    3. in training a shuffle buffer of ``shuffle_buffer`` records;
    4. shuffle before repeat: no record crosses an epoch boundary, files and buffer are drawn anew every epoch;
    5. ``num_epochs`` repetitions;  6. batches of ``batch_size`` (which may span two epochs), ``drop_remainder``.

  TensorFlow's random stream cannot be reproduced: ``seed`` and a numpy Generator supply the draws, as in
  input_pipeline.  The reference's ``dataset.take(...)`` (data_util.py:424) discards its result and so has no effect; it is
  not implemented.  Labels are int32 [B], or with ``return_logits`` float32 [B, 2 * num_classes] rows
  concat(one_hot, teacher logits) (parse_record_sup) for Trainer.split_labels.  The bounding boxes are parsed and, as in
  parse_record_sup, not passed on: the crop is train_window's whole-image crop.

  ``verify``: 'device' -- the batch's payloads go through this module's pinned staging buffer to ``device`` in one copy and
  ops.crc32c_spans checks them against the stored crcs; the status is read before the batch is yielded.  'host' -- the same
  through tf_bundle.crc32c (slow: CPU tests and tools).  'none' -- no check.  A mismatch raises ValueError naming the shard
  and the record's byte position.

  ``keep_payloads``: the batch's payloads go to ``device`` under every ``verify`` mode (which then only decides about the
  checksum launch and its read-back) and ``Batch.payloads`` names the encoded images in that buffer, so that the JPEG
  decoder reads them where they are instead of uploading them again.  The buffer is the dataset's own and is refilled by
  the next batch.

  ``parse``: 'host' -- records._proto record by record.  'device' -- the payloads go to ``device`` as above,
  ops.example_parse walks every record's Example there and the rows come back with the checksum status behind one wait;
  a record the device does not classify as plain (asm_example_row.cls != 0) is parsed by the host as before, so results and
  error texts are the same.  With ``return_logits`` the label rows are written on the device (ops.example_label_rows) and
  ``Batch.labels`` is that float32 device tensor; without, it is the int32 CPU tensor of 'host'."""

  def __init__(self, filenames: Sequence[str], is_training: bool, batch_size: int, shuffle_buffer: int,
               num_train_files: Optional[int] = None, num_epochs: int = 1, cycle_length: int = 20,
               drop_remainder: bool = False, return_logits: bool = False, num_classes: int = 1001,
               seed: Optional[int] = None, verify: str = 'device', device='cuda', keep_payloads: bool = False,
               parse: str = 'host'):
    if verify not in VERIFY_MODES:
      raise ValueError('verify must be one of %s, got %r' % (VERIFY_MODES, verify))
    if parse not in PARSE_MODES:
      raise ValueError('parse must be one of %s, got %r' % (PARSE_MODES, parse))
    if batch_size < 1 or cycle_length < 1 or num_epochs < 0 or (is_training and shuffle_buffer < 1):
      raise ValueError('batch_size, cycle_length and shuffle_buffer are positive, num_epochs is not negative')
    self.filenames = list(filenames)
    self.is_training, self.batch_size, self.shuffle_buffer = bool(is_training), int(batch_size), int(shuffle_buffer)
    self.num_train_files = len(self.filenames) if num_train_files is None else int(num_train_files)
    self.num_epochs, self.cycle_length, self.drop_remainder = int(num_epochs), int(cycle_length), bool(drop_remainder)
    self.return_logits, self.num_classes, self.seed = bool(return_logits), int(num_classes), seed
    self.verify, self.device, self.keep_payloads = verify, torch.device(device), bool(keep_payloads)
    self.parse = parse
    self._staging = staging.Staging()     # its own: a record upload and a pixel upload do not wait on each other's buffer
    self._dev = None                      # grow-only device buffer the payloads are copied to

  def records(self) -> Iterator[Tuple[RecordFile, int]]:
    """(shard, record index) in the order the batches are cut from"""
    rng = np.random.default_rng(self.seed)
    for _ in range(self.num_epochs):
      files = iter(self.filenames)
      if self.is_training:
        files = _shuffled(files, max(self.num_train_files, 1), rng)
      recs = _interleaved(files, self.cycle_length)
      yield from (_shuffled(recs, self.shuffle_buffer, rng) if self.is_training else recs)

  def __iter__(self) -> Iterator[Batch]:
    pending = []
    for rec in self.records():
      pending.append(rec)
      if len(pending) == self.batch_size:
        yield self._batch(pending)
        pending = []
    if pending and not self.drop_remainder:
      yield self._batch(pending)

  def _mismatch(self, f: RecordFile, i: int, what: str):
    return ValueError('%s: corrupt record at byte %d (%s)' % (f.name, int(f.starts[i]), what))

  def _verify_host(self, recs):
    for f, i in recs:
      if mask_crc(crc32c(f.payload(i))) != int(f.stored[i]):
        raise self._mismatch(f, i, 'payload checksum mismatch')

  def _upload(self, recs):
    """the batch's payloads at 16-byte slots -> the pinned staging buffer -> ONE asynchronous copy to the device buffer;
    returns (device view of the slots, int64 slot offsets, int64 payload lengths)"""
    lengths = np.array([f.lengths[i] for f, i in recs], dtype=np.int64)
    offsets, total = staging.slot_layout(lengths)
    total = max(total, 16)
    if self._dev is None or self._dev.numel() < total:
      self._dev = torch.empty(int(total * 1.25) + 4096, dtype=torch.uint8, device=self.device)
    dev = self._dev[:total]
    self._staging.stage_into(dev, [f.payload(i) for f, i in recs], offsets)
    return dev, offsets, lengths

  def _span_table(self, recs, uploaded):
    """the device table of the uploaded payloads' spans, each with the masked crc its record stores"""
    _, offsets, lengths = uploaded
    spans = np.zeros(len(recs), dtype=SPAN_DTYPE)
    spans['offset'], spans['length'], spans['flags'] = offsets, lengths, 1
    spans['expect_masked'] = [f.stored[i] for f, i in recs]
    return staging.upload_table(spans, self.device)

  def _checked(self, recs, status):
    for (f, i), st in zip(recs, status):
      if st:
        raise self._mismatch(f, i, 'payload checksum mismatch' if st == _lib.SPAN_EMISMATCH else 'span status %d' % st)

  def _verify_device(self, recs, uploaded):
    _, status = ops.crc32c_spans(uploaded[0], self._span_table(recs, uploaded), len(recs))
    self._checked(recs, status.cpu().numpy())   # waits for the copy as well: the staging buffer is free for the next batch

  def _host_row(self, f: RecordFile, i: int, base: int):
    """proto_row of one record, with the KD row when the dataset returns logits; errors in the batch's wrapper"""
    try:
      row, logit = proto_row(_buffer(f.payload(i)), base)
      return row, _kd_label(row['label'], logit, self.num_classes) if self.return_logits else None
    except ValueError as err:
      raise ValueError('%s: record at byte %d: %s' % (f.name, int(f.starts[i]), err))

  def assemble(self, recs, rows: np.ndarray, uploaded=None, label_rows: Optional[torch.Tensor] = None) -> Batch:
    """(records, their asm_example_row rows) -> Batch, what the host loop of parse='host' makes.  ``rows``: ROW_DTYPE [B],
    offsets counted from ``uploaded``'s slots (from 0 without it).  A row with cls != 0 is replaced by the host's parse of
    that record, which raises for it what it raises today.  ``label_rows`` (return_logits): the float32 [B, 2 * num_classes]
    device tensor asm_example_label_rows wrote for these rows; the rows the host parsed are patched in with one copy.
    Without it the rows are taken as made by proto_row (their logits do not lie at logit_offset) and parsed here."""
    slots = uploaded[1] if uploaded is not None else np.zeros(len(recs), np.int64)
    rows = rows.copy()
    encoded, names, origins, patched, kd = [], [], [], [], []
    for k, (f, i) in enumerate(recs):
      base = int(slots[k])
      if rows[k]['cls'] != 0 or (self.return_logits and label_rows is None):
        rows[k], row = self._host_row(f, i, base)
        patched.append(k)
        kd.append(row)
      elif self.return_logits and rows[k]['logit_count'] != self.num_classes:
        raise ValueError('%s: record at byte %d: image/logit holds %d values, num_classes is %d' % (
            f.name, int(f.starts[i]), rows[k]['logit_count'], self.num_classes))
      payload = f.payload(i)
      b, nb = int(rows[k]['enc_offset']) - base, int(rows[k]['name_offset']) - base
      encoded.append(payload[b:b + int(rows[k]['enc_length'])])
      names.append(payload[nb:nb + int(rows[k]['name_length'])].tobytes())
      origins.append((f.name, int(f.starts[i])))
    if not self.return_logits:
      labels = torch.from_numpy(rows['label'].astype(np.int32))
    elif label_rows is None:
      labels = torch.from_numpy(np.stack(kd).astype(np.float32))
    else:
      labels = label_rows
      if patched:
        labels[torch.as_tensor(patched, device=labels.device)] = torch.from_numpy(np.stack(kd)).to(labels.device)
    payloads = None
    if self.keep_payloads:
      payloads = (uploaded[0], np.stack([rows['enc_offset'], rows['enc_length']], axis=1).astype(np.int64))
    return Batch(encoded, labels, names, origins, payloads)

  def _batch_device(self, recs) -> Batch:
    """parse='device': the checksum launch (verify='device'), the parse launch and, with return_logits, the label-row launch
    are enqueued behind the upload; status words and rows come back in one copy behind one wait"""
    n = len(recs)
    uploaded = self._upload(recs)
    dev = uploaded[0]
    if self.verify == 'host':
      self._verify_host(recs)
    spans = self._span_table(recs, uploaded)
    back = [ops.crc32c_spans(dev, spans, n)[1].view(torch.uint8)] if self.verify == 'device' else []
    rows_dev = ops.example_parse(dev, spans, n)
    back.append(rows_dev)
    label_rows = ops.example_label_rows(dev, rows_dev, n, self.num_classes)[0] if self.return_logits else None
    host = torch.cat(back).cpu().numpy()          # waits for the copy as well: the staging buffer is free for the next batch
    if self.verify == 'device':
      self._checked(recs, host[:4 * n].view(np.int32))
    return self.assemble(recs, host[host.size - ROW_DTYPE.itemsize * n:].view(ROW_DTYPE), uploaded, label_rows)

  def _batch(self, recs) -> Batch:
    if self.parse == 'device':
      return self._batch_device(recs)
    uploaded = self._upload(recs) if self.verify == 'device' or self.keep_payloads else None
    if self.verify == 'device':
      self._verify_device(recs, uploaded)
    elif self.verify == 'host':
      self._verify_host(recs)
    encoded, labels, names, origins, spans = [], [], [], [], []
    for f, i in recs:
      payload = f.payload(i)
      try:
        (b, e), label, _, name, logit = _proto(_buffer(payload))
        labels.append(_kd_label(label, logit, self.num_classes) if self.return_logits else label)
      except ValueError as err:
        raise ValueError('%s: record at byte %d: %s' % (f.name, int(f.starts[i]), err))
      encoded.append(payload[b:e])
      spans.append((b, e - b))
      names.append(name)
      origins.append((f.name, int(f.starts[i])))
    lab = np.stack(labels).astype(np.float32) if self.return_logits else np.asarray(labels, dtype=np.int32)
    payloads = None
    if self.keep_payloads:
      where = np.array(spans, dtype=np.int64).reshape(-1, 2)
      where[:, 0] += uploaded[1]             # the record's slot + the image's position in the record
      payloads = (uploaded[0], where)
    return Batch(encoded, torch.from_numpy(lab), names, origins, payloads)
