"""TFRecord reading without TensorFlow and without a GPU (assembled_cnn_amd/records.py): the framing and the Example wire
format against known answers (computed with tf_bundle's codecs, which the RFC 3720 vectors pin), round trips, every
truncation, the reference parsers' semantics, the dataset's order, and the argument checks of asm_crc32c_spans on the real
library.  The device check of a batch runs here on a CPU double of asm_crc32c_spans composed from tf_bundle.crc32c."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

from assembled_cnn_amd import records as R
from assembled_cnn_amd import tf_bundle
from tests.cpu_double import CpuDouble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL7 = bytes.fromhex('0a1c0a1a0a11696d6167652f636c6173732f6c6162656c12051a030a0107')


class SpansDouble(CpuDouble):
  """asm_crc32c_spans on the host: the header's contract, through tf_bundle's codecs"""

  def __init__(self):
    super().__init__()
    self.launches = 0

  def asm_crc32c_spans(self, buf, buf_bytes, spans, n, crc, status, stream):
    from assembled_cnn_amd import lib
    if not (buf and spans and crc and status) or n < 0:
      return lib.ASM_EINVAL
    if n == 0:
      return lib.ASM_OK
    self.launches += 1
    data = np.ctypeslib.as_array((ctypes.c_uint8 * max(buf_bytes, 1)).from_address(buf))[:buf_bytes]
    table = (lib.SpanDesc * n).from_address(spans)
    out_c = np.ctypeslib.as_array((ctypes.c_uint32 * n).from_address(crc))
    out_s = np.ctypeslib.as_array((ctypes.c_int32 * n).from_address(status))
    for i, d in enumerate(table):
      if d.offset < 0 or d.length < 0 or d.offset > buf_bytes or d.length > buf_bytes - d.offset:
        out_c[i], out_s[i] = 0, lib.SPAN_EDESC
        continue
      c = tf_bundle.crc32c(data[d.offset:d.offset + d.length])
      out_c[i] = c
      out_s[i] = lib.SPAN_EMISMATCH if (d.flags & 1) and tf_bundle.mask_crc(c) != d.expect_masked else 0
    return lib.ASM_OK


@pytest.fixture
def spans_double():
  from assembled_cnn_amd import ops
  d = SpansDouble()
  ops.set_library(d, is_double=True)
  yield d
  ops.set_library(None, is_double=False)


# ---- framing ---------------------------------------------------------------------------------------------------------
def test_crc_vectors_the_known_answers_rest_on():
  assert tf_bundle.crc32c(b'\x00' * 32) == 0x8a9136aa and tf_bundle.crc32c(b'\xff' * 32) == 0x62a8ab43
  assert tf_bundle.crc32c(bytes(range(32))) == 0x46dd794e and tf_bundle.crc32c(b'123456789') == 0xe3069283


def test_known_answer_framing(tmp_path):
  assert R.frame_record(b'123456789').hex() == '0900000000000000' '37f97139' '313233343536373839' 'e5b08ac7'
  assert R.frame_record(b'').hex() == '0000000000000000' '29039807' 'd8ea82a2'
  path = str(tmp_path / 'two')
  assert R.write_records(path, [b'123456789', b'']) == 2
  raw = open(path, 'rb').read()
  assert raw.hex() == '090000000000000037f97139313233343536373839e5b08ac7' '000000000000000029039807d8ea82a2'
  for src in (path, raw):
    f = R.RecordFile(src)
    assert len(f) == 2 and f.offsets.tolist() == [12, 37] and f.lengths.tolist() == [9, 0] and f.starts.tolist() == [0, 25]
    assert f.stored.tolist() == [0xc78ab0e5, 0xa282ead8] and f.stored.dtype == np.uint32
    assert f.payload(0).tobytes() == b'123456789' and f.payload(1).size == 0
  assert len(R.RecordFile(b'')) == 0


def test_known_answer_example():
  enc = R.encode_example({'image/class/label': np.array([7], dtype=np.int64)})
  assert enc == LABEL7 and len(enc) == 30
  assert R.frame_record(enc).hex() == '1e00000000000000' 'd9dc1232' + LABEL7.hex() + '339aed4e'
  got = R.parse_example(LABEL7)
  assert list(got) == ['image/class/label'] and got['image/class/label'].dtype == np.int64
  assert got['image/class/label'].tolist() == [7]


# ---- Example wire format ---------------------------------------------------------------------------------------------
def _f(fn, wt, body):
  key = tf_bundle._put_varint((fn << 3) | wt)
  return key + (tf_bundle._put_varint(len(body)) if wt == 2 else b'') + body


def _entry(name, feature):
  return _f(1, 2, _f(1, 2, name.encode()) + _f(2, 2, feature))


def test_round_trip_of_all_three_kinds():
  feats = {'image/encoded': [b'\xff\xd8abc', b'', b'\x00' * 300],
           'image/logit': np.array([0.0, -1.5, 3.25e10, np.float32(1e-40)], dtype=np.float32),
           'image/class/label': np.array([-1, 0, 1, 127, 128, 2 ** 63 - 1, -2 ** 63, -300], dtype=np.int64),
           'empty/bytes': [], 'empty/float': np.zeros(0, np.float32), 'empty/int': np.zeros(0, np.int64), 'unset': None}
  got = R.parse_example(R.encode_example(feats))
  assert list(got) == list(feats)
  assert got['image/encoded'] == feats['image/encoded'] and got['empty/bytes'] == [] and got['unset'] is None
  for k in ('image/logit', 'image/class/label', 'empty/float', 'empty/int'):
    assert got[k].dtype == feats[k].dtype and got[k].tobytes() == feats[k].tobytes(), k
  # a negative value is a ten-byte varint
  neg = R.encode_example({'l': np.array([-1])})
  assert neg.endswith(b'\x0a\x0a' + b'\xff' * 9 + b'\x01')


def test_unpacked_lists_unknown_fields_and_duplicate_keys():
  v = tf_bundle._put_varint
  floats = _f(2, 2, _f(1, 5, struct.pack('<f', 1.5)) + _f(1, 2, struct.pack('<ff', 2.5, 3.5)) + _f(1, 5, struct.pack('<f', -4.0)))
  ints = _f(3, 2, _f(1, 0, v(5)) + _f(1, 2, v(6) + v(2 ** 64 - 2)) + _f(1, 0, v(2 ** 64 - 1)) + _f(9, 0, v(1)))
  byts = _f(1, 2, _f(1, 2, b'a') + _f(7, 2, b'skipped') + _f(1, 2, b'bc'))
  features = (_f(5, 0, v(77)) + _entry('f', floats) + _f(6, 1, b'\x00' * 8) + _entry('i', ints) + _entry('b', byts) +
              _entry('dup', _f(3, 2, _f(1, 2, v(1)))) + _entry('dup', _f(1, 2, _f(1, 2, b'last'))) + _f(7, 5, b'\x00' * 4))
  payload = _f(3, 2, b'unknown') + _f(1, 2, features) + _f(2, 0, v(3))
  got = R.parse_example(payload)
  assert got['f'].tolist() == [1.5, 2.5, 3.5, -4.0] and got['f'].dtype == np.float32
  assert got['i'].tolist() == [5, 6, -2, -1] and got['i'].dtype == np.int64
  assert got['b'] == [b'a', b'bc'] and got['dup'] == [b'last']
  assert list(got) == ['f', 'i', 'b', 'dup']
  # the last kind of a Feature wins, as protobuf's oneof does
  assert R.parse_example(_f(1, 2, _entry('k', _f(1, 2, _f(1, 2, b'x')) + _f(3, 2, _f(1, 2, v(9))))))['k'].tolist() == [9]
  # numpy views parse like bytes
  assert R.parse_example(np.frombuffer(payload, np.uint8))['b'] == [b'a', b'bc']


def test_malformed_examples_raise_value_error():
  v = tf_bundle._put_varint
  with pytest.raises(ValueError):
    R.parse_example(_f(1, 2, _entry('k', _f(3, 2, _f(1, 2, b'\xff' * 10 + b'\x01')))))       # eleven-byte varint
  with pytest.raises(ValueError):
    R.parse_example(_f(1, 2, _entry('k', _f(3, 2, _f(1, 2, b'\xff' * 9 + b'\x02')))))        # a 65th bit
  with pytest.raises(ValueError):
    R.parse_example(_f(1, 2, _entry('k', _f(2, 2, _f(1, 2, b'\x00' * 6)))))                  # a float and a half
  with pytest.raises(ValueError):
    R.parse_example(_f(1, 3, b''))                                                           # a group
  with pytest.raises(ValueError):
    R.parse_example(v((1 << 3) | 2) + v(2 ** 40) + b'xx')                                    # a length far past the payload
  with pytest.raises(ValueError):
    R.parse_example(np.zeros((2, 2), np.uint8))


def test_every_truncation_of_an_example_parses_or_raises_value_error():
  full = R.encode_example({'image/encoded': [b'\xff\xd8' + bytes(range(40))], 'image/filename': [b'n01.JPEG'],
                           'image/class/label': np.array([-3]), 'image/logit': np.arange(5, dtype=np.float32),
                           'image/object/bbox/xmin': np.array([0.25], np.float32)})
  assert R.parse_example(full)['image/class/label'].tolist() == [-3]
  raised = 0
  for n in range(len(full)):
    try:
      R.parse_example(full[:n])
    except ValueError:
      raised += 1
  assert raised >= len(full) - 2        # (the empty payload is a valid, empty Example)


# ---- RecordFile ------------------------------------------------------------------------------------------------------
def test_every_truncation_and_every_flipped_length_byte_raises():
  payloads = [b'123456789', b'', bytes(range(50))]
  raw = b''.join(R.frame_record(p) for p in payloads)
  whole = R.RecordFile(raw, name='shard-0')
  assert [whole.payload(i).tobytes() for i in range(3)] == payloads
  boundaries = {0: 0, 25: 1, 41: 2}        # a file that ends behind a record is a complete shorter file
  for n in range(len(raw)):
    if n in boundaries:
      assert len(R.RecordFile(raw[:n])) == boundaries[n]
      continue
    with pytest.raises(ValueError) as err:
      R.RecordFile(raw[:n], name='shard-0')
    start = max(s for s in boundaries if s <= n)
    assert 'shard-0' in str(err.value) and ('byte %d' % start) in str(err.value), n
  for start in whole.starts.tolist():
    for k in range(12):                    # the eight length bytes and the four bytes of their crc
      for bit in (0x01, 0x80):
        bad = bytearray(raw)
        bad[start + k] ^= bit
        with pytest.raises(ValueError) as err:
          R.RecordFile(bytes(bad), name='shard-0')
        assert 'shard-0' in str(err.value) and ('byte %d' % start) in str(err.value)


# ---- the reference's parsers -----------------------------------------------------------------------------------------
def test_parse_example_proto_defaults_and_bbox_order():
  enc, label, bbox, name, logit = R.parse_example_proto(b'')
  assert (enc, name) == (b'', b'') and label == -1 and label.dtype == np.int32
  assert bbox.shape == (1, 0, 4) and bbox.dtype == np.float32 and logit.shape == (0,) and logit.dtype == np.float32
  # a Feature with no kind set takes the default as a missing one does
  assert R.parse_example_proto(R.encode_example({'image/class/label': None, 'image/encoded': None}))[:2] == (b'', -1)
  ex = R.encode_example({'image/encoded': [b'JPEG'], 'image/filename': [b'a.JPEG'], 'image/class/label': np.array([2 ** 32 + 5]),
                         'image/object/bbox/xmin': np.array([0.1, 0.2], np.float32),
                         'image/object/bbox/ymin': np.array([0.3, 0.4], np.float32),
                         'image/object/bbox/xmax': np.array([0.5, 0.6], np.float32),
                         'image/object/bbox/ymax': np.array([0.7, 0.8], np.float32)})
  enc, label, bbox, name, logit = R.parse_example_proto(ex)
  assert (enc, name, int(label)) == (b'JPEG', b'a.JPEG', 5) and logit.size == 0          # tf.cast(int64 -> int32) wraps
  assert bbox.shape == (1, 2, 4)
  assert np.array_equal(bbox, np.array([[[0.3, 0.1, 0.7, 0.5], [0.4, 0.2, 0.8, 0.6]]], np.float32))   # (ymin, xmin, ymax, xmax)
  d = R.parse_example_proto(ex, ret_dict=True)
  assert d['image/encoded'] == b'JPEG' and d['image/object/bbox/ymax'].tolist() == bbox[0, :, 2].tolist()
  assert R.parse_example_proto(np.frombuffer(ex, np.uint8))[0] == b'JPEG'


@pytest.mark.parametrize('features', [
    {'image/class/label': np.array([1.0], np.float32)},               # wrong kind
    {'image/encoded': np.array([1])},
    {'image/class/label': np.array([1, 2])},                          # FixedLenFeature([]) with two values
    {'image/class/label': np.zeros(0, np.int64)},                     # ... with none
    {'image/encoded': [b'a', b'b']},
    {'image/logit': np.array([1])},                                   # VarLenFeature of the wrong kind
    {'image/object/bbox/xmin': np.array([0.1], np.float32)},          # coordinate lists of different lengths
])
def test_parse_single_example_semantics_raise(features):
  with pytest.raises(ValueError):
    R.parse_example_proto(R.encode_example(features))


def test_parse_record_sup_rows_are_split_labels_layout():
  C = 7
  logit = np.linspace(-2, 2, C).astype(np.float32)
  ex = R.encode_example({'image/encoded': [b'J'], 'image/class/label': np.array([3]), 'image/logit': logit,
                         'image/filename': [b'f']})
  plain = R.parse_record_sup(ex)
  assert plain['image'] == b'J' and plain['label'] == 3 and plain['label'].dtype == np.int32
  row = R.parse_record_sup(ex, return_logits=True, num_classes=C)['label']
  assert row.dtype == np.float32 and row.shape == (2 * C,)
  assert row[:C].tolist() == [0, 0, 0, 1, 0, 0, 0] and np.array_equal(row[C:], logit)
  # the layout Trainer.split_labels cuts: [:, :C] the hard targets, [:, C:] the teacher's logits
  from assembled_cnn_amd.train import Trainer

  class P(object):
    num_classes, kd_temp = C, 1.0
  stub = type('T', (), {'p': P()})()
  hard, teacher = Trainer.split_labels(stub, torch.from_numpy(np.stack([row, row])))
  assert hard.shape == teacher.shape == (2, C) and hard[0].tolist() == row[:C].tolist() and np.array_equal(teacher[1].numpy(), logit)
  with pytest.raises(ValueError):
    R.parse_record_sup(ex, return_logits=True, num_classes=C + 1)      # a wrong logit count
  with pytest.raises(ValueError):
    R.parse_record_sup(R.encode_example({'image/class/label': np.array([3])}), return_logits=True, num_classes=C)
  # tf.one_hot of the default label -1 is a row of zeros
  none = R.parse_record_sup(R.encode_example({'image/logit': logit}), return_logits=True, num_classes=C)['label']
  assert not none[:C].any()
  # parse_record: the reference's assertion, and the filename on request
  with pytest.raises(AssertionError):
    R.parse_record(ex, return_logits=True, num_classes=C)
  assert R.parse_record(ex, return_filename=True) == (b'J', 3, b'f') and R.parse_record(ex) == (b'J', 3)
  big = R.encode_example({'image/class/label': np.array([1000]), 'image/logit': np.zeros(1001, np.float32)})
  img, lab = R.parse_record(big, return_logits=True)
  assert lab.shape == (2002,) and lab[1000] == 1.0 and lab.sum() == 1.0


# ---- the dataset -----------------------------------------------------------------------------------------------------
def _example(tag: int, shard: str, logits: int = 0):
  feats = {'image/encoded': [b'\xff\xd8' + bytes([tag]) * (tag + 1)], 'image/filename': [('%s/%d' % (shard, tag)).encode()],
           'image/class/label': np.array([tag])}
  if logits:
    feats['image/logit'] = np.full(logits, tag, np.float32)
  return R.encode_example(feats)


@pytest.fixture
def shards(tmp_path):
  """three shards of unequal length, labels 0..8: a = 0, 1; b = 2..5; c = 6..8"""
  out = []
  for name, tags in (('a', (0, 1)), ('b', (2, 3, 4, 5)), ('c', (6, 7, 8))):
    path = str(tmp_path / ('train-%s' % name))
    R.write_records(path, [_example(t, name, logits=4) for t in tags])
    out.append(path)
  return out


def _labels(ds):
  return [int(l) for b in ds for l in b.labels]


def test_evaluation_order_is_the_interleave_order(shards):
  ds = R.RecordDataset(shards, False, 4, 1, cycle_length=2, verify='host')
  batches = list(ds)
  # slots (a, b): a0 b0 a1 b1; a is exhausted and its slot takes c: c0 b2 c1 b3; b is exhausted, no file is left: c2
  assert [b.labels.tolist() for b in batches] == [[0, 2, 1, 3], [6, 4, 7, 5], [8]]
  assert batches[0].labels.dtype == torch.int32
  assert batches[1].filenames == [b'c/6', b'b/4', b'c/7', b'b/5']
  assert [e.tobytes() for e in batches[2].encoded] == [b'\xff\xd8' + b'\x08' * 9]
  assert batches[2].encoded[0].dtype == np.uint8 and batches[2].encoded[0].base is not None       # a view into the mapping
  f = R.RecordFile(shards[1])
  assert batches[0].origins == [(shards[0], 0), (shards[1], 0), (shards[0], int(R.RecordFile(shards[0]).starts[1])),
                                (shards[1], int(f.starts[1]))]
  # cycle_length 1 reads the files one after the other; a cycle longer than the file list changes nothing else
  assert _labels(R.RecordDataset(shards, False, 4, 1, cycle_length=1, verify='none')) == list(range(9))
  assert _labels(R.RecordDataset(shards, False, 4, 1, cycle_length=20, verify='none')) == [0, 2, 6, 1, 3, 7, 4, 8, 5]
  # evaluation repeats in the same order
  assert _labels(R.RecordDataset(shards, False, 9, 1, cycle_length=2, num_epochs=2, verify='none')) == [0, 2, 1, 3, 6, 4, 7, 5, 8] * 2


def test_training_epochs_are_permutations_that_do_not_mix(shards):
  for seed in (0, 1, 2):
    got = _labels(R.RecordDataset(shards, True, 4, 5, cycle_length=2, num_epochs=3, seed=seed, verify='none'))
    assert len(got) == 27
    epochs = [got[9 * e:9 * e + 9] for e in range(3)]
    assert all(sorted(ep) == list(range(9)) for ep in epochs)        # every record once per epoch, none across a boundary
  a = _labels(R.RecordDataset(shards, True, 4, 5, cycle_length=2, num_epochs=3, seed=7, verify='none'))
  b = _labels(R.RecordDataset(shards, True, 4, 5, cycle_length=2, num_epochs=3, seed=7, verify='none'))
  c = _labels(R.RecordDataset(shards, True, 4, 5, cycle_length=2, num_epochs=3, seed=8, verify='none'))
  assert a == b and a != c
  assert a[:9] != a[9:18] or a[9:18] != a[18:]                        # files and buffer are drawn anew every epoch
  assert a[:9] != [0, 2, 1, 3, 6, 4, 7, 5, 8]


def test_drop_remainder_and_batches_across_epochs(shards):
  keep = list(R.RecordDataset(shards, True, 4, 3, num_epochs=2, seed=1, verify='none'))
  drop = list(R.RecordDataset(shards, True, 4, 3, num_epochs=2, seed=1, drop_remainder=True, verify='none'))
  assert [len(b.encoded) for b in keep] == [4, 4, 4, 4, 2] and [len(b.encoded) for b in drop] == [4, 4, 4, 4]
  assert all(torch.equal(x.labels, y.labels) for x, y in zip(keep, drop))
  assert list(R.RecordDataset(shards, False, 4, 1, num_epochs=0, verify='none')) == []
  with pytest.raises(ValueError):
    R.RecordDataset(shards, False, 4, 1, verify='gpu')


def test_kd_rows_and_a_wrong_logit_count(shards):
  ds = R.RecordDataset(shards, False, 3, 1, cycle_length=1, return_logits=True, num_classes=4, verify='none')
  first = next(iter(ds))
  assert first.labels.dtype == torch.float32 and first.labels.shape == (3, 8)
  assert first.labels[1].tolist() == [0, 1, 0, 0, 1, 1, 1, 1] and first.labels[2].tolist() == [0, 0, 1, 0, 2, 2, 2, 2]
  with pytest.raises(ValueError) as err:
    next(iter(R.RecordDataset(shards, False, 3, 1, cycle_length=1, return_logits=True, num_classes=5, verify='none')))
  assert shards[0] in str(err.value) and 'byte 0' in str(err.value)


def test_mixup_type_1_doubles_batch_and_epochs(tmp_path):
  assert R.batch_size_and_epochs(256, 90, 1, True) == (512, 180)
  assert R.batch_size_and_epochs(256, 90, 1, False) == (256, 90) and R.batch_size_and_epochs(256, 90, 2, True) == (256, 90)
  assert R.batch_size_and_epochs(256, 90, 1, True, num_gpus=8) == (64, 180)
  with pytest.raises(ValueError):
    R.batch_size_and_epochs(100, 1, 0, True, num_gpus=8)
  for n in ('train-00001-of-00002', 'train-00000-of-00002', 'validation-00000-of-00001', 'other'):
    open(str(tmp_path / n), 'wb').close()
  d = str(tmp_path)
  assert [os.path.basename(p) for p in R.get_filenames(True, d)] == ['train-00000-of-00002', 'train-00001-of-00002']
  assert [os.path.basename(p) for p in R.get_filenames(False, d)] == ['validation-00000-of-00001']
  assert [os.path.basename(p) for p in R.get_filenames(False, d, val_regex='o*')] == ['other']
  assert len(list(R.RecordDataset(R.get_filenames(True, d), True, 4, 4, verify='none'))) == 0      # empty shards, no batch


def _flip_payload_byte(path, record):
  """one bit of the record's encoded image, on disk; returns the record's byte position"""
  f = R.RecordFile(path)
  pos = int(f.offsets[record]) + f.payload(record).tobytes().index(b'\xff\xd8') + 3
  start = int(f.starts[record])
  del f
  with open(path, 'r+b') as fh:
    fh.seek(pos)
    b = fh.read(1)
    fh.seek(pos)
    fh.write(bytes([b[0] ^ 0x10]))
  return start


def test_host_verification_names_the_file_and_position(shards):
  assert len(list(R.RecordDataset(shards, False, 2, 1, cycle_length=2, verify='host'))) == 5
  start = _flip_payload_byte(shards[1], 2)         # b2 is the sixth record in evaluation order: the third batch of two
  it = iter(R.RecordDataset(shards, False, 2, 1, cycle_length=2, verify='host'))
  assert next(it).labels.tolist() == [0, 2] and next(it).labels.tolist() == [1, 3]
  with pytest.raises(ValueError) as err:
    next(it)
  assert shards[1] in str(err.value) and ('byte %d' % start) in str(err.value) and 'checksum' in str(err.value)


def test_device_verification_path_on_the_double(shards, spans_double):
  ds = R.RecordDataset(shards, False, 4, 1, cycle_length=2, verify='device', device='cpu')
  assert [b.labels.tolist() for b in ds] == [[0, 2, 1, 3], [6, 4, 7, 5], [8]]
  assert spans_double.launches == 3                    # one launch per batch
  start = _flip_payload_byte(shards[2], 1)          # c1: in the second batch
  it = iter(R.RecordDataset(shards, False, 4, 1, cycle_length=2, verify='device', device='cpu'))
  assert next(it).labels.tolist() == [0, 2, 1, 3]
  with pytest.raises(ValueError) as err:
    next(it)
  assert shards[2] in str(err.value) and ('byte %d' % start) in str(err.value) and 'checksum' in str(err.value)
  # without verification the damaged record goes through (its encoded bytes were hit, not its structure)
  assert len(list(R.RecordDataset(shards, False, 4, 1, cycle_length=2, verify='none'))) == 3


def test_ops_wrapper_on_the_double(spans_double):
  from assembled_cnn_amd import lib, ops
  data = np.random.default_rng(5).integers(0, 256, 1000, dtype=np.uint8)
  spans = np.zeros(4, dtype=R.SPAN_DTYPE)
  spans['offset'], spans['length'] = [0, 3, 999, 990], [1000, 0, 1, 11]
  spans['flags'], spans['expect_masked'][0] = [1, 0, 1, 0], tf_bundle.mask_crc(tf_bundle.crc32c(data))
  crc, status = ops.crc32c_spans(torch.from_numpy(data), torch.from_numpy(spans.view(np.uint8)), 4)
  assert crc.dtype == status.dtype == torch.int32 and crc.shape == status.shape == (4,)
  assert (crc.numpy().view(np.uint32)[:3].tolist() == [tf_bundle.crc32c(data), 0, tf_bundle.crc32c(data[999:])])
  assert status.tolist() == [0, 0, lib.SPAN_EMISMATCH, lib.SPAN_EDESC] and int(crc[3]) == 0
  crc, status = ops.crc32c_spans(torch.from_numpy(data), torch.zeros(0, dtype=torch.uint8), 0)
  assert crc.shape == status.shape == (0,) and spans_double.launches == 1
  with pytest.raises(ValueError):
    ops.crc32c_spans(torch.from_numpy(data), torch.from_numpy(spans.view(np.uint8)), 3)


# ---- the real library, no GPU ----------------------------------------------------------------------------------------
def test_crc32c_spans_argument_checks_need_no_gpu():
  import __graft_entry__
  __graft_entry__.build()
  from assembled_cnn_amd import lib
  L = lib.load()
  assert ctypes.sizeof(lib.SpanDesc) == 24 and lib.SpanDesc.expect_masked.offset == 16 and lib.SpanDesc.flags.offset == 20
  assert 'asm_crc32c_spans' in lib.SIGNATURES and lib.ABI_VERSION == 11 and L.asm_abi_version() == 11
  fake = ctypes.c_void_p(0x1000)
  for k in range(4):
    args = [fake, 64, fake, 1, fake, fake, None]
    args[(0, 2, 4, 5)[k]] = None
    assert L.asm_crc32c_spans(*args) == lib.ASM_EINVAL and b'null' in L.asm_last_error()
  assert L.asm_crc32c_spans(fake, 64, fake, -1, fake, fake, None) == lib.ASM_EINVAL
  assert L.asm_crc32c_spans(fake, -1, fake, 1, fake, fake, None) == lib.ASM_EINVAL
  assert L.asm_crc32c_spans(fake, 1 << 40, fake, 1, fake, fake, None) == lib.ASM_EINVAL
  before = L.asm_launch_count()
  assert L.asm_crc32c_spans(fake, 64, fake, 0, fake, fake, None) == lib.ASM_OK          # nothing to do, nothing launched
  assert L.asm_launch_count() == before
  hdr = open(os.path.join(ROOT, 'include', 'asm_hip.h')).read()
  body = hdr[hdr.index('typedef struct asm_span_desc {'):hdr.index('} asm_span_desc;')]
  assert 'int64_t offset, length;' in body and 'uint32_t expect_masked;' in body and 'uint32_t flags;' in body
  assert '#define ASM_SPAN_EDESC 1' in hdr and '#define ASM_SPAN_EMISMATCH 2' in hdr
  assert (lib.SPAN_EDESC, lib.SPAN_EMISMATCH) == (1, 2)
