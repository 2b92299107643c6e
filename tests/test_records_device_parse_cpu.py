"""RecordDataset(parse=...) without a GPU: rows made from records._proto (proto_row: what asm_example_parse writes for a
class-0 record) go through the assembly function of parse='device' and must give the batch of parse='host' field for
field, on shards written from the JPEG fixtures; the argument check; the default."""
import inspect
import os

import numpy as np
import pytest
import torch

from assembled_cnn_amd import lib, records as R
from tests import example_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 4


@pytest.fixture
def shards(tmp_path):
  """eleven fixture files over two shards: label, filename, four logits, i % 3 boxes; record 4 has no filename and record 7
  its logits as unpacked values"""
  fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_fixtures.npz'))
  files = [(str(n), fx['file_' + str(n)].tobytes()) for n in fx['names']][:11]
  r = np.random.default_rng(5)
  payloads = []
  for i, (name, data) in enumerate(files):
    feats = {ec.ENC: ec.bytes_feat([data]), ec.NAME: ec.bytes_feat([name.encode()]), ec.LABEL: ec.int_feat([i - 1]),
             ec.LOGIT: ec.float_feat(r.normal(size=C).astype(np.float32), 'fixed' if i == 7 else 'packed')}
    feats.update({k: ec.float_feat(r.random(i % 3).astype(np.float32)) for k in R._BBOX})
    if i == 4:
      del feats[ec.NAME]
    payloads.append(ec.build(feats))
  paths = []
  for s in range(2):
    paths.append(str(tmp_path / ('validation-%05d-of-00002' % s)))
    R.write_records(paths[-1], payloads[s::2])
  return paths


def _same(a, b):
  assert [x.tobytes() for x in a.encoded] == [x.tobytes() for x in b.encoded]
  assert all(x.dtype == np.uint8 for x in a.encoded)
  assert a.labels.dtype == b.labels.dtype and a.labels.shape == b.labels.shape
  assert a.labels.numpy().tobytes() == b.labels.numpy().tobytes()
  assert a.filenames == b.filenames and all(type(x) is bytes for x in a.filenames) and a.origins == b.origins
  assert (a.payloads is None) == (b.payloads is None)
  if a.payloads is not None:
    assert a.payloads[1].dtype == b.payloads[1].dtype == np.int64 and a.payloads[1].tolist() == b.payloads[1].tolist()
    for p, e in ((a.payloads, a.encoded), (b.payloads, b.encoded)):      # (the bytes between two slots are nobody's)
      assert [p[0][o:o + n].numpy().tobytes() for o, n in p[1].tolist()] == [x.tobytes() for x in e]


@pytest.mark.parametrize('return_logits,keep', [(False, False), (True, False), (False, True), (True, True)])
def test_rows_from_the_host_parser_assemble_into_the_host_batch(shards, return_logits, keep):
  kw = dict(cycle_length=2, return_logits=return_logits, num_classes=C, verify='none', device='cpu', keep_payloads=keep)
  ds = R.RecordDataset(shards, False, 4, 1, **kw)
  recs = list(ds.records())
  sizes, first = [], []
  for k, b in enumerate(R.RecordDataset(shards, False, 4, 1, **kw)):     # (a batch's payload buffer lives until the next one)
    sizes.append(len(b.encoded))
    first += b.payloads[1][:, 0].tolist() if keep else []
    part = recs[4 * k:4 * k + 4]
    up = ds._upload(part) if keep else None
    rows = np.zeros(len(part), R.ROW_DTYPE)
    for j, (f, i) in enumerate(part):
      rows[j] = R.proto_row(R._buffer(f.payload(i)), int(up[1][j]) if keep else 0)[0]
    assert rows.dtype.itemsize == 48 and (rows['cls'] == 0).all()
    _same(ds.assemble(part, rows, up), b)
    # a row of another class is parsed again by the host: the same batch
    rows['cls'][1::2] = lib.EXAMPLE_PFORM
    rows['enc_length'][1::2] = -7
    _same(ds.assemble(part, rows, up), b)
  assert sizes == [4, 4, 3]
  if keep:
    assert min(first) > 0 and any(x % 16 for x in first) and len(set(first[:4])) == 4


def test_errors_keep_their_text(shards, tmp_path):
  with pytest.raises(ValueError, match=r"parse must be one of \('host', 'device'\), got 'nonsense'"):
    R.RecordDataset(shards, False, 4, 1, parse='nonsense')
  assert R.PARSE_MODES == ('host', 'device')
  texts = []
  for mode in ('host', 'assemble'):
    ds = R.RecordDataset(shards, False, 4, 1, cycle_length=2, return_logits=True, num_classes=C + 1, verify='none', device='cpu')
    with pytest.raises(ValueError) as err:
      if mode == 'host':
        next(iter(ds))
      else:
        part = list(ds.records())[:4]
        ds.assemble(part, np.array([R.proto_row(R._buffer(f.payload(i)))[0] for f, i in part]))
    texts.append(str(err.value))
  assert texts[0] == texts[1] and 'image/logit holds 4 values, num_classes is 5' in texts[0] and 'record at byte 0' in texts[0]
  # a truncated proto behind a valid checksum
  f = R.RecordFile(shards[0])
  bad = str(tmp_path / 'bad')
  R.write_records(bad, [f.payload(0).tobytes(), f.payload(1).tobytes()[:-3]])
  ds = R.RecordDataset([bad], False, 2, 1, verify='host', device='cpu')
  with pytest.raises(ValueError) as host:
    next(iter(ds))
  rows = np.zeros(2, R.ROW_DTYPE)
  rows[0] = R.proto_row(R._buffer(f.payload(0)))[0]
  rows['cls'][1] = lib.EXAMPLE_PMALFORMED
  with pytest.raises(ValueError) as dev:
    ds.assemble(list(ds.records()), rows)
  assert str(dev.value) == str(host.value) and 'record at byte' in str(host.value)


def test_binding_constants_and_row_equal_the_header():
  """lib.py's copies of the window size, the class and status bits and the row's fields against include/asm_hip.h"""
  import re
  hdr = open(os.path.join(ROOT, 'include', 'asm_hip.h')).read()
  define = dict((k, int(v)) for k, v in re.findall(r'^#define ASM_EXAMPLE_(\w+) (\d+)\b', hdr, re.M))
  assert define == {'WINDOW': lib.EXAMPLE_WINDOW, 'PSPAN': lib.EXAMPLE_PSPAN, 'PMALFORMED': lib.EXAMPLE_PMALFORMED,
                    'PSCHEMA': lib.EXAMPLE_PSCHEMA, 'PFORM': lib.EXAMPLE_PFORM, 'LSKIP': lib.EXAMPLE_LSKIP,
                    'LRANGE': lib.EXAMPLE_LRANGE}
  assert ec.WINDOW == define['WINDOW'] and define['WINDOW'] % 16 == 0
  body = hdr[hdr.index('typedef struct asm_example_row {'):hdr.index('} asm_example_row;')]
  fields = []
  for ctype, names in re.findall(r'^\s+(int32_t|int64_t) ([\w, ]+);', body, re.M):
    fields += [(n.strip(), {'int32_t': 4, 'int64_t': 8}[ctype]) for n in names.split(',')]
  assert fields == [(n, R.ROW_DTYPE.fields[n][0].itemsize) for n, _ in lib.ExampleRow._fields_]
  assert [R.ROW_DTYPE.fields[n][1] for n, _ in fields] == [0, 4, 8, 16, 24, 32, 36, 40, 44] and R.ROW_DTYPE.itemsize == 48
  assert '/* 48 bytes */' in hdr[hdr.index('} asm_example_row;'):][:80]


def test_the_default_is_the_host_parser(shards):
  assert inspect.signature(R.RecordDataset.__init__).parameters['parse'].default == 'host'
  a = list(R.RecordDataset(shards, False, 4, 1, cycle_length=2, verify='none', device='cpu'))
  b = list(R.RecordDataset(shards, False, 4, 1, cycle_length=2, verify='none', device='cpu', parse='host'))
  assert len(a) == len(b) == 3
  for x, y in zip(a, b):
    _same(x, y)
  assert a[0].labels.dtype == torch.int32 and a[0].labels.tolist() == [-1, 0, 1, 2] and a[1].filenames[0] == b''
  assert R.Batch._fields == ('encoded', 'labels', 'filenames', 'origins', 'payloads')
