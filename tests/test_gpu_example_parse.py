"""asm_example_parse / asm_example_label_rows on the device (csrc/records.hip, csrc/example_parse.h) against records._proto
and records._kd_label -- the whole case set of tests/example_cases.py in one launch, spans at all 16 alignments, guard bands
around every output -- and RecordDataset(parse='device') against parse='host' end to end."""
import os

import numpy as np
import pytest
import torch

from tests import example_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY, GUARD = 0xa5, 64
NANS = (0x7fc12345, 0xffc00001, 0x7f800001)
_STATE = {}


@pytest.fixture(scope='module')
def product():
  import __graft_entry__
  __graft_entry__.build()
  from assembled_cnn_amd import lib, ops
  ops.set_library(None, is_double=False)
  return lib.load()


def table(rows):
  from assembled_cnn_amd import records
  t = np.zeros(len(rows), dtype=records.SPAN_DTYPE)
  t['offset'], t['length'] = [r[0] for r in rows], [r[1] for r in rows]
  t['flags'], t['expect_masked'] = 0xffffffff, 0x12345678            # both are ignored
  return t


def guarded(nbytes):
  return torch.full((GUARD + nbytes + GUARD,), CANARY, dtype=torch.uint8, device='cuda')


def inside(t, nbytes):
  h = t.cpu().numpy()
  assert (h[:GUARD] == CANARY).all() and (h[GUARD + nbytes:] == CANARY).all(), 'a write outside the output array'
  return h[GUARD:GUARD + nbytes].copy()


def parse(L, dev, spans, buf_bytes=None):
  """one launch through the C ABI with guard bands around the rows -> ROW_DTYPE [n]"""
  n = len(spans)
  sd = torch.from_numpy(table(spans).view(np.uint8)).cuda()
  rows = guarded(48 * n)
  rc = L.asm_example_parse(dev.data_ptr(), dev.numel() if buf_bytes is None else buf_bytes, sd.data_ptr(), n,
                           rows.data_ptr() + GUARD, torch.cuda.current_stream().cuda_stream)
  assert rc == 0, L.asm_last_error()
  torch.cuda.synchronize()
  return inside(rows, 48 * n).view(cases.ROW_DTYPE)


def layout(L):
  """every case in one buffer of seeded bytes -- the cases of the must list that are not made in bulk at all 16 start
  alignments, the others at one each in rotation -- parsed by one launch: once"""
  if _STATE:
    return _STATE
  every, want = cases.all_cases(), cases.host_results()
  places, at = [], 64                                     # (case index, offset)
  for k, (label, payload, expect) in enumerate(every):
    bulk = expect != cases.MUST or 'filler of' in label or len(payload) > 2048
    for a in ([k % 16] if bulk else range(16)):
      at = (at + 15) // 16 * 16 + a
      places.append((k, at))
      at += len(payload) + 3                              # (+ 3: the byte behind a span is never the next one's first)
  tail = at + 64                                          # 8 KB of seeded bytes behind the cases, NaN patterns planted
  host = np.random.default_rng(20241106).integers(0, 256, size=tail + 8192, dtype=np.uint8)
  for k, o in places:
    host[o:o + len(every[k][1])] = np.frombuffer(every[k][1], np.uint8)
  host[tail + 21:tail + 33] = np.frombuffer(np.array(NANS, '<u4').tobytes(), np.uint8)
  dev = torch.from_numpy(host).cuda()
  rows = parse(L, dev, [(o, len(every[k][1])) for k, o in places])
  _STATE.update(tail=tail, host=host, dev=dev, places=places, rows=rows, every=every, want=want)
  return _STATE


def test_every_case_keeps_the_contract_in_one_launch(product):
  st = layout(product)
  every, want = st['every'], st['want']
  assert len(st['places']) >= len(every) + 15 * 90
  aligned = {}
  for (k, o), row in zip(st['places'], st['rows']):
    cases.check_row('%s at %d' % (every[k][0], o % 16), every[k][1], every[k][2], want[k], row, base=o)
    aligned.setdefault(k, set()).add(o % 16)
  assert sum(len(a) == 16 for a in aligned.values()) >= 90 and {o % 16 for _, o in st['places']} == set(range(16))
  assert sum(int(r['cls']) == 0 for r in st['rows']) > 2500


def test_spans_outside_the_buffer_and_refused_arguments(product):
  from assembled_cnn_amd import lib
  L = product
  st = layout(L)
  dev, size = st['dev'], st['dev'].numel()
  i64 = np.iinfo(np.int64)
  k, o = st['places'][0]
  good = (o, len(st['every'][k][1]))
  spans = [good, (-1, 16), (16, -1), (size - 8, 9), (size + 1, 0), (i64.max, 1), (i64.max - 2, i64.max), (1, i64.max),
           (i64.min, i64.min), good, (size, 0)]
  rows = parse(L, dev, spans)
  assert rows['cls'].tolist() == [0] + [lib.EXAMPLE_PSPAN] * 8 + [0, 0]
  zero = np.zeros((), cases.ROW_DTYPE)
  zero['cls'] = lib.EXAMPLE_PSPAN
  assert all(r == zero for r in rows[1:9])
  assert rows[0] == rows[9] == st['rows'][0]
  empty = np.zeros((), cases.ROW_DTYPE)                   # the empty span at the buffer's end: an Example with no features
  empty['label'], empty['enc_offset'], empty['name_offset'], empty['logit_offset'] = -1, size, size, size
  assert rows[10] == empty
  # the range is buf_bytes, not the allocation
  rows = parse(L, dev, [good, (good[0], good[1] + 1)], buf_bytes=good[0] + good[1])
  assert rows['cls'].tolist() == [0, lib.EXAMPLE_PSPAN]
  # a span of 2^31 bytes or more is left to the host before a byte of it is read (buf_bytes says the buffer is that long)
  rows = parse(L, dev, [(0, 2 ** 31), (16, 2 ** 40 - 17), (2 ** 31, 0)], buf_bytes=2 ** 40 - 1)
  assert rows['cls'].tolist() == [lib.EXAMPLE_PFORM, lib.EXAMPLE_PFORM, 0]
  # refused before any launch; n == 0 launches nothing
  sd = torch.from_numpy(table([good]).view(np.uint8)).cuda()
  out, status = guarded(48), guarded(4)
  stream = torch.cuda.current_stream().cuda_stream
  count = L.asm_launch_count()
  b, s, r = dev.data_ptr(), sd.data_ptr(), out.data_ptr() + GUARD
  assert L.asm_example_parse(b, size, s, 0, r, stream) == lib.ASM_OK
  for args in ((None, size, s, 1, r), (b, size, None, 1, r), (b, size, s, 1, None), (b, size, s, -1, r), (b, -1, s, 1, r),
               (b, 1 << 40, s, 1, r)):
    assert L.asm_example_parse(*args, stream) == lib.ASM_EINVAL, args
  lab, stt = guarded(4 * 16), status.data_ptr() + GUARD
  o = lab.data_ptr() + GUARD
  assert L.asm_example_label_rows(b, size, r, 0, 5, o, 10, stt, stream) == lib.ASM_OK
  for args in ((None, size, r, 1, 5, o, 10, stt), (b, size, None, 1, 5, o, 10, stt), (b, size, r, 1, 5, None, 10, stt),
               (b, size, r, 1, 5, o, 10, None), (b, size, r, -1, 5, o, 10, stt), (b, size, r, 1, 0, o, 10, stt),
               (b, size, r, 1, -3, o, 10, stt), (b, size, r, 1, 5, o, 9, stt), (b, -1, r, 1, 5, o, 10, stt),
               (b, 1 << 40, r, 1, 5, o, 10, stt)):
    assert L.asm_example_label_rows(*args, stream) == lib.ASM_EINVAL, args
  assert L.asm_launch_count() == count
  torch.cuda.synchronize()
  assert (out.cpu().numpy() == CANARY).all() and (lab.cpu().numpy() == CANARY).all() and (status.cpu().numpy() == CANARY).all()


def label_rows(L, dev, rows, C, ld, buf_bytes=None):
  """one launch with `out` and `status` pre-filled and guard-banded -> (uint32 [n, ld], int32 [n])"""
  n = len(rows)
  rd = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8)).cuda()
  out, status = guarded(4 * n * ld), guarded(4 * n)
  rc = L.asm_example_label_rows(dev.data_ptr(), dev.numel() if buf_bytes is None else buf_bytes, rd.data_ptr(), n, C,
                                out.data_ptr() + GUARD, ld, status.data_ptr() + GUARD, torch.cuda.current_stream().cuda_stream)
  assert rc == 0, L.asm_last_error()
  torch.cuda.synchronize()
  return inside(out, 4 * n * ld).view(np.uint32).reshape(n, ld), inside(status, 4 * n).view(np.int32)


@pytest.mark.parametrize('extra', [0, 3])
def test_label_rows_of_the_case_set(product, extra):
  from assembled_cnn_amd import lib
  st = layout(product)
  C = cases.NUM_CLASSES
  got, status = label_rows(product, st['dev'], st['rows'], C, 2 * C + extra)
  blank = 0x01010101 * CANARY
  written, labels = 0, set()
  for (k, _), row, g, s in zip(st['places'], st['rows'], got, status):
    kd = cases.kd_row(st['want'][k]) if row['cls'] == 0 else None
    assert (g[2 * C:] == blank).all()
    if kd is None:
      assert s == lib.EXAMPLE_LSKIP and (g == blank).all(), st['every'][k][0]
    else:
      assert s == 0 and g[:2 * C].tolist() == kd.tolist(), st['every'][k][0]
      written += 1
      labels.add(int(row['label']))
  assert written > 1500 and {-1, 0, C - 1, C} <= labels


def test_label_rows_of_1001_classes_and_the_range_check(product):
  from assembled_cnn_amd import lib, records
  st = layout(product)
  host, size, tail = st['host'], st['host'].size, st['tail']
  C = 1001
  i64 = np.iinfo(np.int64)
  rows = np.zeros(14, cases.ROW_DTYPE)
  rows['logit_count'] = C
  spec = [(tail + 1, -1), (tail + 2, 0), (tail + 19, 1000), (tail + 15, C), (size - 4 * C, 500), (64, -2 ** 31)]    # (offset, label): written
  for j, (o, lab) in enumerate(spec):
    rows[j]['logit_offset'], rows[j]['label'] = o, lab
  rows[6]['cls'], rows[6]['logit_offset'] = lib.EXAMPLE_PFORM, 64
  rows[7]['logit_count'], rows[7]['logit_offset'] = C - 1, 64
  rows[8]['logit_count'], rows[8]['logit_offset'] = 0, 64
  for j, o in zip(range(9, 14), (-1, size - 4 * C + 1, size, i64.max, i64.min)):
    rows[j]['logit_offset'] = o
  want_status = [0] * 6 + [lib.EXAMPLE_LSKIP] * 3 + [lib.EXAMPLE_LRANGE] * 5
  blank = 0x01010101 * CANARY
  for ld in (2 * C, 2 * C + 6):
    got, status = label_rows(product, st['dev'], rows, C, ld)
    assert status.tolist() == want_status
    for j, (o, lab) in enumerate(spec):
      logit = np.frombuffer(host[o:o + 4 * C].tobytes(), '<f4')
      assert got[j, :2 * C].tolist() == records._kd_label(np.int32(lab), logit, C).view(np.uint32).tolist()
      assert (got[j, 2 * C:] == blank).all()
    assert (got[6:] == blank).all()
    assert set(NANS) <= set(got[0, C:2 * C].tolist())      # (offset tail + 1: the planted NaN patterns are values 5..7)
  # the range is buf_bytes, not the allocation
  got, status = label_rows(product, st['dev'], rows[:2], C, 2 * C, buf_bytes=tail + 1 + 4 * C)
  assert status.tolist() == [0, lib.EXAMPLE_LRANGE] and (got[1] == blank).all()
  # ops.example_parse / ops.example_label_rows: the same launches behind the tensor wrappers
  from assembled_cnn_amd import ops
  places = st['places'][:300]
  sd = torch.from_numpy(table([(o, len(st['every'][k][1])) for k, o in places]).view(np.uint8)).cuda()
  rd = ops.example_parse(st['dev'], sd, len(places))
  assert rd.cpu().numpy().view(cases.ROW_DTYPE).tolist() == st['rows'][:300].tolist()
  out = torch.full((300, 16), 7.0, device='cuda')
  o2, s2 = ops.example_label_rows(st['dev'], rd, 300, cases.NUM_CLASSES, out=out[:, :12])
  ref, sref = label_rows(product, st['dev'], st['rows'][:300], cases.NUM_CLASSES, 10)
  done = sref == 0
  assert s2.cpu().numpy().tolist() == sref.tolist() and done.sum() > 100 and (~done).sum() > 2
  assert out.cpu().numpy().view(np.uint32)[done, :10].tolist() == ref[done].tolist()
  assert (out.cpu().numpy()[~done] == 7.0).all() and (out.cpu().numpy()[:, 10:] == 7.0).all()


# ---- end to end --------------------------------------------------------------------------------------------------------
C4 = 4


@pytest.fixture
def shards(tmp_path):
  """eleven device-decodable fixtures over two shards: label, filename, four logits, i % 3 boxes; record 4 has no filename,
  record 7 its logits as unpacked values (a form left to the host)"""
  from assembled_cnn_amd import records
  fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_fixtures.npz'))
  files = [(str(n), fx['file_' + str(n)].tobytes()) for n in fx['names'] if str(fx['kind_' + str(n)]) == 'device'][:11]
  r = np.random.default_rng(5)
  payloads = []
  for i, (name, data) in enumerate(files):
    feats = {cases.ENC: cases.bytes_feat([data]), cases.NAME: cases.bytes_feat([name.encode()]),
             cases.LABEL: cases.int_feat([i - 1]),
             cases.LOGIT: cases.float_feat(r.normal(size=C4).astype(np.float32), 'fixed' if i == 7 else 'packed')}
    feats.update({k: cases.float_feat(r.random(i % 3).astype(np.float32)) for k in cases.BBOX})
    if i == 4:
      del feats[cases.NAME]
    payloads.append(cases.build(feats))
  paths = []
  for s in range(2):
    paths.append(str(tmp_path / ('validation-%05d-of-00002' % s)))
    records.write_records(paths[-1], payloads[s::2])
  return paths, payloads


@pytest.mark.parametrize('batch', [5, 3])
@pytest.mark.parametrize('return_logits,keep', [(False, False), (True, False), (True, True)])
def test_dataset_device_parse_equals_host_parse(product, shards, batch, return_logits, keep):
  from assembled_cnn_amd import input_pipeline as ip, records
  paths, _ = shards
  kw = dict(cycle_length=2, return_logits=return_logits, num_classes=C4, verify='device', device='cuda', keep_payloads=keep)
  host = iter(records.RecordDataset(paths, False, batch, 1, **kw))
  seen = 0
  for d in records.RecordDataset(paths, False, batch, 1, parse='device', **kw):
    h = next(host)
    assert [x.tobytes() for x in d.encoded] == [x.tobytes() for x in h.encoded] and d.filenames == h.filenames
    assert d.origins == h.origins and all(type(x) is bytes for x in d.filenames)
    assert d.labels.is_cuda == return_logits and not h.labels.is_cuda
    assert d.labels.dtype == h.labels.dtype and d.labels.shape == h.labels.shape
    assert d.labels.cpu().numpy().tobytes() == h.labels.numpy().tobytes()
    assert (d.payloads is None) == (h.payloads is None) == (not keep)
    if keep:
      assert d.payloads[1].dtype == np.int64 and d.payloads[1].tolist() == h.payloads[1].tolist()
      if seen == 0:
        kw2 = dict(image_size=16, jpeg_entropy='parallel', jpeg_parse='device')
        got = ip.preprocess_batch(d.encoded, False, 'cuda', jpeg_resident=d.payloads, **kw2)
        ref = ip.preprocess_batch(h.encoded, False, 'cuda', jpeg_resident=h.payloads, **kw2)
        assert got.shape == (len(d.encoded), 16, 16, 3) and torch.equal(got, ref)
    seen += len(d.encoded)
  assert seen == 11 and next(host, None) is None


def test_dataset_errors_are_the_host_parsers(product, shards, tmp_path):
  from assembled_cnn_amd import records
  paths, payloads = shards
  texts = {}
  cut = str(tmp_path / 'cut')
  records.write_records(cut, [payloads[0], payloads[1][:-3], payloads[2]])      # a truncated proto behind a valid checksum
  for parse in ('host', 'device'):
    ds = records.RecordDataset([cut], False, 3, 1, verify='device', device='cuda', parse=parse)
    with pytest.raises(ValueError) as err:
      next(iter(ds))
    ds = records.RecordDataset(paths, False, 3, 1, verify='device', device='cuda', parse=parse, return_logits=True, num_classes=C4 + 1)
    with pytest.raises(ValueError) as count:
      next(iter(ds))
    texts[parse] = (str(err.value), str(count.value))
  assert texts['host'] == texts['device']
  assert 'cut: record at byte' in texts['host'][0] and 'image/logit holds 4 values, num_classes is 5' in texts['host'][1]
  # a checksum mismatch is reported first, as today
  with open(cut, 'r+b') as fh:
    fh.seek(40)
    b = fh.read(1)
    fh.seek(40)
    fh.write(bytes([b[0] ^ 0x10]))
  for parse in ('host', 'device'):
    with pytest.raises(ValueError, match='payload checksum mismatch'):
      next(iter(records.RecordDataset([cut], False, 3, 1, verify='device', device='cuda', parse=parse)))
