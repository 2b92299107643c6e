"""The device header parse (asm_jpeg_parse / asm_jpeg_parse_fill, csrc/jpeg_parse.h) against jpeg.parse / jpeg.pack: the
class of every file, every row field by field, and decode_batch / preprocess_batch with parse='device' against the host
parse on the same batch -- exact equality everywhere."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import gpu_guard as G
from tests import jpeg_parse_cases as cases
from tests.gpu_guard import _release_inputs  # noqa: F401

pytestmark = pytest.mark.gpu

ALIGNED = ('tex_200x152_420', 'stuffed_noise_32x24_444', 'rst1_444_noise_72x72', 'rst1_grey_168x160')
_FILES = {}


@pytest.fixture(scope='module')
def product():
  import __graft_entry__
  __graft_entry__.build()
  from assembled_cnn_amd import ops
  ops.set_library(None, is_double=False)
  return ops


def batch():
  """[(name, bytes, accepted by jpeg.parse)]: every device fixture, every header variant, cmyk and progressive"""
  if not _FILES:
    fx = cases.load()
    for n, (data, kind, _) in fx.items():
      if kind == 'device':
        _FILES[n] = data
    _FILES.update(cases.variants(fx))
  return [(n, d, cases.expected(d)) for n, d in _FILES.items()]


def _check_rows(pk, where, descs, tables, intervals, first):
  """device rows (numpy views) against jpeg.pack's; where: position in buf of each row's file"""
  from assembled_cnn_amd import jpeg
  descs, tables = descs.view(jpeg.DESC_DTYPE), tables.view(jpeg.TABLES_DTYPE)
  intervals = intervals.view(jpeg.INTERVAL_DTYPE)
  assert len(descs) == len(pk.descs) and len(intervals) == len(pk.intervals)
  for f in jpeg.DESC_DTYPE.names:
    if f != 'scan_offset':
      assert np.array_equal(descs[f], pk.descs[f]), f
  assert tables.tobytes() == pk.tables.tobytes()
  for f in ('image', 'first_mcu', 'n_mcus', 'rst'):
    assert np.array_equal(intervals[f], pk.intervals[f]), f
  # positions: in the caller's buffer here, in the host's pool there; equal relative to scan_offset
  img = intervals['image']
  for f in ('byte_begin', 'byte_end'):
    assert np.array_equal(intervals[f] - descs['scan_offset'][img], pk.intervals[f] - pk.descs['scan_offset'][img]), f
  assert np.array_equal(descs['scan_offset'] - where, [jpeg.parse(pk_file).scan_begin for pk_file in pk.row_files])
  if first is not None:
    assert np.array_equal(first, pk.segment_first)


def _host_pack(files, segment_bytes):
  from assembled_cnn_amd import jpeg
  pk = jpeg.pack(files, segment_bytes=segment_bytes)
  pk.row_files = files
  return pk


@pytest.mark.parametrize('segment_bytes', [16, 128])
def test_every_file_in_one_ragged_call_between_flanks(product, segment_bytes):
  from assembled_cnn_amd import jpeg, lib
  files = batch()
  n = len(files)
  lengths = np.array([len(d) for _, d, _ in files], np.int64)
  offsets = 1 + np.cumsum(lengths) - lengths          # back to back, no padding, odd offsets among them
  assert (offsets % 2).any() and (offsets % 16 != 0).sum() > n // 2
  raw = np.concatenate([[0xFF]] + [np.frombuffer(d, np.uint8) for _, d, _ in files]).astype(np.uint8)
  buf = G.In(raw, dtype=torch.uint8, flank_value=0xFF)
  spans = np.zeros(n, jpeg.SPAN_DTYPE)
  spans['offset'], spans['length'] = offsets, lengths
  spans_dev = G.dev(spans.view(np.uint8), torch.uint8)
  heads_out = G.Out((n * jpeg.HEAD_DTYPE.itemsize,), torch.uint8)
  tables_out = G.Out((n * jpeg.TABLES_DTYPE.itemsize,), torch.uint8)
  G.call('asm_jpeg_parse', buf.p, raw.size, G.ptr(spans_dev), n, segment_bytes, heads_out.p, tables_out.p)
  heads_out.check_flanks()
  tables_out.check_flanks()
  heads = heads_out.t.cpu().numpy().view(jpeg.HEAD_DTYPE)
  for (name, _, ok), h in zip(files, heads):
    assert (h['cls'] == 0) == ok, (name, int(h['cls']))
  for name in ('empty', 'one_byte', 'zeros'):
    assert heads['cls'][[f[0] for f in files].index(name)] == lib.JPEG_PNOTJPEG
  block = tables_out.t.cpu().numpy().reshape(n, -1)
  assert not block[heads['cls'] != 0].any()
  accepted = [d for _, d, ok in files if ok]
  pk = _host_pack(accepted, segment_bytes)
  place, rows, dst_offsets, total, totals = jpeg.layout_heads(heads, [(0, 0)] * n,
                                                             [k for k in range(n) if heads['cls'][k]], segment_bytes)
  assert totals == dict(total_blocks=pk.total_blocks, max_blocks=pk.max_blocks, max_pixels=pk.max_pixels,
                        n_intervals=len(pk.intervals), total_segments=pk.total_segments)
  assert np.array_equal(dst_offsets[rows], pk.offsets) and max(total, 16) == pk.total_bytes
  n_rows, n_iv = len(place), totals['n_intervals']
  out = [G.Out((n_rows * jpeg.DESC_DTYPE.itemsize,), torch.uint8), G.Out((n_rows * jpeg.TABLES_DTYPE.itemsize,), torch.uint8),
         G.Out((n_iv * jpeg.INTERVAL_DTYPE.itemsize,), torch.uint8), G.Out((n_iv,), torch.int32),
         G.Out((n_rows,), torch.int32)]
  G.call('asm_jpeg_parse_fill', buf.p, raw.size, G.ptr(spans_dev), n, heads_out.p, tables_out.p,
         G.ptr(G.dev(place.view(np.uint8), torch.uint8)), n_rows, n_iv, totals['total_segments'], segment_bytes,
         *[o.p for o in out])
  for o in out:
    o.check_flanks()
  assert not out[4].t.cpu().numpy().any()
  _check_rows(pk, offsets[rows], *[o.t.cpu().numpy() for o in out[:4]])


def test_every_start_alignment_of_the_scan(product):
  """each file at all 16 offsets of a 16-byte vector: every FF xx pair crosses the lane and pass boundaries of the scan"""
  from assembled_cnn_amd import jpeg, staging
  fx = cases.load()
  files, where, at = [], [], 0
  for name in ALIGNED:
    for a in range(16):
      at = (at + 15) // 16 * 16 + a
      files.append(fx[name][0])
      where.append(at)
      at += len(fx[name][0])
  raw = np.full(at + 16, 0xFF, np.uint8)
  for o, d in zip(where, files):
    raw[o:o + len(d)] = np.frombuffer(d, np.uint8)
  n = len(files)
  spans = np.zeros(n, jpeg.SPAN_DTYPE)
  spans['offset'], spans['length'] = where, [len(d) for d in files]
  buf, spans_dev = torch.from_numpy(raw).cuda(), staging.upload_table(spans, 'cuda')
  for segment_bytes in (16, 128):
    heads_dev, tables_dev = product.jpeg_parse(buf, spans_dev, n, segment_bytes)
    heads = heads_dev.cpu().numpy().view(jpeg.HEAD_DTYPE)
    assert not heads['cls'].any()
    place, rows, _, _, totals = jpeg.layout_heads(heads, None, (), segment_bytes)
    got = product.jpeg_parse_fill(buf, spans_dev, n, heads_dev, tables_dev, staging.upload_table(place, 'cuda'), n,
                                  totals['n_intervals'], totals['total_segments'], segment_bytes)
    assert not got[4].cpu().numpy().any()
    _check_rows(_host_pack(files, segment_bytes), np.array(where), *[t.cpu().numpy() for t in got[:4]])


def _mixed():
  fx = cases.load()
  v = cases.variants(fx)
  names = [n for n, f in fx.items() if f[1] == 'device']
  files = [fx[n][0] for n in names]
  decoded = np.arange(6 * 9 * 3, dtype=np.uint8).reshape(6, 9, 3)
  extra = [v['cmyk_16x16'], decoded, v['progressive_16x16'], v['fill_bytes'], v['dqt_16bit'], v['dht_merged']]
  return names, files + extra, fx


def _fallback(data):
  return np.full((4, 5, 3), len(data) % 251, np.uint8)


def _slots(buf, offsets, sizes):
  host = buf.cpu().numpy()
  return [host[int(o):int(o) + h * w * 3].reshape(h, w, 3) for o, (h, w) in zip(offsets, sizes)]


@pytest.mark.parametrize('entropy,progressive', [('sequential', False), ('parallel', False), ('parallel', True)])
def test_decode_batch_with_device_parse_equals_host_parse(product, entropy, progressive):
  from assembled_cnn_amd import jpeg
  names, files, fx = _mixed()
  kw = dict(fallback=_fallback, progressive=progressive, entropy=entropy)
  ref, ref_offsets, ref_sizes = jpeg.decode_batch(files, 'cuda', parse='host', **kw)
  got, offsets, sizes = jpeg.decode_batch(files, 'cuda', parse='device', **kw)
  assert np.array_equal(offsets, ref_offsets) and sizes == ref_sizes and got.shape == ref.shape
  a, b = _slots(got, offsets, sizes), _slots(ref, ref_offsets, ref_sizes)
  for k in range(len(files)):
    assert np.array_equal(a[k], b[k]), k
  for k, name in enumerate(names):
    assert np.array_equal(a[k], fx[name][2]), name


def test_device_parse_raises_what_the_host_parse_raises(product):
  from assembled_cnn_amd import jpeg
  _, files, fx = _mixed()
  for bad in (files, files[:3] + [cases.variants(fx)['no_eoi']] + files[3:5]):
    errors = []
    for parse in ('host', 'device'):
      with pytest.raises((NotImplementedError, ValueError)) as err:
        jpeg.decode_batch(bad, 'cuda', parse=parse, fallback=None if bad is files else _fallback)
      errors.append((type(err.value), str(err.value)))
    assert errors[0] == errors[1]
  assert errors[0][0] is ValueError and 'EOI' in errors[0][1]
  buf = torch.zeros(64, dtype=torch.uint8, device='cuda')
  with pytest.raises(ValueError, match='entry 1: a decoded image cannot be resident'):
    jpeg.pack_device([files[0], np.zeros((2, 2, 3), np.uint8)], 'cuda', resident=(buf, np.zeros((2, 2), np.int64)))


@pytest.mark.parametrize('verify', ['device', 'host', 'none'])
def test_records_keep_their_payloads_for_the_decoder(product, tmp_path, verify):
  from assembled_cnn_amd import input_pipeline as ip, records
  names, files, fx = _mixed()
  files = [f for f in files if not isinstance(f, np.ndarray)]
  path = str(tmp_path / 'validation-00000-of-00001')
  records.write_records(path, [records.encode_example({'image/encoded': [d], 'image/filename': [b'f%d' % i],
                                                       'image/class/label': np.array([i])}) for i, d in enumerate(files)])
  half = (len(files) + 1) // 2
  ds = records.RecordDataset([path], False, half, 1, verify=verify, device='cuda', keep_payloads=True)
  seen = 0
  for b in ds:                                   # two consecutive batches: the staging buffers are reused
    n = len(b.encoded)
    buf, where = b.payloads
    assert buf.is_cuda and where.shape == (n, 2) and where.dtype == np.int64
    assert [e.tobytes() for e in b.encoded] == files[seen:seen + n]
    assert np.array_equal(where[:, 1], [len(d) for d in files[seen:seen + n]])
    windows = [dict(crop_y=0, crop_x=0, crop_h=h, crop_w=w, resize_h=16, resize_w=16, out_y=0, out_x=0, flip=k % 2)
               for k, (h, w) in enumerate(_sizes(b.encoded))]
    kw = dict(image_size=16, windows=windows, jpeg_fallback=_fallback, jpeg_entropy='parallel')
    ref = ip.preprocess_batch(b.encoded, False, 'cuda', **kw)
    got = ip.preprocess_batch(b.encoded, False, 'cuda', jpeg_parse='device', jpeg_resident=b.payloads, **kw)
    assert torch.equal(got, ref)
    seen += n
  assert seen == len(files) and half < len(files)


def _sizes(encoded):
  from assembled_cnn_amd import jpeg
  out = []
  for e in encoded:
    info = jpeg.parse(e)
    out.append((4, 5) if info.unsupported is not None else (info.height, info.width))
  return out


def test_empty_and_refused_calls_launch_nothing(product):
  from assembled_cnn_amd import jpeg, lib
  L = product.L()
  buf = torch.zeros(64, dtype=torch.uint8, device='cuda')
  t = torch.zeros(4096, dtype=torch.uint8, device='cuda')
  p, b = t.data_ptr(), buf.data_ptr()
  before = L.asm_launch_count()
  assert L.asm_jpeg_parse(b, 64, p, 0, 16, p, p, 0) == lib.ASM_OK
  assert L.asm_jpeg_parse_fill(b, 64, p, 0, p, p, p, 0, 0, 0, 16, p, p, p, p, p, 0) == lib.ASM_OK
  assert L.asm_jpeg_parse_fill(b, 64, p, 0, p, p, p, 0, 0, 0, 0, p, p, p, 0, p, 0) == lib.ASM_OK
  parse_bad = [(0, 64, p, 1, 16, p, p), (b, 64, 0, 1, 16, p, p), (b, 64, p, 1, 16, 0, p), (b, 64, p, 1, 16, p, 0),
               (b, 64, p, -1, 16, p, p), (b, 64, p, 1, 8, p, p), (b, 64, p, 1, 24, p, p), (b, 64, p, 1, 65552, p, p),
               (b, -1, p, 1, 16, p, p), (b, 2 ** 40, p, 1, 16, p, p)]
  for args in parse_bad:
    assert L.asm_jpeg_parse(*args, 0) == lib.ASM_EINVAL, args
  good = [b, 64, p, 1, p, p, p, 1, 1, 1, 16, p, p, p, p, p]
  for at, value in ((0, 0), (2, 0), (4, 0), (5, 0), (6, 0), (11, 0), (12, 0), (13, 0), (14, 0), (15, 0), (3, -1), (7, -1),
                    (8, -1), (9, -1), (9, 2 ** 30), (10, 8), (10, 24), (1, -1), (1, 2 ** 40)):
    args = list(good)
    args[at] = value
    assert L.asm_jpeg_parse_fill(*args, 0) == lib.ASM_EINVAL, (at, value)
  assert L.asm_launch_count() == before
  heads, tables = product.jpeg_parse(buf, t[:0], 0, 16)
  assert heads.numel() == 0 and tables.numel() == 0
  pk = jpeg.pack_device([], 'cuda', segment_bytes=16)
  out = jpeg.decode_packed(pk, 'cuda', entropy='parallel')
  assert out[1] is None and L.asm_launch_count() == before
  assert C.sizeof(lib.JpegHead) == 72 and os.path.exists(os.path.join(cases.GOLDEN, 'jpeg_parse_fixtures.npz'))
