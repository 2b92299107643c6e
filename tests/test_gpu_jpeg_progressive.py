"""Progressive JPEG decode on the device (jpeg_progressive_kernel + the pixel stages of csrc/jpeg.hip) against the recorded
Pillow pixels and tests/jpeg_progressive_ref.py: exact equality."""
import os

import numpy as np
import pytest
import torch

from tests import jpeg_progressive_ref as ref
from tests import jpeg_progressive_writer as writer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECODED = ('smooth_1x1_420', 'noise_13x17_420', 'smooth_17x33_422', 'noise_31x9_444', 'grey_13x17', 'flat_20x20',
           'opt_420_31x29')
_FX, _BASE, _RECODED = {}, {}, []


def fixtures():
  """name -> (file bytes, recorded pixels), loaded once"""
  if not _FX:
    fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_progressive_fixtures.npz'))
    for name in fx['names']:
      _FX[str(name)] = (fx['file_' + str(name)].tobytes(), fx['pix_' + str(name)])
  return _FX


def baseline():
  if not _BASE:
    fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_fixtures.npz'))
    for name in fx['names']:
      if str(fx['kind_' + str(name)]) == 'device':
        _BASE[str(name)] = (fx['file_' + str(name)].tobytes(), fx['pix_' + str(name)])
  return _BASE


def recoded():
  """[(name, file bytes, the baseline fixture's pixels)]: every script of the writer over a few baseline fixtures"""
  if not _RECODED:
    for name in RECODED:
      f, pix = baseline()[name]
      for script in writer.SCRIPTS:
        _RECODED.append(('%s/%s' % (name, script), writer.recode(f, script), pix))
  return _RECODED


@pytest.fixture(scope='module')
def product():
  import __graft_entry__
  __graft_entry__.build()
  from assembled_cnn_amd import ops
  ops.set_library(None, is_double=False)
  return ops


def _images(buf, offsets, sizes):
  host = buf.cpu().numpy()
  return [host[int(o):int(o) + h * w * 3].reshape(h, w, 3) for o, (h, w) in zip(offsets, sizes)]


def test_every_fixture_and_recoded_file_in_one_ragged_launch(product):
  from assembled_cnn_amd import jpeg
  fx = [(n, f, p) for n, (f, p) in fixtures().items()] + recoded()
  pk = jpeg.pack([f for _, f, _ in fx], progressive=True)
  assert pk.prog_index == list(range(len(fx))) and pk.dev_index == [] and len(fx) >= 48 + 21
  dst, status, ws, prog_ws = jpeg.decode_packed(pk, 'cuda', return_workspace=True)
  assert ws is None and status.tolist() == [0] * len(fx)
  for (name, _, pix), got in zip(fx, _images(dst, pk.offsets, pk.sizes)):
    assert got.shape == pix.shape and np.array_equal(got, pix), name
  # the raw coefficients the entropy stage left in the workspace: equal to the reference's on each component's true block
  # grid, and zero in the padded blocks no scan visits (as the reference leaves them)
  coefs = prog_ws.cpu().numpy()[:pk.prog_total_blocks * 128].view('<i2')
  for (name, f, _), d in zip(fx, pk.prog_descs):
    want, h = ref.coefficients(f)
    at = int(d['coef_offset'])
    for c, w in enumerate(want):
      got = coefs[at:at + w.size].reshape(w.shape)
      th, tw = ref.true_grid(h, c)
      assert np.array_equal(got[:th, :tw], w[:th, :tw]), (name, c)
      assert np.array_equal(got, w), (name, c)
      at += w.size


def test_single_image_batches(product):
  from assembled_cnn_amd import jpeg
  for name in ('noise_1x1_420', 'noise_17x33_420', 'rst1_grey_40x48', 'rst2_422_33x47', 'grey_13x17'):
    f, pix = fixtures()[name]
    buf, offsets, sizes = jpeg.decode_batch([f], 'cuda', progressive=True)
    assert sizes == [pix.shape[:2]] and np.array_equal(_images(buf, offsets, sizes)[0], pix), name


def test_seventy_entries_of_both_kinds(product):
  from assembled_cnn_amd import jpeg
  seq = list(baseline().items())
  prog = list(fixtures().items())
  batch = [(seq if k % 2 == 0 else prog)[(k // 2) % len(prog if k % 2 else seq)] for k in range(70)]
  # bytes, bytearray and uint8 arrays are all encoded files; entry 33 is an already decoded image
  files = [f if k % 3 == 0 else bytearray(f) if k % 3 == 1 else np.frombuffer(f, np.uint8) for k, (_, (f, _)) in enumerate(batch)]
  files[33] = np.ascontiguousarray(batch[33][1][1])
  buf, offsets, sizes = jpeg.decode_batch(files, 'cuda', dct_method='INTEGER_ACCURATE', progressive=True)
  assert all(int(o) % 16 == 0 for o in offsets)
  for (name, (_, pix)), got in zip(batch, _images(buf, offsets, sizes)):
    assert np.array_equal(got, pix), name
  pk = jpeg.pack(files, progressive=True)
  assert len(pk.dev_index) == 35 and len(pk.prog_index) == 34 and sorted(pk.fallback) == [33]


@pytest.mark.parametrize('is_training', [False, True])
def test_preprocess_batch_from_progressive_bytes_equals_preprocess_batch_from_pixels(product, is_training):
  from assembled_cnn_amd import input_pipeline as ip
  fx = [(n, f, p) for n, (f, p) in fixtures().items() if min(p.shape[:2]) >= 8]
  fx.insert(3, ('baseline', ) + baseline()['smooth_17x33_420'])      # a sequential file among them
  rng = np.random.default_rng(7)
  side = 16
  if is_training:
    windows = [ip.train_window(p.shape[0], p.shape[1], side, side, rng) for _, _, p in fx]
  else:
    windows = [ip.eval_window(p.shape[0], p.shape[1], side, side) for _, _, p in fx]
  kw = dict(is_training=is_training, device='cuda', image_size=side, windows=windows)
  want = ip.preprocess_batch([np.ascontiguousarray(p) for _, _, p in fx], **kw)
  got = ip.preprocess_batch([f for _, f, _ in fx], jpeg_progressive=True, **kw)
  assert got.shape == want.shape == (len(fx), side, side, 3)
  assert torch.equal(got, want)
  with pytest.raises(NotImplementedError, match='entry 0.*progressive'):
    ip.preprocess_batch([f for _, f, _ in fx], **kw)


def _scan_row(pk, image, pick):
  """row of pk.prog_scans: the first scan of `image` for which pick(row) holds"""
  d = pk.prog_descs[image]
  for k in range(int(d['first_interval']), int(d['first_interval'] + d['n_intervals'])):
    if pick(pk.prog_scans[k]):
      return k
  raise AssertionError('no such scan')


def test_damaged_scans_and_rows_take_the_status_paths(product):
  """The error paths, not faults.  Damage done AFTER packing, so that it reaches the device as it is.  Every input is one
  tools/probes/jpeg_progressive_host.cpp runs under the sanitizers: a truncation of a scan, two bytes of a scan replaced by
  FF D9, a wrong RSTm, an interval count off by one, a Huffman-pool index out of range."""
  from assembled_cnn_amd import jpeg, lib
  fx = fixtures()
  names = ['smooth_13x17_444', 'noise_17x33_420', 'noise_17x33_444', 'rst2_422_33x47', 'rst1_grey_40x48', 'noise_13x17_422',
           'smooth_31x9_420']
  pk = jpeg.pack([fx[n][0] for n in names], progressive=True)
  sc, iv = pk.prog_scans, pk.prog_intervals
  # 1: the first AC refinement scan ends in its middle
  k = _scan_row(pk, 1, lambda r: r['ss'] > 0 and r['ah'] > 0)
  mid = int(sc[k]['byte_begin'] + sc[k]['byte_end']) // 2
  assert sc[k]['n_intervals'] == 1 and sc[k]['byte_begin'] + 4 < mid
  sc['byte_end'][k] = iv['byte_end'][int(sc[k]['first_interval'])] = mid
  # 2: FF D9 in the middle of the DC scan
  k = _scan_row(pk, 2, lambda r: r['ss'] == 0 and r['ah'] == 0)
  mid = int(sc[k]['byte_begin'] + sc[k]['byte_end']) // 2
  pk.prog_files[mid], pk.prog_files[mid + 1] = 0xFF, 0xD9
  # 3: the marker after the second interval of the second scan is RST2 where RST1 belongs
  k = int(pk.prog_descs[3]['first_interval']) + 1
  assert sc[k]['n_intervals'] > 2
  iv['rst'][int(sc[k]['first_interval']) + 1] = 2
  # 4: one interval fewer than the fourth scan's geometry has
  sc['n_intervals'][int(pk.prog_descs[4]['first_interval']) + 3] -= 1
  # 5: a Huffman-pool row past the pool
  k = _scan_row(pk, 5, lambda r: r['ss'] > 0)
  sc['huff'][k][0] = len(pk.prog_huff)
  dst, status = jpeg.decode_packed(pk, 'cuda', check=False)
  status = status.cpu().tolist()
  assert status[0] == 0 and status[6] == 0
  for k in (1, 2):
    assert status[k] & (lib.JPEG_EOVERRUN | lib.JPEG_EBADCODE) and not status[k] & (lib.JPEG_ERESTART | lib.JPEG_EDESC)
  assert status[3] == lib.JPEG_ERESTART and status[4] == lib.JPEG_ERESTART and status[5] == lib.JPEG_EDESC
  out = _images(dst, pk.offsets, pk.sizes)
  for k in range(1, 6):
    assert not out[k].any(), names[k]
  assert np.array_equal(out[0], fx[names[0]][1]) and np.array_equal(out[6], fx[names[6]][1])      # the neighbours decode


def test_corrupt_files_of_either_group_are_named_in_one_value_error(product):
  """A progressive file whose AC refinement scan lost its second half (a truncation the host sanitizer program runs) and a
  sequential file cut in its scan (one tools/probes/jpeg_entropy_host.cpp runs), among good files of both kinds."""
  from assembled_cnn_amd import jpeg
  f, pix = fixtures()['noise_17x33_420']
  info = jpeg.parse(f, progressive=True)
  scan = [s for s in info.scans if s.ss > 0 and s.ah > 0][0]
  cut = f[:(scan.begin + scan.end) // 2] + f[scan.end:]
  good, good_pix = baseline()['noise_17x33_420']
  binfo = jpeg.parse(good)
  truncated = good[:(binfo.scan_begin + binfo.scan_end) // 2] + b'\xff\xd9'
  files = [good, cut, f, truncated, cut]
  with pytest.raises(ValueError, match=r'entries \[1, 3, 4\]'):
    jpeg.decode_batch(files, 'cuda', progressive=True)
  pk = jpeg.pack(files, progressive=True)
  dst, status = jpeg.decode_packed(pk, 'cuda', check=False)
  assert [bool(s) for s in status.cpu().tolist()] == [False, True, True, False, True]      # rows: 0, 3 | 1, 2, 4
  out = _images(dst, pk.offsets, pk.sizes)
  assert np.array_equal(out[0], good_pix) and np.array_equal(out[2], pix)
  assert not out[1].any() and not out[3].any() and not out[4].any()
