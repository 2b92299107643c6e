"""JPEG decode on the device (csrc/jpeg.hip) against the recorded Pillow pixels and tests/jpeg_ref.py: exact equality."""
import os

import numpy as np
import pytest
import torch

from tests import jpeg_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FX = {}


def fixtures():
  """name -> (kind, file bytes, recorded pixels or None), loaded once"""
  if not _FX:
    fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_fixtures.npz'))
    for name in fx['names']:
      name = str(name)
      kind = str(fx['kind_' + name])
      _FX[name] = (kind, fx['file_' + name].tobytes(), fx['pix_' + name] if kind == 'device' else None)
  return _FX


def device_fixtures():
  return [(n, f, p) for n, (k, f, p) in fixtures().items() if k == 'device']


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


def test_every_fixture_in_one_ragged_launch_equals_pillow_and_the_reference_coefficients(product):
  from assembled_cnn_amd import jpeg
  fx = device_fixtures()
  pk = jpeg.pack([f for _, f, _ in fx])
  assert len(pk.dev_index) == len(fx) >= 39
  dst, status, ws = jpeg.decode_packed(pk, 'cuda', return_workspace=True)
  assert status.tolist() == [0] * len(fx)
  for (name, _, pix), got in zip(fx, _images(dst, pk.offsets, pk.sizes)):
    assert got.shape == pix.shape and np.array_equal(got, pix), name
  # the raw coefficients the entropy stage left in the workspace
  coefs = ws.cpu().numpy()[:pk.total_blocks * 128].view('<i2')
  for (name, f, _), d in zip(fx, pk.descs):
    want = np.concatenate([c.reshape(-1) for c in jpeg_ref.coefficients(f)[0]])
    got = coefs[int(d['coef_offset']):int(d['coef_offset']) + want.size]
    assert np.array_equal(got, want), name


def test_single_image_batches(product):
  from assembled_cnn_amd import jpeg
  for name in ('noise_1x1_420', 'noise_17x33_420', 'rst1_444_noise_72x72', 'grey_13x17'):
    _, f, pix = fixtures()[name]
    buf, offsets, sizes = jpeg.decode_batch([f], 'cuda')
    assert sizes == [pix.shape[:2]] and np.array_equal(_images(buf, offsets, sizes)[0], pix), name


def test_seventy_images(product):
  from assembled_cnn_amd import jpeg
  fx = device_fixtures()
  batch = [fx[k % len(fx)] for k in range(70)]
  # bytes, bytearray and uint8 arrays are all encoded files
  files = [f if k % 3 == 0 else bytearray(f) if k % 3 == 1 else np.frombuffer(f, np.uint8) for k, (_, f, _) in enumerate(batch)]
  buf, offsets, sizes = jpeg.decode_batch(files, 'cuda', dct_method='INTEGER_ACCURATE')
  assert all(int(o) % 16 == 0 for o in offsets)
  for (name, _, pix), got in zip(batch, _images(buf, offsets, sizes)):
    assert np.array_equal(got, pix), name


def _big_enough():
  """fixtures an eval window of side 16 fits (the resize needs at least 16 x 16 after scaling: any size does) """
  return [(n, f, p) for n, f, p in device_fixtures() if min(p.shape[:2]) >= 8]


@pytest.mark.parametrize('is_training', [False, True])
def test_preprocess_batch_from_bytes_equals_preprocess_batch_from_pixels(product, is_training):
  from assembled_cnn_amd import input_pipeline as ip
  fx = _big_enough()
  rng = np.random.default_rng(7)
  side = 16
  if is_training:
    windows = [ip.train_window(p.shape[0], p.shape[1], side, side, rng) for _, _, p in fx]
  else:
    windows = [ip.eval_window(p.shape[0], p.shape[1], side, side) for _, _, p in fx]
  kw = dict(is_training=is_training, device='cuda', image_size=side, windows=windows)
  want = ip.preprocess_batch([np.ascontiguousarray(p) for _, _, p in fx], **kw)
  got = ip.preprocess_batch([f for _, f, _ in fx], **kw)
  assert got.shape == want.shape == (len(fx), side, side, 3)
  assert torch.equal(got, want)
  # the windows preprocess_batch computes itself come from the parsed header: the same as from the pixels
  if not is_training:
    assert torch.equal(ip.preprocess_batch([f for _, f, _ in fx], False, 'cuda', image_size=side), want)


def test_mixed_batch_with_a_fallback_entry_and_a_decoded_array(product):
  from assembled_cnn_amd import input_pipeline as ip, jpeg
  fxs = fixtures()
  _, prog, _ = fxs['progressive_16x16']
  stand_in = np.arange(16 * 16 * 3, dtype=np.uint8).reshape(16, 16, 3)      # what the caller's decoder returns
  calls = []

  def fallback(data):
    calls.append(data)
    return stand_in

  names = ['smooth_17x33_420', 'noise_13x17_422', 'rst2_422_33x47']
  decoded = fxs['opt_444_24x20'][2]
  entries = [fxs[names[0]][1], prog, fxs[names[1]][1], decoded, fxs[names[2]][1]]
  pixels = [fxs[names[0]][2], stand_in, fxs[names[1]][2], decoded, fxs[names[2]][2]]
  buf, offsets, sizes = jpeg.decode_batch([e for e in entries if not isinstance(e, np.ndarray)], 'cuda', fallback=fallback)
  assert calls == [prog]
  for got, want in zip(_images(buf, offsets, sizes), [p for p, e in zip(pixels, entries) if not isinstance(e, np.ndarray)]):
    assert np.array_equal(got, want)
  got = ip.preprocess_batch(entries, False, 'cuda', image_size=16, jpeg_fallback=fallback)
  want = ip.preprocess_batch([np.ascontiguousarray(p) for p in pixels], False, 'cuda', image_size=16)
  assert torch.equal(got, want)
  with pytest.raises(NotImplementedError, match='entry 1.*progressive'):
    ip.preprocess_batch(entries, False, 'cuda', image_size=16)
  with pytest.raises(NotImplementedError, match='INTEGER_FAST'):
    ip.preprocess_batch(entries, False, 'cuda', image_size=16, dct_method='INTEGER_FAST', jpeg_fallback=fallback)


def test_corrupt_scans_give_a_status_zero_pixels_and_a_value_error(product):
  """The error path, not a fault: both inputs are among those tools/probes/jpeg_entropy_host.cpp runs under the sanitizers
  (a truncation of this scan; this scan with one byte replaced by FF and by D9)."""
  from assembled_cnn_amd import jpeg, lib
  _, good, pix = fixtures()['noise_17x33_420']
  info = jpeg.parse(good)
  mid = (info.scan_begin + info.scan_end) // 2
  truncated = good[:mid] + b'\xff\xd9'                      # cut in the middle of the (only) interval
  a = bytearray(good)
  a[mid], a[mid + 1] = 0xFF, 0xD9                            # an EOI marker inside the scan
  _, other, other_pix = fixtures()['smooth_13x17_444']
  files = [other, truncated, bytes(a), other]
  pk = jpeg.pack(files)
  dst, status = jpeg.decode_packed(pk, 'cuda', check=False)
  status = status.cpu().tolist()
  assert status[0] == 0 and status[3] == 0
  assert status[1] & (lib.JPEG_EOVERRUN | lib.JPEG_EBADCODE) and status[2] & (lib.JPEG_EOVERRUN | lib.JPEG_EBADCODE)
  out = _images(dst, pk.offsets, pk.sizes)
  assert np.array_equal(out[0], other_pix) and np.array_equal(out[3], other_pix)      # the neighbours are untouched
  assert not out[1].any() and not out[2].any()
  with pytest.raises(ValueError, match=r'entries \[1, 2\]'):
    jpeg.decode_batch(files, 'cuda')


@pytest.mark.parametrize('entropy', ['sequential', 'parallel'])
def test_damaged_tables_take_the_status_paths(product, entropy):
  """Damage done AFTER packing, so that it reaches the device as it is (the host parser would end the scan at a marker):
  a marker inside an interval, a restart marker out of sequence, an interval count that does not match the geometry, an
  interval row outside the image's scan, a descriptor with an impossible geometry.  Each ends its image with the status
  bit of its kind and zero pixels; the untouched images of the same launch decode.  The damaged scans are among those the
  host sanitizer programs run (a byte replaced by FF; the damaged rows of tools/probes/jpeg_probe.h).
  entropy='parallel': the same pack in segments of 16 bytes, the segment table made from the damaged rows so that they
  reach the kernel's own check of each interval row; every status word also equals the sequential run's."""
  from assembled_cnn_amd import jpeg, lib
  fxs = fixtures()
  names = ['noise_17x33_420', 'rst2_422_33x47', 'rst1_444_40x48', 'rst1_grey_40x48', 'smooth_13x17_444', 'noise_13x17_422']
  pk = jpeg.pack([fxs[n][1] for n in names], segment_bytes=16 if entropy == 'parallel' else None)
  d, iv = pk.descs, pk.intervals
  # 0: FF + a non-zero byte in the middle of the only interval: the data ends there, the MCUs after it are missing
  mid = int(d[0]['scan_offset'] + d[0]['scan_bytes'] // 2)
  pk.files[mid], pk.files[mid + 1] = 0xFF, 0x5A
  # 1: the marker after the second interval is RST2 where RST1 belongs
  iv['rst'][int(d[1]['first_interval']) + 1] = 2
  # 2: one interval fewer than the geometry has
  d['n_intervals'][2] -= 1
  # 3: an interval row that ends past the image's scan
  iv['byte_end'][int(d[3]['first_interval']) + 5] = int(d[3]['scan_offset'] + d[3]['scan_bytes']) + 1
  # 4: a geometry that is none (the slot in dst still fits, so it is zeroed)
  d['mcus_x'][4] += 1
  if entropy == 'parallel':
    pk.segment_first, pk.total_segments = jpeg.segment_table(pk.intervals, pk.segment_bytes)
    assert jpeg.decode_packed(pk, 'cuda', check=False)[1].cpu().tolist() == \
        jpeg.decode_packed(pk, 'cuda', check=False, entropy='parallel')[1].cpu().tolist()
  dst, status = jpeg.decode_packed(pk, 'cuda', check=False, entropy=entropy)
  status = status.cpu().tolist()
  assert status[0] & lib.JPEG_EOVERRUN and not status[0] & (lib.JPEG_ERESTART | lib.JPEG_EDESC)
  assert status[1] == lib.JPEG_ERESTART and status[2] == lib.JPEG_ERESTART
  assert status[3] == lib.JPEG_EDESC and status[4] == lib.JPEG_EDESC and status[5] == 0
  out = _images(dst, pk.offsets, pk.sizes)
  for k in range(5):
    assert not out[k].any(), names[k]
  assert np.array_equal(out[5], fxs[names[5]][2])
