"""The segment-parallel JPEG entropy stage (asm_jpeg_decode_parallel, csrc/jpeg_parallel.h) against the recorded Pillow
pixels, tests/jpeg_ref.py's coefficients and the sequential stage on the same pack: exact equality everywhere."""
import os

import numpy as np
import pytest
import torch

from tests import jpeg_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = 256       # jpeg_entropy_parallel_kernel's workgroup
BIG = 'tex_200x152_420'
_FX = {}


def fixtures():
  """name -> (kind, file bytes, recorded pixels or None) of both fixture files, loaded once"""
  if not _FX:
    for npz in ('jpeg_fixtures.npz', 'jpeg_parallel_fixtures.npz'):
      fx = np.load(os.path.join(ROOT, 'tests', 'golden', npz))
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


def _slots_equal(a, b, offsets, sizes):
  """torch.equal on every byte of the two output buffers that the call defines: the images' slots (the few bytes that
  pad a slot to 16 are never written by either path)"""
  used = torch.zeros(a.numel(), dtype=torch.bool, device=a.device)
  for o, (h, w) in zip(offsets, sizes):
    used[int(o):int(o) + h * w * 3] = True
  return a.shape == b.shape and torch.equal(a[used], b[used])


_REF = {}


def _reference_coefficients(name, f):
  if name not in _REF:
    _REF[name] = np.concatenate([c.reshape(-1) for c in jpeg_ref.coefficients(f)[0]])
  return _REF[name]


@pytest.mark.parametrize('segment_bytes', [16, None])
def test_every_fixture_in_one_ragged_launch(product, segment_bytes):
  from assembled_cnn_amd import jpeg
  segment_bytes = jpeg.DEFAULT_SEGMENT_BYTES if segment_bytes is None else segment_bytes
  fx = device_fixtures()
  pk = jpeg.pack([f for _, f, _ in fx], segment_bytes=segment_bytes)
  assert len(pk.dev_index) == len(fx) >= 46
  dst, status, ws, info = jpeg.decode_packed(pk, 'cuda', return_workspace=True, entropy='parallel', return_info=True)
  assert status.tolist() == [0] * len(fx)
  for (name, _, pix), got in zip(fx, _images(dst, pk.offsets, pk.sizes)):
    assert got.shape == pix.shape and np.array_equal(got, pix), name
  coefs = ws.cpu().numpy()[:pk.total_blocks * 128].view('<i2')
  for (name, f, _), d in zip(fx, pk.descs):
    want = _reference_coefficients(name, f)
    got = coefs[int(d['coef_offset']):int(d['coef_offset']) + want.size]
    assert np.array_equal(got, want), name
  sequential = jpeg.decode_packed(pk, 'cuda')[0]
  assert _slots_equal(dst, sequential, pk.offsets, pk.sizes)
  # the two entry points on one pack and on output buffers filled beforehand: the buffers are torch.equal as they
  # stand, and neither path has written outside the images' slots
  from assembled_cnn_amd.staging import upload_table
  tabs = [upload_table(t, 'cuda') for t in (pk.files, pk.descs, pk.tables, pk.intervals)]
  out_s = torch.full((pk.total_bytes,), 0xA5, dtype=torch.uint8, device='cuda')
  out_p = out_s.clone()
  sizes = (pk.total_blocks, pk.max_blocks, pk.max_pixels)
  st_s, _ = product.jpeg_decode(*tabs, len(fx), len(pk.intervals), *sizes, out_s)
  st_p, _ = product.jpeg_decode_parallel(*tabs, upload_table(pk.segment_first, 'cuda'), len(fx), len(pk.intervals),
                                         pk.total_segments, segment_bytes, *sizes, out_p)
  assert torch.equal(st_p, st_s) and torch.equal(out_p, out_s)
  used = torch.zeros(pk.total_bytes, dtype=torch.bool, device='cuda')
  for o, (h, w) in zip(pk.offsets, pk.sizes):
    used[int(o):int(o) + h * w * 3] = True
  assert bool((out_p[~used] == 0xA5).all()) and _slots_equal(out_p, dst, pk.offsets, pk.sizes)
  # info: segments and rounds per image
  info = info.cpu().numpy()
  names = [n for n, _, _ in fx]
  first = np.concatenate([pk.segment_first, [pk.total_segments]])
  for row, d in enumerate(pk.descs):
    lo, hi = int(d['first_interval']), int(d['first_interval']) + int(d['n_intervals'])
    assert info[row, 0] == first[hi] - first[lo], names[row]
  print('\n'.join('%s: %d segments, %d rounds' % (n, s, r) for n, (s, r) in zip(names, info.tolist())))
  assert np.all(info[:, 1] >= 1) and np.all(info[:, 1] <= info[:, 0] + 1)
  if segment_bytes == 16:
    assert info[names.index(BIG), 0] > 2 * LANES       # several passes of the workgroup over its segments
    assert info[names.index('noise_17x33_444'), 1] > 1 and info[:, 1].max() >= 12


def test_single_image_batches_and_seventy(product):
  from assembled_cnn_amd import jpeg
  for name in ('noise_1x1_420', 'rst1_444_noise_72x72', 'grey_13x17'):
    _, f, pix = fixtures()[name]
    for sb in (16, None):
      buf, offsets, sizes = jpeg.decode_batch([f], 'cuda', entropy='parallel', segment_bytes=sb)
      assert sizes == [pix.shape[:2]] and np.array_equal(_images(buf, offsets, sizes)[0], pix), name
  fx = device_fixtures()
  batch = [fx[k % len(fx)] for k in range(70)]
  files = [f if k % 3 == 0 else bytearray(f) if k % 3 == 1 else np.frombuffer(f, np.uint8) for k, (_, f, _) in enumerate(batch)]
  buf, offsets, sizes = jpeg.decode_batch(files, 'cuda', entropy='parallel', segment_bytes=16)
  for (name, _, pix), got in zip(batch, _images(buf, offsets, sizes)):
    assert np.array_equal(got, pix), name


@pytest.mark.parametrize('is_training', [False, True])
def test_mixed_batch_through_preprocess_batch(product, is_training):
  """progressive rows, a fallback entry (CMYK) and a decoded array beside sequential files"""
  from assembled_cnn_amd import input_pipeline as ip, jpeg
  fxs = fixtures()
  stand_in = np.arange(16 * 16 * 3, dtype=np.uint8).reshape(16, 16, 3)
  calls = []

  def fallback(data):
    calls.append(data)
    return stand_in

  entries = [fxs['smooth_17x33_420'][1], fxs['progressive_16x16'][1], fxs[BIG][1], fxs['opt_444_24x20'][2],
             fxs['cmyk_16x16'][1], fxs['rstrow_tex_120x80_420'][1], fxs['stuffed_noise_32x24_444'][1]]
  pk = jpeg.pack(entries, fallback, progressive=True)
  rng = np.random.default_rng(11)
  side = 16
  windows = [ip.train_window(h, w, side, side, rng) if is_training else ip.eval_window(h, w, side, side) for h, w in pk.sizes]
  kw = dict(is_training=is_training, device='cuda', image_size=side, windows=windows, jpeg_fallback=fallback,
            jpeg_progressive=True)
  want = ip.preprocess_batch(entries, **kw)
  got = ip.preprocess_batch(entries, jpeg_entropy='parallel', **kw)
  assert len(calls) == 3 and got.shape == (len(entries), side, side, 3)
  assert torch.equal(got, want)
  buf, offsets, sizes = jpeg.decode_batch([e for e in entries if not isinstance(e, np.ndarray)], 'cuda', fallback=fallback,
                                          progressive=True, entropy='parallel')
  seq = jpeg.decode_batch([e for e in entries if not isinstance(e, np.ndarray)], 'cuda', fallback=fallback, progressive=True)
  assert np.array_equal(offsets, seq[1]) and sizes == seq[2] and _slots_equal(buf, seq[0], offsets, sizes)


def test_corrupt_scans_give_the_sequential_status_zero_pixels_and_the_same_value_error(product):
  """The error path, not a fault: every input is one tools/probes/jpeg_parallel_host.cpp runs under the sanitizers (the
  host parser ends both damaged files' scans at the marker: a truncation of that scan)."""
  from assembled_cnn_amd import jpeg
  _, other, other_pix = fixtures()['smooth_13x17_444']
  files = [other]
  for name in ('noise_17x33_420', BIG):
    _, good, _ = fixtures()[name]
    info = jpeg.parse(good)
    mid = (info.scan_begin + info.scan_end) // 2
    a = bytearray(good)
    a[mid], a[mid + 1] = 0xFF, 0xD9
    files += [good[:mid] + b'\xff\xd9', bytes(a)]
  files.append(other)
  for sb in (16, jpeg.DEFAULT_SEGMENT_BYTES):
    pk = jpeg.pack(files, segment_bytes=sb)
    want = jpeg.decode_packed(pk, 'cuda', check=False)[1].cpu().tolist()
    dst, status = jpeg.decode_packed(pk, 'cuda', check=False, entropy='parallel')
    assert status.cpu().tolist() == want and want[0] == want[5] == 0 and all(want[1:5])
    out = _images(dst, pk.offsets, pk.sizes)
    assert np.array_equal(out[0], other_pix) and np.array_equal(out[5], other_pix)
    assert not any(o.any() for o in out[1:5])
  with pytest.raises(ValueError) as sequential:
    jpeg.decode_batch(files, 'cuda')
  with pytest.raises(ValueError) as parallel:
    jpeg.decode_batch(files, 'cuda', entropy='parallel')
  assert str(parallel.value) == str(sequential.value) and 'entries [1, 2, 3, 4]' in str(parallel.value)


def test_argument_checks(product):
  from assembled_cnn_amd import jpeg, lib
  from assembled_cnn_amd.staging import upload_table
  _, f, _ = fixtures()['grey_13x17']
  pk = jpeg.pack([f], segment_bytes=16)
  dev = torch.device('cuda')
  tabs = [upload_table(t, dev) for t in (pk.files, pk.descs, pk.tables, pk.intervals, pk.segment_first)]
  dst = torch.empty(pk.total_bytes, dtype=torch.uint8, device=dev)
  for bad in (0, 8, 24, 131072):
    with pytest.raises(ValueError, match='segment_bytes'):
      product.jpeg_decode_parallel(*tabs, 1, len(pk.intervals), pk.total_segments, bad, pk.total_blocks, pk.max_blocks,
                                   pk.max_pixels, dst)
    with pytest.raises(ValueError, match='segment_bytes'):
      jpeg.pack([f], segment_bytes=bad)
  L = lib.load()
  status = torch.zeros(1, dtype=torch.int32, device=dev)
  ws = torch.empty(pk.total_blocks * 192 + pk.total_segments * 32, dtype=torch.uint8, device=dev)
  args = lambda n, ws_bytes: (tabs[0].data_ptr(), tabs[0].numel(), tabs[1].data_ptr(), tabs[2].data_ptr(), tabs[3].data_ptr(),
                              tabs[4].data_ptr(), n, len(pk.intervals), pk.total_segments, 16, pk.total_blocks, pk.max_blocks,
                              pk.max_pixels, dst.data_ptr(), dst.numel(), status.data_ptr(), None, ws.data_ptr(), ws_bytes, 3,
                              None)
  assert L.asm_jpeg_decode_parallel(*args(1, ws.numel() - 1)) == lib.ASM_EINVAL
  assert b'workspace too small' in L.asm_last_error()
  assert L.asm_jpeg_decode_parallel(*args(0, ws.numel())) == lib.ASM_OK
  st, w = product.jpeg_decode_parallel(*(t[:0] for t in tabs), 0, 0, 0, 16, 0, 0, 0, dst)
  assert st.numel() == 0 and w is None
