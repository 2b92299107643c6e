"""Host side of the JPEG decoder without a GPU: the numpy reference against the recorded Pillow pixels, jpeg.parse's
header reading and classification, the packing of the device tables."""
import ctypes
import io
import os

import numpy as np
import pytest

from assembled_cnn_amd import jpeg, lib
from tests import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FX = {}


def fixtures():
  if not _FX:
    fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_fixtures.npz'))
    for name in fx['names']:
      name = str(name)
      kind = str(fx['kind_' + name])
      _FX[name] = (kind, fx['file_' + name].tobytes(), fx['pix_' + name] if kind == 'device' else None)
  return _FX


def device_fixtures():
  return [(n, f, p) for n, (k, f, p) in fixtures().items() if k == 'device']


def test_fixture_file_is_small_and_complete():
  assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'jpeg_fixtures.npz')) < 256 * 1024
  names = set(fixtures())
  for size in ('1x1', '8x8', '13x17', '31x9', '17x33'):
    for sub in ('444', '422', '420'):
      assert {'smooth_%s_%s' % (size, sub), 'noise_%s_%s' % (size, sub)} <= names
  assert len(device_fixtures()) >= 39


def test_reference_decoder_equals_the_recorded_pillow_pixels():
  longest, stuffed = 0, 0
  for name, f, pix in device_fixtures():
    assert np.array_equal(jpeg_ref.decode(f), pix), name
    st = jpeg_ref.stats(f)
    longest, stuffed = max(longest, st['max_code_length']), stuffed + st['stuffed']
  assert longest == 16 and stuffed > 0      # the set reaches the slow Huffman path and byte stuffing


def test_idct_shortcut_is_no_different():
  """a block with only a DC coefficient: the all-zero-AC shortcut of libjpeg, (dc * q + 4) >> 3, is what the full
  two-pass arithmetic gives"""
  q = np.full(64, 3, np.int64)
  for dc in (-1024, -77, -1, 0, 1, 5, 300, 1023):
    c = np.zeros((1, 1, 64), np.int16)
    c[0, 0, 0] = dc
    want = np.clip(((dc * 3 + 4) >> 3) + 128, 0, 255)
    assert (jpeg_ref.idct_plane(c, q) == want).all(), dc


def test_upsampling_rules_on_a_hand_worked_plane():
  p = np.array([[10, 20, 40], [50, 70, 90]], np.uint8)
  h = jpeg_ref.upsample_h2v1(p)
  assert h[0].tolist() == [10, (30 + 20 + 2) >> 2, (60 + 10 + 1) >> 2, (60 + 40 + 2) >> 2, (120 + 20 + 1) >> 2, 40]
  v = jpeg_ref.upsample_h2v2(p)
  s0 = [3 * 10 + 10, 3 * 20 + 20, 3 * 40 + 40]        # the top row replicates itself
  assert v[0].tolist() == [(4 * s0[0] + 8) >> 4, (3 * s0[0] + s0[1] + 7) >> 4, (3 * s0[1] + s0[0] + 8) >> 4,
                           (3 * s0[1] + s0[2] + 7) >> 4, (3 * s0[2] + s0[1] + 8) >> 4, (4 * s0[2] + 7) >> 4]
  s1 = [3 * 10 + 50, 3 * 20 + 70, 3 * 40 + 90]        # output row 1: the row below weighs 1
  assert v[1, :2].tolist() == [(4 * s1[0] + 8) >> 4, (3 * s1[0] + s1[1] + 7) >> 4]
  # planes of one or two columns are replicated, not interpolated
  assert jpeg_ref.upsample_h2v1(p[:, :2])[0].tolist() == [10, 10, 20, 20]


def test_parse_geometry_sampling_tables_and_intervals():
  fx = fixtures()
  want = {  # name: (width, height, ncomp, hs, vs, restart interval, intervals)
      'noise_1x1_420': (1, 1, 3, 2, 2, 0, 1), 'smooth_13x17_422': (13, 17, 3, 2, 1, 0, 1),
      'noise_31x9_444': (31, 9, 3, 1, 1, 0, 1), 'grey_13x17': (13, 17, 1, 1, 1, 0, 1),
      'rst1_grey_40x48': (40, 48, 1, 1, 1, 1, 30), 'rst1_444_40x48': (40, 48, 3, 1, 1, 1, 30),
      'rst1_444_noise_72x72': (72, 72, 3, 1, 1, 1, 81), 'rstrow_420_48x64': (48, 64, 3, 2, 2, 3, 4),
      'rst2_422_33x47': (33, 47, 3, 2, 1, 2, 9), 'flat_20x20': (20, 20, 3, 2, 2, 0, 1)}
  for name, (w, h, nc, hs, vs, ri, ni) in want.items():
    data = fx[name][1]
    info = jpeg.parse(data)
    assert info.unsupported is None, name
    assert (info.width, info.height, info.ncomp, info.hs, info.vs, info.restart_interval, len(info.intervals)) == (
        w, h, nc, hs, vs, ri, ni), name
    assert info.mcus_x == -(-w // (8 * hs)) and info.mcus_y == -(-h // (8 * vs))
    # against the reference's own header reader
    hdr = jpeg_ref.read_header(data)
    assert info.scan_begin == hdr['scan_begin'] and data[info.scan_end:] == b'\xff\xd9'
    for tq, q in hdr['q'].items():
      assert np.array_equal(info.qtables[tq], q), name
    for key, (counts, vals) in hdr['huff'].items():
      assert info.huffman[key][0].tolist() == counts and info.huffman[key][1].tolist() == vals, name
    # the intervals tile the scan, two marker bytes apart, and the markers count 0..7 round and round
    iv = info.intervals
    assert iv[0, 0] == info.scan_begin and iv[-1, 1] == info.scan_end and (iv[1:, 0] - iv[:-1, 1] == 2).all()
    assert info.rst.tolist() == [k & 7 for k in range(ni - 1)]
    for k in range(ni - 1):
      assert data[iv[k, 1]] == 0xFF and data[iv[k, 1] + 1] == 0xD0 + (k & 7)
  assert len(jpeg.parse(fx['rst1_grey_40x48'][1]).rst) > 8       # RSTm wraps


def test_parse_accepts_bytes_bytearray_and_uint8_arrays():
  f = fixtures()['smooth_8x8_444'][1]
  for form in (f, bytearray(f), np.frombuffer(f, np.uint8), memoryview(f)):
    assert jpeg.is_encoded(form) and jpeg.parse(form).width == 8
  assert not jpeg.is_encoded(np.zeros((8, 8, 3), np.uint8))
  with pytest.raises(ValueError):
    jpeg.parse(np.zeros(8, np.int32))


def _with_segment(f, marker, payload, before=0xDA):
  """insert a marker segment in front of the first `before` marker"""
  at = f.index(bytes([0xFF, before]))
  return f[:at] + bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + payload + f[at:]


def test_unsupported_kinds_are_classified_and_go_to_the_fallback():
  fx = fixtures()
  good = fx['smooth_13x17_444'][1]
  cases = {'progressive': fx['progressive_16x16'][1], 'CMYK': fx['cmyk_16x16'][1], 'not a JPEG': b'\x89PNG\r\n\x1a\n' + bytes(32),
           'arithmetic': _with_segment(good, 0xCC, b'\x00\x10'),
           'DNL': _with_segment(good, 0xDC, b'\x00\x11'),
           'Adobe': _with_segment(good, 0xEE, b'Adobe\x00\x64\x00\x00\x00\x00\x00'),
           '16-bit': _with_segment(good, 0xDB, b'\x12' + b'\x00\x09' * 64)}
  sof = good.index(b'\xff\xc0')
  a = bytearray(good)
  a[sof + 11] = 0x12                                     # luma sampling 1x2
  cases['sampling'] = bytes(a)
  a = bytearray(good)
  a[sof + 4] = 12                                        # sample precision
  cases['12-bit'] = bytes(a)
  a = bytearray(good)
  for k, cid in enumerate(b'RGB'):                       # component ids R, G, B, in the frame and the scan header
    a[sof + 10 + 3 * k] = cid
  sos = good.index(b'\xff\xda')
  for k, cid in enumerate(b'RGB'):
    a[sos + 5 + 2 * k] = cid
  cases['RGB'] = bytes(a)
  cases['several scans'] = good[:-2] + good[sos:]        # a second scan after the first
  for what, data in cases.items():
    info = jpeg.parse(data)
    assert info.unsupported is not None and what.lower()[:6] in info.unsupported.lower().replace('4 components / ', ''), (
        what, info.unsupported)
    with pytest.raises(NotImplementedError, match='entry 1'):
      jpeg.pack([good, data])
    seen = []
    stand_in = np.zeros((5, 7, 3), np.uint8)
    pk = jpeg.pack([good, data, good], fallback=lambda b: (seen.append(b), stand_in)[1])
    assert seen == [data] and pk.dev_index == [0, 2] and pk.fallback[1] is stand_in
    assert pk.sizes == [(17, 13), (5, 7), (17, 13)]
  # a fallback that returns something else than uint8 [H, W, 3] is an error
  with pytest.raises(ValueError):
    jpeg.pack([cases['progressive']], fallback=lambda b: np.zeros((4, 4), np.uint8))
  # comment and application segments are skipped
  ok = jpeg.parse(_with_segment(_with_segment(good, 0xFE, b'hello'), 0xE1, b'Exif\x00\x00' + bytes(20)))
  assert ok.unsupported is None and ok.width == 13
  assert jpeg.parse(_with_segment(good, 0xEE, b'Adobe\x00\x64\x00\x00\x00\x00\x01')).unsupported is None


def test_malformed_headers_raise_value_error():
  good = fixtures()['smooth_13x17_420'][1]
  info = jpeg.parse(good)
  bad = {}
  for cut in (3, 10, good.index(b'\xff\xc4') + 7, good.index(b'\xff\xc0') + 6, info.scan_begin - 3, info.scan_begin + 5,
              len(good) - 2):
    bad['cut at %d' % cut] = good[:cut]
  dht = good.index(b'\xff\xc4')
  a = bytearray(good)
  a[dht + 5 + 3] = 200                                   # more symbols than the segment holds
  bad['DHT counts'] = bytes(a)
  a = bytearray(good)
  a[dht + 5] = 3                                         # three codes of one bit
  bad['DHT overflow'] = bytes(a)
  a = bytearray(good)
  a[dht + 4] = 0x25                                      # table class 2
  bad['DHT class'] = bytes(a)
  dqt = good.index(b'\xff\xdb')
  a = bytearray(good)
  a[dqt + 4] = 0x07                                      # quantisation table id 7
  bad['DQT id'] = bytes(a)
  sof = good.index(b'\xff\xc0')
  a = bytearray(good)
  a[sof + 9] = 2                                         # two components in an 17-byte frame header
  bad['SOF count'] = bytes(a)
  a = bytearray(good)
  a[sof + 12] = 3                                        # a quantisation table nobody defined
  bad['undefined DQT'] = bytes(a)
  sos = good.index(b'\xff\xda')
  a = bytearray(good)
  a[sos + 5] = 9                                         # a scan component the frame does not have
  bad['SOS component'] = bytes(a)
  a = bytearray(good)
  a[sos + 6] = 0x22                                      # Huffman tables nobody defined
  bad['undefined DHT'] = bytes(a)
  bad['garbage between segments'] = good[:dqt] + b'\x00\x01' + good[dqt:]
  for what, data in bad.items():
    try:
      jpeg.parse(data)
    except ValueError:
      continue
    pytest.fail('%s was accepted' % what)


def test_descriptor_packing_round_trips():
  fx = device_fixtures()
  decoded = np.zeros((9, 11, 3), np.uint8)
  entries = [f for _, f, _ in fx] + [decoded]
  pk = jpeg.pack(entries)
  n = len(fx)
  assert pk.descs.tobytes().__len__() == 96 * n and pk.tables.tobytes().__len__() == 1600 * n
  assert pk.intervals.tobytes().__len__() == 32 * len(pk.intervals)
  descs = (lib.JpegDesc * n).from_buffer_copy(pk.descs.tobytes())
  tables = (lib.JpegTables * n).from_buffer_copy(pk.tables.tobytes())
  rows = (lib.JpegInterval * len(pk.intervals)).from_buffer_copy(pk.intervals.tobytes())
  blocks = 0
  for k, (name, f, pix) in enumerate(fx):
    d, info = descs[k], jpeg.parse(f)
    assert (d.width, d.height, d.ncomp, d.hs, d.vs, d.mcus_x, d.mcus_y, d.restart_interval, d.n_intervals) == (
        info.width, info.height, info.ncomp, info.hs, info.vs, info.mcus_x, info.mcus_y, info.restart_interval,
        len(info.intervals)), name
    assert d.scan_offset % 16 == 0 and d.dst_offset % 16 == 0 and d.dst_offset == pk.offsets[k]
    assert d.coef_offset == d.plane_offset == blocks * 64
    blocks += info.n_blocks
    scan = f[info.scan_begin:info.scan_end]
    assert pk.files[d.scan_offset:d.scan_offset + d.scan_bytes].tobytes() == scan
    for c, ((_, _, _, tq), (_, td, ta)) in enumerate(zip(info.components, info.scan_components)):
      assert list(tables[k].quant[d.qsel[c]]) == info.qtables[tq].tolist()
      for slot, key in ((tables[k].dc[d.dcsel[c]], (0, td)), (tables[k].ac[d.acsel[c]], (1, ta))):
        bits, vals = info.huffman[key]
        assert list(slot.bits) == bits.tolist() and list(slot.vals)[:vals.size] == vals.tolist()
    for j in range(d.n_intervals):
      r = rows[d.first_interval + j]
      ri = d.restart_interval
      assert r.image == k and r.first_mcu == j * ri and r.rst == (-1 if j == d.n_intervals - 1 else j & 7)
      assert r.n_mcus == (min(ri, info.n_mcus - j * ri) if ri else info.n_mcus)
      assert pk.files[r.byte_begin:r.byte_end].tobytes() == f[info.intervals[j, 0]:info.intervals[j, 1]]
  assert pk.total_blocks == blocks and pk.max_blocks == max(jpeg.parse(f).n_blocks for _, f, _ in fx)
  assert pk.max_pixels == 72 * 72
  # every entry, decoded ones included, has a 16-byte aligned slot of its own size
  ends = [int(o) + h * w * 3 for o, (h, w) in zip(pk.offsets, pk.sizes)]
  assert pk.sizes[-1] == (9, 11) and pk.fallback[n] is decoded
  assert all(o % 16 == 0 for o in pk.offsets) and all(e <= o for e, o in zip(ends, pk.offsets[1:]))
  assert pk.total_bytes >= ends[-1]
  assert ctypes.sizeof(lib.JpegDesc) == 96 and ctypes.sizeof(lib.JpegTables) == 1600 and ctypes.sizeof(lib.JpegInterval) == 32


def test_dct_method_names():
  jpeg.check_dct_method('')
  jpeg.check_dct_method('INTEGER_ACCURATE')
  with pytest.raises(NotImplementedError):
    jpeg.check_dct_method('INTEGER_FAST')
  with pytest.raises(ValueError):
    jpeg.check_dct_method('FLOAT')


def test_reference_decoder_equals_pillow_on_fresh_files():
  """A few hundred files generated here: every sampling layout, grey, qualities 30..100, optimised tables, restart
  intervals, widths and heights 1..40 (chroma planes of one and two columns among them)."""
  Image = pytest.importorskip('PIL.Image')
  rng = np.random.default_rng(5)
  count = 0
  for k in range(240):
    w, h = (int(rng.integers(1, 7)), int(rng.integers(1, 41))) if k % 6 == 0 else (int(rng.integers(1, 41)), int(rng.integers(1, 41)))
    if k % 2:
      arr = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    else:
      y, x = np.mgrid[0:h, 0:w]
      arr = np.stack([(x * (3 + c) + y * (5 - c) + 40 * c) % 256 for c in range(3)], axis=-1).astype(np.uint8)
    kw = dict(quality=int(rng.integers(30, 101)), optimize=bool(k % 5 == 0))
    if k % 7 == 0:
      kw['restart_marker_blocks'] = int(rng.integers(1, 4))
    if k % 9 == 0:
      im = Image.fromarray(arr[..., 0], 'L')
    else:
      im = Image.fromarray(arr, 'RGB')
      kw['subsampling'] = k % 3
    buf = io.BytesIO()
    im.save(buf, 'JPEG', **kw)
    data = buf.getvalue()
    want = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
    assert np.array_equal(jpeg_ref.decode(data), want), (k, w, h, kw)
    assert jpeg.parse(data).unsupported is None
    count += 1
  assert count == 240
