"""Files for the tests of the device JPEG header parser (asm_jpeg_parse): the device fixtures of the three .npz files and
header variants made from them by byte surgery.  jpeg.parse / jpeg.pack are the oracle: ``expected(data)`` says whether a
file is one the device path takes.  No Pillow, nothing outside the tree."""
import os

import numpy as np

from assembled_cnn_amd import jpeg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BASE = 'noise_13x17_420'        # the fixture the variants are cut from: three components, four DHT segments, two DQT


def load():
  """{name: (bytes, kind, recorded pixels)} of jpeg_fixtures.npz, jpeg_parallel_fixtures.npz and jpeg_parse_fixtures.npz"""
  out = {}
  for f in ('jpeg_fixtures.npz', 'jpeg_parallel_fixtures.npz', 'jpeg_parse_fixtures.npz'):
    z = np.load(os.path.join(GOLDEN, f))
    for n in z['names']:
      out[str(n)] = (z['file_' + n].tobytes(), str(z['kind_' + n]), z['pix_' + n] if 'pix_' + n in z.files else None)
  return out


def segments(data):
  """[(marker byte, position of its FF, position behind the segment)] from SOI to the SOS header of a well-formed file"""
  out, at = [], 2
  while True:
    m, size = data[at + 1], (data[at + 2] << 8) | data[at + 3]
    out.append((m, at, at + 2 + size))
    if m == 0xDA:
      return out
    at += 2 + size


def _seg(marker, body):
  return bytes([0xFF, marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + bytes(body)


def _huffman_tables(data):
  """[(class << 4 | id, 16 counts, symbols)] of every DHT segment, in file order"""
  tables = []
  for m, a, e in segments(data):
    p = a + 4
    while m == 0xC4 and p < e:
      cnt = sum(data[p + 1:p + 17])
      tables.append((data[p], data[p + 1:p + 17], data[p + 17:p + 17 + cnt]))
      p += 17 + cnt
  return tables


def _regroup_dht(data, merged):
  """every Huffman table in ONE DHT segment (merged) or in a segment of its own, where the first DHT segment stood"""
  tables = _huffman_tables(data)
  dht = [(a, e) for m, a, e in segments(data) if m == 0xC4]
  bodies = [bytes([t]) + bits + vals for t, bits, vals in tables]
  new = _seg(0xC4, b''.join(bodies)) if merged else b''.join(_seg(0xC4, b) for b in bodies)
  out, at = b'', 0
  for k, (a, e) in enumerate(dht):
    out += data[at:a] + (new if k == 0 else b'')
    at = e
  return out + data[at:]


def _adobe(transform):
  return _seg(0xEE, b'Adobe' + bytes([0, 100, 0, 0, 0, 0, transform]))


def variants(files):
  """{name: bytes}: the header edits of the parser's tests"""
  d = files[BASE][0]
  seg = segments(d)
  sof = next(a for m, a, e in seg if m == 0xC0)
  sos = next(a for m, a, e in seg if m == 0xDA)
  dqt = next(a for m, a, e in seg if m == 0xDB)
  second = seg[1][1]
  v = {}
  v['com_behind_soi'] = d[:2] + _seg(0xFE, b'a comment') + d[2:]
  v['fill_bytes'] = d[:second] + b'\xff\xff' + d[second:-2] + b'\xff\xff\xff' + d[-2:]
  # segments and fill longer than the parser's 4096-byte window
  v['long_app1'] = d[:2] + _seg(0xE1, bytes(range(256)) * 20) + d[2:]
  v['long_fill'] = d[:second] + b'\xff' * 5000 + d[second:]
  v['adobe_transform_1'] = d[:2] + _adobe(1) + d[2:]
  v['sof1'] = d[:sof + 1] + b'\xc1' + d[sof + 2:]
  v['bytes_behind_eoi'] = d + b'\x00\x01 trailing \xff\xd8\xff\xda'
  v['adobe_transform_0'] = d[:2] + _adobe(0) + d[2:]
  v['sof2'] = d[:sof + 1] + b'\xc2' + d[sof + 2:]
  v['no_eoi'] = d[:-2]
  v['ends_in_ff'] = d[:-2] + b'\xff'
  v['cut_at_100'] = d[:100]
  v['empty'] = b''
  v['one_byte'] = b'\xff'
  v['zeros'] = bytes(64)
  # a table the file defines again later: the later one counts
  v['dht_redefined'] = d[:2] + _seg(0xC4, bytes([0x00, 0, 1] + [0] * 14 + [5])) + d[2:]
  v['dht_merged'] = _regroup_dht(d, True)
  v['dht_split'] = _regroup_dht(_regroup_dht(d, True), False)
  wide = b''.join(bytes([0, x]) for x in d[dqt + 5:dqt + 69])
  v['dqt_16bit'] = d[:dqt] + _seg(0xDB, bytes([0x10 | d[dqt + 4]]) + wide) + d[dqt + 69:]
  rgb = bytearray(d)
  for k, c in enumerate(b'RGB'):
    rgb[sof + 10 + 3 * k] = c
    rgb[sos + 5 + 2 * k] = c
  v['rgb_ids'] = bytes(rgb)
  v['dht_unused_id_3'] = d[:sos] + _seg(0xC4, bytes([0x03, 0, 2] + [0] * 14 + [7, 9])) + d[sos:]
  v['cmyk_16x16'] = files['cmyk_16x16'][0]
  v['progressive_16x16'] = files['progressive_16x16'][0]
  return v


ACCEPTED_VARIANTS = ('com_behind_soi', 'fill_bytes', 'long_app1', 'long_fill', 'adobe_transform_1', 'sof1', 'bytes_behind_eoi', 'dht_redefined',
                     'dht_merged', 'dht_split', 'dht_unused_id_3')


def expected(data):
  """True where jpeg.parse neither raises nor calls the file unsupported"""
  try:
    return jpeg.parse(data).unsupported is None
  except ValueError:
    return False


def error_of(data):
  """what jpeg.parse raises for the file, as text (None when it returns)"""
  try:
    jpeg.parse(data)
    return None
  except ValueError as e:
    return str(e)
