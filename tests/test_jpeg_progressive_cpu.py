"""Host side of the progressive JPEG path without a GPU: the numpy reference against the recorded Pillow pixels, the
re-coded files against the baseline pixels, jpeg.parse(progressive=True)'s scan reading and its rejection rules, the
packing of the second group of device tables."""
import ctypes
import os
import re

import numpy as np
import pytest

from assembled_cnn_amd import jpeg, lib
from tests import jpeg_progressive_ref as ref
from tests import jpeg_progressive_writer as writer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FX, _BASE = {}, {}


def fixtures():
  """name -> (file bytes, recorded pixels), loaded once"""
  if not _FX:
    fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_progressive_fixtures.npz'))
    for name in fx['names']:
      _FX[str(name)] = (fx['file_' + str(name)].tobytes(), fx['pix_' + str(name)])
  return _FX


def baseline():
  """the sequential fixtures the device decodes: name -> (file bytes, recorded pixels)"""
  if not _BASE:
    fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_fixtures.npz'))
    for name in fx['names']:
      if str(fx['kind_' + str(name)]) == 'device':
        _BASE[str(name)] = (fx['file_' + str(name)].tobytes(), fx['pix_' + str(name)])
  return _BASE


def test_parse_with_the_flag_reads_the_scans_as_the_reference_does():
  for name, (f, pix) in fixtures().items():
    info = jpeg.parse(f, progressive=True)
    assert info.unsupported is None and info.progressive, (name, info.unsupported)
    assert (info.height, info.width) == pix.shape[:2]
    h = ref.read_scans(f)
    assert len(info.scans) == len(h['scans'])
    for got, want in zip(info.scans, h['scans']):
      assert (got.components, got.ss, got.se, got.ah, got.al, got.restart_interval, got.begin, got.end) == (
          want['comps'], want['ss'], want['se'], want['ah'], want['al'], want['ri'], want['begin'], want['end']), name
      # the intervals tile the scan: ceil(scan MCUs / DRI) of them, RSTm counting from 0 in every scan
      ri, mcus = got.restart_interval, got.n_mcus(info)
      assert len(got.intervals) == (-(-mcus // ri) if ri else 1), name
      assert got.rst.tolist() == [k & 7 for k in range(len(got.intervals) - 1)]
      assert got.intervals[0, 0] == got.begin and got.intervals[-1, 1] == got.end
      assert np.all(got.intervals[1:, 0] == got.intervals[:-1, 1] + 2)


def test_fixture_file_is_small_and_complete():
  assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'jpeg_progressive_fixtures.npz')) < 256 * 1024
  names = set(fixtures())
  for size in ('1x1', '8x8', '9x7', '13x17', '31x9', '17x33'):
    for sub in ('444', '422', '420'):
      assert {'smooth_%s_%s' % (size, sub), 'noise_%s_%s' % (size, sub)} <= names
  assert {'smooth_3x5_420', 'noise_4x3_422', 'grey_13x17', 'flat_grey_72x72', 'rst1_grey_40x48', 'rst2_422_33x47',
          'rstrow_422_48x40', 'noopt_420_31x29'} <= names
  kinds = set()
  for f, _ in fixtures().values():
    kinds |= set((sc['ss'] > 0, sc['ah'] > 0) for sc in ref.read_scans(f)['scans'])
  assert len(kinds) == 4      # DC first, DC refinement, AC first, AC refinement


def test_reference_decoder_equals_the_recorded_pillow_pixels():
  for name, (f, pix) in fixtures().items():
    assert np.array_equal(ref.decode(f), pix), name


def test_named_fixtures_have_the_geometry_they_are_there_for():
  fx = fixtures()
  # DRI changes between the scans of a restart_marker_rows file: 6 MCUs per row of the interleaved DC scan, 6 and 3 blocks
  # per row of the luma and chroma scans
  info = jpeg.parse(fx['rstrow_422_48x40'][0], progressive=True)
  assert (info.hs, info.vs, info.mcus_x, info.mcus_y) == (2, 1, 3, 5)
  assert sorted(set(sc.restart_interval for sc in info.scans)) == [3, 6]
  for sc in info.scans:
    assert sc.restart_interval == (3 if len(sc.components) > 1 or sc.components[0] > 0 else 6)
    assert len(sc.intervals) == 5
  # one block per interval: 30 intervals in every scan of the grey file, so RSTm wraps
  info = jpeg.parse(fx['rst1_grey_40x48'][0], progressive=True)
  assert all(len(sc.intervals) == 30 and sc.restart_interval == 1 for sc in info.scans)
  # a scan of one component walks its true grid: 9x7 at 4:2:0 has a 2x1 luma grid padded to 2x2, and one chroma block
  info = jpeg.parse(fx['smooth_9x7_420'][0], progressive=True)
  assert (info.mcus_x, info.mcus_y, info.n_blocks) == (1, 1, 6)
  assert sorted(set((len(sc.components), sc.components[0], sc.n_mcus(info)) for sc in info.scans)) == [
      (1, 0, 2), (1, 1, 1), (1, 2, 1), (3, 0, 1)]
  # 17x33 at 4:2:2: luma 3 x 5 true blocks in a 4 x 5 padded grid
  info = jpeg.parse(fx['noise_17x33_422'][0], progressive=True)
  assert [sc.n_mcus(info) for sc in info.scans if sc.components == [0]][0] == 15 and info.n_mcus == 10


def test_recoded_files_decode_to_the_baseline_pixels():
  for name, (f, pix) in baseline().items():
    for script in writer.SCRIPTS:
      data = writer.recode(f, script)
      info = jpeg.parse(data, progressive=True)
      assert info.unsupported is None, (name, script, info.unsupported)
      assert all(sc.ah == 0 and sc.al == 0 for sc in info.scans)
      assert np.array_equal(ref.decode(data), pix), (name, script)
  bands = [(sc.ss, sc.se) for sc in info.scans if sc.components == [0]]
  assert bands == [(0, 0), (1, 5), (6, 20), (21, 63)]


def test_without_the_flag_a_progressive_file_is_classified_as_before():
  f = fixtures()['smooth_17x33_420'][0]
  for info in (jpeg.parse(f), jpeg.parse(f, progressive=False)):
    assert info.unsupported == 'progressive (SOF2)' and info.scans is None and not info.progressive
  with pytest.raises(NotImplementedError, match=r'entry 1: progressive \(SOF2\) is not decoded on the device'):
    jpeg.pack([baseline()['smooth_17x33_420'][0], f])
  # a sequential file reads the same either way
  for name, (g, _) in list(baseline().items())[:6]:
    a, b = jpeg.parse(g), jpeg.parse(g, progressive=True)
    assert b.scans is None and not b.progressive and b.unsupported is None
    assert (a.scan_begin, a.scan_end, a.restart_interval, a.scan_components) == (
        b.scan_begin, b.scan_end, b.restart_interval, b.scan_components)
    assert np.array_equal(a.intervals, b.intervals) and np.array_equal(a.rst, b.rst)


# ---- the rejection rules: a Pillow file (ten scans: DC Al 1; Y 1-5 Al 2; Cr, Cb 1-63 Al 1; Y 6-63 Al 2; Y 1-63 Ah 2 Al 1;
# DC Ah 1; Cr, Cb, Y 1-63 Ah 1 Al 0) edited in place
def _sos_start(sc):
  return sc['begin'] - (8 + 2 * len(sc['comps']))


def _edited(name='smooth_13x17_444'):
  f = fixtures()[name][0]
  return bytearray(f), ref.read_scans(f)['scans']


def _reason(data):
  info = jpeg.parse(bytes(data), progressive=True)
  assert not info.progressive
  return info.unsupported


def test_pillow_script_is_the_one_the_edits_assume():
  _, scans = _edited()
  assert [(sc['comps'], sc['ss'], sc['se'], sc['ah'], sc['al']) for sc in scans] == [
      ([0, 1, 2], 0, 0, 0, 1), ([0], 1, 5, 0, 2), ([2], 1, 63, 0, 1), ([1], 1, 63, 0, 1), ([0], 6, 63, 0, 2),
      ([0], 1, 63, 2, 1), ([0, 1, 2], 0, 0, 1, 0), ([2], 1, 63, 1, 0), ([1], 1, 63, 1, 0), ([0], 1, 63, 1, 0)]


def test_rejects_a_dc_scan_with_ac_coefficients():
  a, scans = _edited()
  a[scans[0]['begin'] - 2] = 5      # Se
  assert 'mixes DC and AC' in _reason(a)


def test_rejects_two_components_in_an_ac_scan():
  a, scans = _edited()
  sc = scans[1]
  sos = bytes([0xFF, 0xDA, 0, 10, 2, 1, 0x00, 2, 0x11, 1, 5, 0x02])
  assert 'AC scan 1 names 2 components' in _reason(a[:_sos_start(sc)] + sos + a[sc['begin']:])


def test_rejects_al_other_than_ah_minus_one():
  a, scans = _edited()
  a[scans[5]['begin'] - 1] = 0x20
  assert 'bad successive approximation Ah 2, Al 0' in _reason(a)
  a[scans[5]['begin'] - 1] = 0xFE      # Al 14
  assert 'bad successive approximation' in _reason(a)


def test_rejects_a_refinement_before_its_first_scan():
  a, scans = _edited()
  a[scans[1]['begin'] - 1] = 0x32
  assert 'scan 1: refinement out of sequence' in _reason(a)
  # and a first scan over coefficients already seen
  a, scans = _edited()
  a[scans[5]['begin'] - 1] = 0x01
  assert 'scan 5: refinement out of sequence' in _reason(a)


def test_rejects_an_ac_scan_before_the_dc_scan():
  a, scans = _edited()
  assert 'AC scan 0 before the DC scan' in _reason(a[:_sos_start(scans[0])] + a[scans[0]['end']:])


def test_rejects_incomplete_scans():
  a, scans = _edited()
  assert _reason(a[:_sos_start(scans[-1])] + a[scans[-1]['end']:]) == 'progressive file with incomplete scans'
  # the DC refinement alone missing
  assert _reason(a[:_sos_start(scans[6])] + a[scans[6]['end']:]) == 'progressive file with incomplete scans'


def test_rejects_quantisation_tables_between_scans():
  a, scans = _edited()
  dqt = bytes([0xFF, 0xDB, 0, 67, 0]) + bytes([1] * 64)
  at = scans[0]['end']
  assert 'quantisation tables redefined between scans' in _reason(a[:at] + dqt + a[at:])


def test_rejects_more_than_256_scans():
  a, scans = _edited()
  last = bytes(a[_sos_start(scans[-1]):scans[-1]['end']])
  assert _reason(a[:scans[-1]['end']] + last * 247 + b'\xff\xd9') == 'more than 256 scans'
  assert 'refinement out of sequence' in _reason(a[:scans[-1]['end']] + last * 246 + b'\xff\xd9')      # 256: not the cap


def test_missing_tables_truncation_and_a_missing_eoi_raise():
  a, scans = _edited()
  f = bytes(a)
  first_dht = f.index(b'\xff\xc4')
  seglen = (f[first_dht + 2] << 8) | f[first_dht + 3]
  with pytest.raises(ValueError, match='Huffman table of progressive scan 0 is not defined'):
    jpeg.parse(f[:first_dht] + f[first_dht + 2 + seglen:], progressive=True)
  with pytest.raises(ValueError, match='EOI'):
    jpeg.parse(f[:(scans[4]['begin'] + scans[4]['end']) // 2], progressive=True)
  with pytest.raises(ValueError, match='EOI'):
    jpeg.parse(f[:-2], progressive=True)


def test_unsupported_progressive_shapes_keep_taking_the_fallback():
  a, scans = _edited()
  calls = []

  def fallback(data):
    calls.append(data)
    return np.zeros((17, 13, 3), np.uint8)

  damaged = bytes(a[:_sos_start(scans[-1])] + a[scans[-1]['end']:])
  good = fixtures()['grey_13x17'][0]
  with pytest.raises(NotImplementedError, match='entry 1: progressive file with incomplete scans'):
    jpeg.pack([good, damaged], progressive=True)
  pk = jpeg.pack([good, damaged], fallback, progressive=True)
  assert calls == [damaged] and pk.prog_index == [0] and sorted(pk.fallback) == [1]


def test_pack_with_the_flag_keeps_the_sequential_fields_and_orders_the_slots():
  fx, base = fixtures(), baseline()
  seq = [base['smooth_17x33_420'][0], base['rst2_422_33x47'][0]]
  prog = [fx['noise_13x17_422'][0], fx['rst1_grey_40x48'][0]]
  decoded = base['opt_444_24x20'][1]
  entries = [prog[0], seq[0], decoded, prog[1], seq[1]]
  pk = jpeg.pack(entries, progressive=True)
  assert pk.dev_index == [1, 4] and pk.prog_index == [0, 3] and sorted(pk.fallback) == [2]
  assert pk.sizes == [(17, 13), (33, 17), (20, 24), (48, 40), (47, 33)]
  # slots: the sequential rows, the progressive rows, the hosted entries; 16-byte aligned, back to back
  order = [1, 4, 0, 3, 2]
  at = 0
  for k in order:
    assert pk.offsets[k] == at
    at += (pk.sizes[k][0] * pk.sizes[k][1] * 3 + 15) // 16 * 16
  assert pk.total_bytes == at and pk.host_begin == pk.offsets[2]
  alone = jpeg.pack(seq)
  for name in ('files', 'descs', 'tables', 'intervals'):
    assert np.array_equal(getattr(pk, name), getattr(alone, name)), name
  assert (pk.total_blocks, pk.max_blocks, pk.max_pixels) == (alone.total_blocks, alone.max_blocks, alone.max_pixels)
  # the progressive tables
  infos = [jpeg.parse(f, progressive=True) for f in prog]
  assert pk.prog_descs['dst_offset'].tolist() == [pk.offsets[0], pk.offsets[3]]
  assert pk.prog_descs['first_interval'].tolist() == [0, len(infos[0].scans)]
  assert pk.prog_descs['n_intervals'].tolist() == [len(i.scans) for i in infos]
  assert not pk.prog_descs['restart_interval'].any() and not pk.prog_descs['dcsel'].any() and not pk.prog_descs['acsel'].any()
  assert len(pk.prog_scans) == sum(len(i.scans) for i in infos)
  assert pk.prog_total_blocks == sum(i.n_blocks for i in infos)
  assert len(pk.prog_intervals) == sum(len(sc.intervals) for i in infos for sc in i.scans)
  for row, info in enumerate(infos):
    d = pk.prog_descs[row]
    rows = pk.prog_scans[int(d['first_interval']):int(d['first_interval'] + d['n_intervals'])]
    for r, sc in zip(rows, info.scans):
      assert r['image'] == row and r['ncomp'] == len(sc.components)
      assert (r['ss'], r['se'], r['ah'], r['al'], r['restart_interval']) == (sc.ss, sc.se, sc.ah, sc.al, sc.restart_interval)
      body = pk.prog_files[int(r['byte_begin']):int(r['byte_end'])]
      assert body.tobytes() == prog[row][sc.begin:sc.end]
      assert d['scan_offset'] <= r['byte_begin'] and r['byte_end'] <= d['scan_offset'] + d['scan_bytes']
      n_tab = 1 if sc.ss else len(sc.components) if sc.ah == 0 else 0
      assert all(0 <= h < len(pk.prog_huff) for h in r['huff'][:n_tab]) and all(h == -1 for h in r['huff'][n_tab:])
      iv = pk.prog_intervals[int(r['first_interval']):int(r['first_interval'] + r['n_intervals'])]
      assert (iv['image'] == row).all() and iv['n_mcus'].sum() == sc.n_mcus(info) and iv['rst'][-1] == -1


def test_scan_struct_matches_the_header():
  assert ctypes.sizeof(lib.JpegScan) == 56 == jpeg.SCAN_DTYPE.itemsize
  hdr = open(os.path.join(ROOT, 'include', 'asm_hip.h')).read()
  assert re.search(r'\} asm_jpeg_scan;\s*/\* 56 bytes \*/', hdr)
  src = open(os.path.join(ROOT, 'assembled_cnn_amd', 'csrc', 'jpeg.hip')).read()
  assert 'sizeof(asm_jpeg_scan) == 56' in src[:src.index('namespace')]
  # field order, types and offsets, read off the typedef
  body = hdr[hdr.index('typedef struct asm_jpeg_scan {'):hdr.index('} asm_jpeg_scan;')]
  names = []
  for ctype, decl in re.findall(r'^  (int32_t|int64_t|uint8_t) ([^;]+);', body, re.M):
    names += [n.split('[')[0].strip() for n in decl.split(',')]
  assert names == [n for n, _ in lib.JpegScan._fields_]
  offsets = {n: getattr(lib.JpegScan, n).offset for n in names}
  assert (offsets['comp'], offsets['ss'], offsets['huff'], offsets['restart_interval'], offsets['byte_begin'],
          offsets['byte_end']) == (8, 12, 16, 28, 40, 48)
  assert lib.ABI_VERSION == 11 and 'asm_jpeg_decode_progressive' in lib.SIGNATURES
