"""The host side of the device header parse (jpeg.pack_device): the layout function between the two launches against
jpeg.pack on a mixed batch, the unchanged records.Batch, and the argument errors.  No GPU."""
import os

import numpy as np
import pytest

from assembled_cnn_amd import input_pipeline as ip
from assembled_cnn_amd import jpeg, records
from tests import jpeg_parse_cases as cases

NAMES = ('noise_13x17_420', 'rst1_444_noise_72x72', 'cmyk_16x16', 'grey_13x17', 'progressive_16x16', 'noise_8x8_422',
         'rst1_grey_168x160', 'tex_56x40_444')


def _heads(files, infos, segment_bytes):
  """the head rows asm_jpeg_parse writes for these files, made from jpeg.parse's results"""
  heads = np.zeros(len(files), jpeg.HEAD_DTYPE)
  for k, info in enumerate(infos):
    h = heads[k]
    if info is None or info.unsupported is not None or info.progressive:
      h['cls'] = 4 if info is not None else 1
      continue
    h['width'], h['height'], h['ncomp'], h['hs'], h['vs'] = info.width, info.height, info.ncomp, info.hs, info.vs
    h['restart_interval'], h['n_intervals'] = info.restart_interval, len(info.intervals)
    h['scan_begin'], h['scan_bytes'] = info.scan_begin, info.scan_end - info.scan_begin
    if segment_bytes is not None:
      size = info.intervals[:, 1] - info.intervals[:, 0]
      h['n_segments'] = np.maximum(-(-size // segment_bytes), 1).sum()
  return heads


@pytest.mark.parametrize('segment_bytes', [None, 16, 128])
def test_layout_of_head_rows_equals_pack(segment_bytes):
  fx = cases.load()
  decoded = np.arange(7 * 5 * 3, dtype=np.uint8).reshape(7, 5, 3)
  files = [fx[n][0] for n in NAMES[:5]] + [decoded] + [fx[n][0] for n in NAMES[5:]]
  fallback = lambda data: np.full((16, 16, 3), 9, np.uint8)       # noqa: E731
  infos = [jpeg.parse(f, True) if jpeg.is_encoded(f) else None for f in files]
  pk = jpeg.pack(files, fallback, infos=infos, progressive=True, segment_bytes=segment_bytes)
  assert pk.prog_index == [4] and sorted(pk.fallback) == [2, 5] and len(pk.dev_index) == 6
  sizes = [(0, 0) if k in pk.dev_index else pk.sizes[k] for k in range(len(files))]
  place, rows, offsets, total, totals = jpeg.layout_heads(_heads(files, infos, segment_bytes), sizes,
                                                          pk.prog_index + sorted(pk.fallback), segment_bytes)
  assert rows == pk.dev_index and place['span'].tolist() == pk.dev_index
  assert np.array_equal(offsets, pk.offsets) and max(total, 16) == pk.total_bytes
  assert int(offsets[sorted(pk.fallback)[0]]) == pk.host_begin
  assert (totals['total_blocks'], totals['max_blocks'], totals['max_pixels']) == (pk.total_blocks, pk.max_blocks,
                                                                                  pk.max_pixels)
  assert totals['n_intervals'] == len(pk.intervals)
  assert np.array_equal(place['first_interval'], pk.descs['first_interval'])
  assert np.array_equal(place['coef_offset'], pk.descs['coef_offset'])
  assert np.array_equal(place['dst_offset'], pk.descs['dst_offset'])
  if segment_bytes is None:
    assert totals['total_segments'] == 0 and not place['first_segment'].any()
  else:
    assert totals['total_segments'] == pk.total_segments
    assert np.array_equal(place['first_segment'], pk.segment_first[pk.descs['first_interval']])


def test_layout_refuses_what_segment_table_refuses():
  heads = np.zeros(2, jpeg.HEAD_DTYPE)
  heads['width'] = heads['height'] = 8
  heads['ncomp'] = heads['hs'] = heads['vs'] = heads['n_intervals'] = 1
  heads['n_segments'] = 2 ** 29
  with pytest.raises(ValueError, match='segment_bytes = 16 gives %d segments, more than one call takes' % 2 ** 30):
    jpeg.layout_heads(heads, None, (), 16)
  iv = np.zeros(1, jpeg.INTERVAL_DTYPE)
  iv['byte_end'] = 16 * 2 ** 30
  with pytest.raises(ValueError, match='segment_bytes = 16 gives %d segments, more than one call takes' % 2 ** 30):
    jpeg.segment_table(iv, 16)
  with pytest.raises(ValueError, match='every entry once'):
    jpeg.layout_heads(heads, None, (1,), None)


def test_batch_without_payloads_is_unchanged(tmp_path):
  assert records.Batch._fields == ('encoded', 'labels', 'filenames', 'origins', 'payloads')
  assert records.Batch._field_defaults == {'payloads': None}
  fx = cases.load()
  path = str(tmp_path / 'validation-00000-of-00001')
  records.write_records(path, [records.encode_example({'image/encoded': [fx[n][0]], 'image/filename': [n.encode()],
                                                       'image/class/label': np.array([i])})
                               for i, n in enumerate(NAMES)])
  batches = list(records.RecordDataset([path], False, 5, 1, verify='host', device='cpu'))
  assert [len(b.encoded) for b in batches] == [5, 3] and all(b.payloads is None for b in batches)
  assert [e.tobytes() for b in batches for e in b.encoded] == [fx[n][0] for n in NAMES]
  assert len(batches[0]) == 5 and batches[0][:4] == (batches[0].encoded, batches[0].labels, batches[0].filenames,
                                                     batches[0].origins)


def test_argument_errors():
  fx = cases.load()
  files = [fx[NAMES[0]][0]]
  with pytest.raises(ValueError, match="parse must be one of"):
    jpeg.decode_batch(files, 'cpu', parse='gpu')
  with pytest.raises(ValueError, match="resident needs parse='device'"):
    jpeg.decode_batch(files, 'cpu', resident=(None, None))
  with pytest.raises(ValueError, match="jpeg_parse must be one of"):
    ip.preprocess_batch(files, False, 'cpu', jpeg_parse='both')
  with pytest.raises(ValueError, match="resident needs parse='device'"):
    ip.preprocess_batch(files, False, 'cpu', jpeg_resident=(None, None))
  with pytest.raises(ValueError, match='segment_bytes must be a multiple of 16'):
    jpeg.pack_device(files, 'cpu', segment_bytes=24)
  assert os.path.exists(os.path.join(cases.GOLDEN, 'make_jpeg_parse_fixtures.py'))
