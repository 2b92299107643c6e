"""Host side of the segment-parallel JPEG entropy stage, without a GPU: the segment table jpeg.pack fills, the binding
of asm_jpeg_decode_parallel against the header, and the argument checks of the real library (they come before any
launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _files():
  out = []
  for npz in ('jpeg_fixtures.npz', 'jpeg_parallel_fixtures.npz'):
    fx = np.load(os.path.join(ROOT, 'tests', 'golden', npz))
    out += [fx['file_' + str(n)].tobytes() for n in fx['names'] if str(fx['kind_' + str(n)]) == 'device']
  return out


@pytest.mark.parametrize('segment_bytes', [16, 48, 128, 65536])
def test_segment_table_is_consistent_with_the_interval_rows(segment_bytes):
  from assembled_cnn_amd import jpeg
  files = _files()
  pk = jpeg.pack(files, segment_bytes=segment_bytes)
  plain = jpeg.pack(files)
  # nothing else changes
  for name in ('files', 'descs', 'tables', 'intervals', 'offsets'):
    assert np.array_equal(getattr(pk, name), getattr(plain, name)), name
  assert plain.segment_bytes is None and plain.total_segments == 0 and plain.segment_first.size == 0
  assert pk.segment_bytes == segment_bytes and pk.segment_first.dtype == np.int32
  assert pk.segment_first.shape == (len(pk.intervals),)
  size = pk.intervals['byte_end'] - pk.intervals['byte_begin']
  counts = np.array([max(1, -(-int(s) // segment_bytes)) for s in size])
  assert pk.segment_first[0] == 0 and np.array_equal(pk.segment_first[1:], np.cumsum(counts)[:-1])
  assert pk.total_segments == counts.sum()
  # the last segment of an interval takes the remainder; an interval no longer than one segment is one segment
  assert np.all((counts - 1) * segment_bytes < np.maximum(size, 1)) and np.all(counts * segment_bytes >= size)
  if segment_bytes == 16:
    assert counts.max() > 256          # more segments than the workgroup has lanes
    assert (counts == 1).any()         # a scan shorter than a segment


def test_default_pack_and_decode_arguments():
  from assembled_cnn_amd import jpeg
  f = _files()[0]
  for bad in (0, 8, 24, 131072, 16.5):
    with pytest.raises(ValueError, match='segment_bytes'):
      jpeg.pack([f], segment_bytes=bad)
  pk = jpeg.pack([f])
  with pytest.raises(ValueError, match='packed with segment_bytes'):
    jpeg.decode_packed(pk, 'cpu', entropy='parallel')
  with pytest.raises(ValueError, match='entropy must be'):
    jpeg.decode_packed(pk, 'cpu', entropy='fast')
  with pytest.raises(ValueError, match='entropy must be'):
    jpeg.decode_batch([f], 'cpu', entropy='fast')
  with pytest.raises(ValueError, match="needs entropy='parallel'"):
    jpeg.decode_batch([f], 'cpu', segment_bytes=64)
  assert jpeg.DEFAULT_SEGMENT_BYTES % 16 == 0 and 16 <= jpeg.DEFAULT_SEGMENT_BYTES <= 65536


def test_binding_matches_the_header():
  from assembled_cnn_amd import lib
  hdr = open(os.path.join(ROOT, 'include', 'asm_hip.h')).read()
  assert '#define ASM_ABI_VERSION 11' in hdr and lib.ABI_VERSION == 11
  decl = re.search(r'^int asm_jpeg_decode_parallel\((.*?)\);', hdr, re.S | re.M).group(1)
  params = [' '.join(p.split()) for p in decl.split(',')]
  kinds = {'int': C.c_int, 'int64_t': C.c_int64}
  want = [C.c_void_p if '*' in p else kinds[p.rsplit(' ', 1)[0]] for p in params]
  restype, argtypes = lib.SIGNATURES['asm_jpeg_decode_parallel']
  assert restype is C.c_int and argtypes == want
  assert [p.rsplit(' ', 1)[1].lstrip('*') for p in params][5:10] == ['segment_first', 'N', 'n_intervals', 'total_segments',
                                                                    'segment_bytes']
  # the state row the workspace query counts is the header's "32 bytes"
  src = open(os.path.join(ROOT, 'assembled_cnn_amd', 'csrc', 'jpeg.hip')).read()
  assert 'sizeof(jpeg_seg) == 32' in src


def test_argument_checks_go_through_the_real_library():
  import __graft_entry__
  __graft_entry__.build()
  from assembled_cnn_amd import lib
  L = lib.load()
  need = C.c_int64(-1)
  assert L.asm_jpeg_decode_parallel_workspace_bytes(10, 7, C.byref(need)) == lib.ASM_OK and need.value == 10 * 192 + 7 * 32
  assert L.asm_jpeg_decode_parallel_workspace_bytes(10, -1, C.byref(need)) == lib.ASM_EINVAL
  assert L.asm_jpeg_decode_parallel_workspace_bytes(10, 2 ** 30, C.byref(need)) == lib.ASM_EINVAL
  buf = (C.c_uint8 * 4096)()
  p = C.addressof(buf) // 16 * 16 + 16       # non-null, 16-byte aligned; never dereferenced: every call below is refused

  def call(N=1, segment_bytes=16, total_segments=4, total_blocks=4, ws_bytes=4 * 192 + 4 * 32, stages=3, files_bytes=64):
    return L.asm_jpeg_decode_parallel(p, files_bytes, p, p, p, p, N, 1, total_segments, segment_bytes, total_blocks, 4, 64, p,
                                      1024, p, None, p, ws_bytes, stages, None)

  for bad in (0, 8, 24, 131072, -16, 65552):
    assert call(segment_bytes=bad) == lib.ASM_EINVAL
    assert b'segment_bytes' in L.asm_last_error()
  assert call(ws_bytes=4 * 192 + 4 * 32 - 1) == lib.ASM_EINVAL and b'workspace too small' in L.asm_last_error()
  assert call(total_segments=-1) == lib.ASM_EINVAL
  assert call(total_segments=2 ** 30) == lib.ASM_EINVAL
  assert call(files_bytes=2 ** 40) == lib.ASM_EINVAL
  assert call(stages=0) == lib.ASM_EINVAL and call(stages=4) == lib.ASM_EINVAL
  assert call(N=65536) == lib.ASM_EINVAL
  # N == 0 is a no-op: no pointer is looked at, nothing is launched
  assert L.asm_jpeg_decode_parallel(None, 0, None, None, None, None, 0, 0, 0, 16, 0, 0, 0, None, 0, None, None, None, 0, 3,
                                    None) == lib.ASM_OK
  # a null table is refused before any launch
  assert L.asm_jpeg_decode_parallel(p, 64, p, p, p, None, 1, 1, 4, 16, 4, 4, 64, p, 1024, p, None, p, 4 * 192 + 4 * 32, 3,
                                    None) == lib.ASM_EINVAL
  assert b'null pointer' in L.asm_last_error()
