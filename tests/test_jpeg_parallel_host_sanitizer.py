"""The segment-parallel JPEG entropy decoder's own text (csrc/jpeg_parallel.h), compiled for the host with the address and
undefined-behaviour sanitizers and run as a stand-alone program (tools/probes/jpeg_parallel_host.cpp) with the lanes of
the workgroup simulated by a loop, at segment_bytes 16, 48 and 128 and at 5 and 256 lanes.  Every device fixture of
jpeg_fixtures.npz and jpeg_parallel_fixtures.npz intact (coefficients equal tests/jpeg_ref.py's), then every truncation
of each scan and every single byte replaced by 00, FF and D9 (the status word equals the sequential decoder's) -- for the
one scan longer than 8 KB at every seventh position and at its middle -- and two images on shared state rows.  No GPU;
nothing is loaded into this interpreter, nothing is preloaded, the environment is passed on as it is."""
import os
import re
import struct
import subprocess

import numpy as np

from tests import jpeg_ref
from tests.sanitizer_build import compile_command

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tools', 'probes', 'jpeg_parallel_host.cpp')


def _cases():
  from assembled_cnn_amd import jpeg
  blobs = []
  for npz in ('jpeg_fixtures.npz', 'jpeg_parallel_fixtures.npz'):
    fx = np.load(os.path.join(ROOT, 'tests', 'golden', npz))
    for name in fx['names']:
      if str(fx['kind_' + name]) != 'device':
        continue
      data = fx['file_' + name].tobytes()
      pk = jpeg.pack([data])
      coefs, _ = jpeg_ref.coefficients(data)
      expected = np.concatenate([c.reshape(-1) for c in coefs]).astype('<i2')
      scan = pk.files[:int(pk.descs[0]['scan_bytes'])]
      blobs.append(pk.descs.tobytes() + pk.tables.tobytes() + struct.pack('<i', len(pk.intervals)) +
                   pk.intervals.tobytes() + struct.pack('<q', scan.size) + scan.tobytes() +
                   struct.pack('<q', expected.size) + expected.tobytes())
  return struct.pack('<i', len(blobs)) + b''.join(blobs), len(blobs)


def test_parallel_entropy_decoder_is_clean_and_equal_under_host_sanitizers(tmp_path):
  exe = str(tmp_path / 'jpeg_parallel_host')
  r = subprocess.run(compile_command(SRC, exe), capture_output=True, text=True)
  assert r.returncode == 0, 'compile failed:\n%s\n%s' % (r.stdout, r.stderr)
  blob, n = _cases()
  path = str(tmp_path / 'cases.bin')
  with open(path, 'wb') as f:
    f.write(blob)
  r = subprocess.run([exe, path], capture_output=True, text=True)
  assert r.returncode == 0, 'sanitizer program failed (%d):\n%s\n%s' % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
  assert 'ERROR' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
  assert ('%d cases intact and equal' % n) in r.stdout and n >= 46, r.stdout[-2000:]
  assert ', 0 mismatches' in r.stdout, r.stdout[-2000:]
  rows = [tuple(int(v) for v in m) for m in re.findall(
      r'^case (\d+) segment_bytes (\d+) lanes (\d+) segments (\d+) rounds (\d+)$', r.stdout, re.M)]
  assert len(rows) == n * 6, 'one line per case, segment size and lane count'
  print('\n'.join('case %d segment_bytes %d lanes %d: %d segments, %d rounds' % row for row in rows))
  assert all(1 <= rounds <= segments + 1 for _, _, _, segments, rounds in rows)
  assert any(rounds > 1 for _, _, _, _, rounds in rows)
  # one simulated lane count is smaller than the segment count of the largest case: several passes of 256 lanes
  assert max(segments for _, _, _, segments, _ in rows) > 2 * 256
  assert re.search(r'^shared state rows: cases \d+ \(1 intervals\) and \d+ \(81 intervals\), 12 runs$', r.stdout, re.M), r.stdout[-2000:]
