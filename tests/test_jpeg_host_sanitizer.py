"""The device JPEG entropy decoder's own text (csrc/jpeg_entropy.h), compiled for the host with the address and
undefined-behaviour sanitizers and run as a stand-alone program (tools/probes/jpeg_entropy_host.cpp): every fixture intact
(coefficients equal tests/jpeg_ref.py's), then every truncation of each scan and every single byte replaced by 00, FF and
D9, then damaged interval rows.  The program's `status digest` line pins the status word of every damaged run to the
value recorded in tests/golden/jpeg_status_digests.json.  No GPU; nothing is loaded into this interpreter, nothing is
preloaded, the environment is passed on as it is."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import jpeg_ref
from tests.sanitizer_build import compile_command

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tools', 'probes', 'jpeg_entropy_host.cpp')


def recorded_digest(program):
  with open(os.path.join(ROOT, 'tests', 'golden', 'jpeg_status_digests.json')) as f:
    return json.load(f)[program]


def _cases():
  from assembled_cnn_amd import jpeg
  fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_fixtures.npz'))
  blobs = []
  for name in fx['names']:
    if str(fx['kind_' + name]) != 'device':
      continue
    data = fx['file_' + name].tobytes()
    pk = jpeg.pack([data])
    coefs, _ = jpeg_ref.coefficients(data)
    expected = np.concatenate([c.reshape(-1) for c in coefs]).astype('<i2')
    scan = pk.files[:int(pk.descs[0]['scan_bytes'])]
    blobs.append(pk.descs.tobytes() + pk.tables.tobytes() + struct.pack('<i', len(pk.intervals)) + pk.intervals.tobytes() +
                 struct.pack('<q', scan.size) + scan.tobytes() + struct.pack('<q', expected.size) + expected.tobytes())
  return struct.pack('<i', len(blobs)) + b''.join(blobs), len(blobs)


def test_entropy_decoder_is_clean_under_host_sanitizers(tmp_path):
  exe = str(tmp_path / 'jpeg_entropy_host')
  r = subprocess.run(compile_command(SRC, exe), capture_output=True, text=True)
  assert r.returncode == 0, 'compile failed:\n%s\n%s' % (r.stdout, r.stderr)
  blob, n = _cases()
  path = str(tmp_path / 'cases.bin')
  with open(path, 'wb') as f:
    f.write(blob)
  r = subprocess.run([exe, path], capture_output=True, text=True)
  assert r.returncode == 0, 'sanitizer program failed (%d):\n%s\n%s' % (r.returncode, r.stdout, r.stderr[-4000:])
  assert 'ERROR' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
  assert ('%d cases intact and equal' % n) in r.stdout and n >= 39, r.stdout
  assert ('status digest: %s\n' % recorded_digest('jpeg_entropy_host')) in r.stdout, r.stdout
