"""The progressive entropy stage's own text (csrc/jpeg_entropy.h), compiled for the host with the address and
undefined-behaviour sanitizers and run as a stand-alone program (tools/probes/jpeg_progressive_host.cpp): every progressive
fixture and a re-coded file of every script intact (coefficients equal tests/jpeg_progressive_ref.py's), then every
truncation of every scan and every entropy-coded byte replaced by 00, FF and D9, then damaged table rows.  The program's
`status digest` line pins the status word of every damaged run to the value recorded in
tests/golden/jpeg_status_digests.json.  No GPU; nothing is loaded into this interpreter, nothing is preloaded, the
environment is passed on as it is."""
import os
import struct
import subprocess

import numpy as np

from tests import jpeg_progressive_ref, jpeg_progressive_writer
from tests.sanitizer_build import compile_command
from tests.test_jpeg_host_sanitizer import recorded_digest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tools', 'probes', 'jpeg_progressive_host.cpp')
RECODED = (('noise_13x17_420', 'dc_each_ac_1_63'), ('smooth_17x33_422', 'dc_all_ac_1_2_3_63'),
           ('noise_31x9_444', 'dc_each_ac_1_5_6_20_21_63'))


def _files():
  fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_progressive_fixtures.npz'))
  files = [fx['file_' + str(name)].tobytes() for name in fx['names']]
  base = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_fixtures.npz'))
  return files + [jpeg_progressive_writer.recode(base['file_' + name].tobytes(), script) for name, script in RECODED]


def _rows(table):
  return struct.pack('<i', len(table)) + table.tobytes()


def _cases():
  from assembled_cnn_amd import jpeg
  blobs = []
  for data in _files():
    pk = jpeg.pack([data], progressive=True)
    assert pk.prog_index == [0]
    coefs, _ = jpeg_progressive_ref.coefficients(data)
    expected = np.concatenate([c.reshape(-1) for c in coefs]).astype('<i2')
    body = pk.prog_files[:int(pk.prog_descs[0]['scan_bytes'])]
    blobs.append(pk.prog_descs.tobytes() + _rows(pk.prog_scans) + _rows(pk.prog_huff) + _rows(pk.prog_intervals) +
                 struct.pack('<q', body.size) + body.tobytes() + struct.pack('<q', expected.size) + expected.tobytes())
  return struct.pack('<i', len(blobs)) + b''.join(blobs), len(blobs)


def test_progressive_entropy_decoder_is_clean_under_host_sanitizers(tmp_path):
  exe = str(tmp_path / 'jpeg_progressive_host')
  r = subprocess.run(compile_command(SRC, exe), capture_output=True, text=True)
  assert r.returncode == 0, 'compile failed:\n%s\n%s' % (r.stdout, r.stderr)
  blob, n = _cases()
  path = str(tmp_path / 'cases.bin')
  with open(path, 'wb') as f:
    f.write(blob)
  r = subprocess.run([exe, path], capture_output=True, text=True)
  assert r.returncode == 0, 'sanitizer program failed (%d):\n%s\n%s' % (r.returncode, r.stdout, r.stderr[-4000:])
  assert 'ERROR' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
  assert ('%d cases intact and equal' % n) in r.stdout and n >= 51, r.stdout
  assert ('status digest: %s\n' % recorded_digest('jpeg_progressive_host')) in r.stdout, r.stdout
