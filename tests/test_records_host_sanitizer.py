"""The span checksum's device text (csrc/crc32c_spans.h: the range check, the chunk bounds, the chunk routine, the zero-byte
operators), compiled for the host with the address and undefined-behaviour sanitizers and run as a stand-alone program
(tools/probes/crc32c_spans_host.cpp): the known answers, every length at which the chunking changes shape at four start
alignments and four lane counts, each span at the end of an exact-size heap block, and the out-of-range descriptors.  No
GPU; nothing is loaded into this interpreter, nothing is preloaded, the environment is passed on as it is."""
import os
import subprocess

from tests.sanitizer_build import compile_command

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tools', 'probes', 'crc32c_spans_host.cpp')


def test_span_checksum_is_clean_under_host_sanitizers(tmp_path):
  exe = str(tmp_path / 'crc32c_spans_host')
  r = subprocess.run(compile_command(SRC, exe), capture_output=True, text=True)
  assert r.returncode == 0, 'compile failed:\n%s\n%s' % (r.stdout, r.stderr)
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, 'sanitizer program failed (%d):\n%s\n%s' % (r.returncode, r.stdout, r.stderr[-4000:])
  assert 'ERROR' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
  # 17 lengths x 4 alignments x 4 lane counts
  assert '272 spans equal the byte-at-a-time crc, 4 known answers, 12 descriptors refused, 0 failures' in r.stdout, r.stdout
