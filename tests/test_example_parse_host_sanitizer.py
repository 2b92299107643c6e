"""The device Example parser's text (csrc/example_parse.h: the walk through its window, the schema checks, the row, the KD
label row), compiled for the host with the address and undefined-behaviour sanitizers and run as a stand-alone program
(tools/probes/example_parse_host.cpp).  No GPU; nothing is loaded into this interpreter, nothing is preloaded, the
environment is passed on as it is.

The whole case set of tests/example_cases.py goes through the program, every payload in a heap block that ends with its last
byte and at all 16 start alignments; the rows it writes must keep the contract against records._proto, and the label rows
must equal records._kd_label word for word (NaN patterns, a label of -1 and of num_classes among them)."""
import os
import struct
import subprocess

import numpy as np

from assembled_cnn_amd import lib
from tests import example_cases as cases
from tests.sanitizer_build import compile_command

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tools', 'probes', 'example_parse_host.cpp')
CANARY = 0xA5A5A5A5


def test_example_parser_is_clean_and_keeps_the_contract(tmp_path):
  every = cases.all_cases()
  want = cases.host_results()
  C = cases.NUM_CLASSES
  path, out = str(tmp_path / 'cases.bin'), str(tmp_path / 'rows.bin')
  with open(path, 'wb') as f:
    f.write(struct.pack('<ii', len(every), C))
    for _, payload, _ in every:
      f.write(struct.pack('<q', len(payload)) + payload)
  exe = str(tmp_path / 'example_parse_host')
  r = subprocess.run(compile_command(SRC, exe), capture_output=True, text=True)
  assert r.returncode == 0, 'compile failed:\n%s\n%s' % (r.stdout, r.stderr)
  r = subprocess.run([exe, path, out], capture_output=True, text=True)
  assert r.returncode == 0, 'sanitizer program failed (%d):\n%s\n%s' % (r.returncode, r.stdout, r.stderr[-4000:])
  assert 'ERROR' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
  rec = np.dtype([('row', cases.ROW_DTYPE), ('status', '<i4'), ('words', '<u4', (2 * C,))])
  got = np.fromfile(out, dtype=rec)
  assert got.size == len(every)
  assert 'example_parse_host: %d cases at 16 alignments, %d class 0, 0 mismatches' % (
      len(every), int((got['row']['cls'] == 0).sum())) in r.stdout, r.stdout
  written, seen_labels, nan_rows = 0, set(), 0
  for (label, payload, expect), w, g in zip(every, want, got):
    cases.check_row(label, payload, expect, w, g['row'])
    kd = cases.kd_row(w) if w is not None and g['row']['cls'] == 0 else None
    if kd is None:
      assert g['status'] == lib.EXAMPLE_LSKIP and (g['words'] == CANARY).all(), label
    else:
      assert g['status'] == 0 and g['words'].tolist() == kd.tolist(), label
      written += 1
      seen_labels.add(w[1])
      nan_rows += int(np.isnan(kd[C:].view(np.float32)).any() and 0x7fc12345 in kd[C:].tolist())
  assert written > 1000 and {-1, 0, C - 1, C} <= seen_labels and nan_rows >= 1
  # what the counts above rest on: the must list and the content mutations are there
  kinds = [e for _, _, e in every]
  assert kinds.count(cases.MUST) > 500 and kinds.count(cases.CONTENT) > 400
  assert sum(w is not None for w, e in zip(want, kinds) if e == cases.ANY) > 1000
