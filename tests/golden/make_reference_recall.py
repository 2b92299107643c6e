#!/usr/bin/env python
"""Generate tests/golden/reference_recall.json by RUNNING the reference's own get_recall (metric/recall_metric.py:217-228).

  python tests/golden/make_reference_recall.py --reference <checkout of clovaai/assembled-cnn> [--check]

The module is imported unmodified with `tensorflow` replaced by an inert stand-in (as make_reference_golden.py does);
scikit-learn is imported by it and never called.  get_recall is plain Python over the top-k index rows, so the cases below
are small hand-made rows: what the file pins is the self-removal rule and the label lookup, not a similarity.
--check re-derives every case and compares it with the committed file instead of writing it.
"""
import argparse
import json
import os
import sys
from unittest import mock

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'reference_recall.json')

CASES = [
    # four classes of two, distractors at the END: query position == index position, the self entry is dropped
    dict(name='distractors_at_end', labels=[0, 0, 1, 1, 2, 2, -1, -1], k_list=[1, 5],
         sorted_idx=[[0, 1, 6, 2, 3, 4], [1, 6, 0, 2, 3, 4], [2, 7, 3, 0, 1, 4], [3, 0, 1, 4, 5, 2], [4, 6, 7, 0, 1, 5],
                     [5, 0, 1, 2, 3, 6]]),
    # distractors INTERLEAVED: queries are index rows 1, 2, 4, 5 but are numbered 0..3, so row 0 drops index 0 (a
    # distractor), not its own entry 1 -- the self-match stays and counts as a hit (the quirk)
    dict(name='distractors_interleaved', labels=[-1, 0, 1, -1, 0, 1], k_list=[1, 5],
         sorted_idx=[[1, 0, 4, 2, 3, 5], [2, 1, 5, 0, 3, 4], [4, 2, 0, 3, 5, 1], [5, 3, 0, 1, 2, 4]]),
    # the self index is absent from a row: nothing is dropped, the first k of all K entries count
    dict(name='self_absent', labels=[0, 1, 0, 1, 2, 2], k_list=[1, 5],
         sorted_idx=[[3, 1, 4, 5, 2, 2], [0, 2, 4, 5, 3, 3], [2, 0, 1, 3, 4, 5], [1, 3, 0, 2, 4, 5], [0, 1, 2, 3, 5, 5],
                     [5, 4, 0, 1, 2, 3]]),
    # every row carries the same label twice and more
    dict(name='duplicate_labels', labels=[7, 7, 7, 7, 3, 3], k_list=[1, 5],
         sorted_idx=[[0, 4, 5, 1, 2, 3], [1, 0, 2, 3, 4, 5], [4, 5, 2, 0, 1, 3], [3, 4, 5, 2, 1, 0], [4, 0, 1, 2, 3, 5],
                     [0, 1, 2, 3, 5, 4]]),
    dict(name='k_1_2_4_8', labels=[0, 1, 2, 3, 0, 1, 2, 3, 4, 4, -1, -1], k_list=[1, 2, 4, 8],
         sorted_idx=[[0, 1, 4, 2, 3, 5, 6, 7, 8], [1, 10, 11, 0, 5, 2, 3, 4, 6], [2, 0, 1, 3, 4, 5, 7, 8, 6],
                     [3, 0, 1, 2, 4, 5, 6, 8, 9], [4, 1, 2, 3, 5, 6, 7, 8, 9], [0, 2, 3, 4, 6, 7, 8, 9, 1],
                     [6, 10, 2, 0, 1, 3, 4, 5, 7], [7, 0, 1, 2, 4, 5, 6, 8, 9], [9, 8, 0, 1, 2, 3, 4, 5, 6],
                     [9, 0, 1, 2, 3, 4, 5, 6, 7]]),
]


def _import_reference(ref):
  import importlib.abc
  import importlib.machinery
  sys.path.insert(0, ref)
  fake = mock.MagicMock(name='tensorflow')
  fake.VERSION = fake.__version__ = '1.14.0'
  fake.__path__ = []

  class _Loader(importlib.abc.Loader):
    def create_module(self, spec):
      return fake

    def exec_module(self, module):
      pass

  class _Finder(importlib.abc.MetaPathFinder):
    def find_spec(self, name, path=None, target=None):
      if name.split('.')[0] in ('tensorflow', 'absl', 'tensorflow_hub'):
        return importlib.machinery.ModuleSpec(name, _Loader(), is_package=True)
      return None
  sys.meta_path.insert(0, _Finder())
  from metric import recall_metric
  return recall_metric


def derive(ref):
  import numpy as np
  rm = _import_reference(ref)
  out = []
  for c in CASES:
    labels = np.asarray(c['labels'], dtype=np.int64)
    qlab = labels[labels != -1]                                   # recall_metric.py:151-154
    idx = np.asarray(c['sorted_idx'], dtype=np.int32)
    assert len(idx) == len(qlab) and idx.shape[1] == max(c['k_list']) + 1, c['name']
    rec = rm.get_recall(idx, qlab, labels, list(c['k_list']))
    out.append(dict(c, query_labels=[int(v) for v in qlab], recall={str(k): float(v) for k, v in rec.items()}))
  return {'source': 'metric/recall_metric.py:217-228 get_recall', 'cases': out}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reference', default=os.environ.get('ASSEMBLED_CNN_REFERENCE'), help='checkout of the reference repository')
  ap.add_argument('--check', action='store_true')
  a = ap.parse_args()
  if not a.reference or not os.path.isdir(a.reference):
    sys.exit('give the reference checkout with --reference (or ASSEMBLED_CNN_REFERENCE)')
  out = derive(a.reference)
  if a.check:
    have = json.load(open(OUT))
    if have != json.loads(json.dumps(out)):
      sys.exit('reference_recall.json differs from what the reference computes')
    print('ok: %d cases match' % len(out['cases']))
    return
  json.dump(out, open(OUT, 'w'), indent=1, sort_keys=True)
  print('wrote', OUT, len(out['cases']), 'cases')


if __name__ == '__main__':
  main()
