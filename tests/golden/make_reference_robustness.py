#!/usr/bin/env python
"""Generate tests/golden/reference_robustness.json by RUNNING the reference's own mce/eval_robustness.py.

  python tests/golden/make_reference_robustness.py --reference <checkout of clovaai/assembled-cnn> [--check]

The module is imported unmodified with `tensorflow` / `absl` replaced by the inert stand-in of make_reference_recall.py and
FLAGS set to a plain namespace.  Its model loop (show_corruption_error_by_distortion) needs TensorFlow and ImageNet-C, so it
is patched with SCRIPTED error rates; tf.gfile.GFile is patched with open, and the Coordinator with one that joins its
threads.  What the file pins is everything around the loop: the AlexNet tables and their order, the quota arithmetic of
process (:249-273), the report lines (:282-284, :301-302), the CE / mCE arithmetic (:278-281, :297-300) and get_synsets2idx
(:151-158).  Only data is written.  --check re-derives everything and compares it with the committed file.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import types
from unittest import mock

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'reference_robustness.json')

WORKERS = list(range(1, 9)) + [19, 20]
LABEL_LINES = ['n01440764\n', ' n01443537 \n', 'Great White Shark\n', 'N01491361\n', 'tiger  shark\n', 'n01496331']


def scripted_rates(names, table):
  """error rate of every corruption, exact decimal fractions: table 0 rises evenly, table 1 is irregular"""
  if table == 0:
    return {n: (50 + 40 * i) / 1000.0 for i, n in enumerate(names)}
  return {n: (((7 * i * i + 3 * i + 11) % 97) * 10 + 13) / 1000.0 for i, n in enumerate(names)}


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
  from mce import eval_robustness
  return eval_robustness, fake


class _Coordinator(object):
  def join(self, threads):
    for t in threads:
      t.join()


def _zero(d):
  for k in d:
    d[k] = 0.0


def derive(ref):
  er, tf = _import_reference(ref)
  names = list(er.ALEXNET_CE.keys())
  out = {'source': 'mce/eval_robustness.py', 'alexnet_ce': [[k, v] for k, v in er.ALEXNET_CE.items()],
         'alexnet_fp': [[k, v] for k, v in er.ALEXNET_FP.items()], 'quota': [], 'tables': []}
  tf.gfile.GFile = open
  tf.gfile.IsDirectory = lambda path: False
  tf.train.Coordinator = _Coordinator

  rates = scripted_rates(names, 0)
  er.show_corruption_error_by_distortion = lambda name, ckpt, gpu: rates[name]
  for n in WORKERS:
    er.FLAGS = types.SimpleNamespace(gpu_index=','.join(str(i) for i in range(n)))
    workers = []
    for w in range(n):
      _zero(er.ABSOLUTE_CE)
      _zero(er.OURS_CE)
      buf = io.StringIO()
      with contextlib.redirect_stdout(buf):
        er.process(w, 'model.ckpt-1')
      workers.append({'handled': [k for k, v in er.ABSOLUTE_CE.items() if v != 0.0], 'lines': buf.getvalue().splitlines()})
    out['quota'].append({'num_workers': n, 'workers': workers})

  for table, gpu_index in ((0, '0'), (1, '0,1,2')):
    rates = scripted_rates(names, table)
    er.show_corruption_error_by_distortion = lambda name, ckpt, gpu, rates=rates: rates[name]
    er.FLAGS = types.SimpleNamespace(gpu_index=gpu_index, model_dir='run/model.ckpt-100')
    _zero(er.ABSOLUTE_CE)
    _zero(er.OURS_CE)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
      er.show_corruption_error()
    out['tables'].append({'gpu_index': gpu_index, 'rates': [[k, rates[k]] for k in names],
                          'ours_ce': [[k, float(v)] for k, v in er.OURS_CE.items()],
                          'absolute_ce': [[k, float(v)] for k, v in er.ABSOLUTE_CE.items()],
                          'mce_lines': [l for l in buf.getvalue().splitlines() if l.startswith('mCE')]})

  with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, 'labels.txt')
    with open(path, 'w') as f:
      f.writelines(LABEL_LINES)
    out['synsets'] = {'lines': LABEL_LINES, 'map': er.get_synsets2idx(path)}
  return out


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
      sys.exit('reference_robustness.json differs from what the reference computes')
    print('ok: %d quota splits, %d rate tables match' % (len(out['quota']), len(out['tables'])))
    return
  json.dump(out, open(OUT, 'w'), indent=1, sort_keys=True)
  print('wrote', OUT)


if __name__ == '__main__':
  main()
