#!/usr/bin/env python
"""What does the host code ask of the library?  Runs whole networks on the CPU test double of the C ABI
(tests/cpu_double.py) behind a proxy that logs every C-ABI call -- its name, every integer / float argument, a pointer as
null / non-null, a convolution descriptor as its fields -- and prints, per case, the number of calls, a sha256 of that log
and a sha256 of the bytes the case left behind (logits, gradient / weight / state arenas).  Two checkouts that print the
same table make the same calls in the same order with the same arguments and compute the same bits: the check for a
host-side refactor (run it from each checkout, diff the output).  Nothing is pinned: a change of launches changes the table.

Cases = configurations (tests/model_parity.CONFIGS, at the sizes tests/test_fusion_knobs_cpu.py uses) x knob sets x modes:
  knob sets  fused (every switch below on), plain (every one off), and each of ASM_BN_DUAL / ASM_BN_DEFER / ASM_LAZY_DZ /
             ASM_POOL_FUSE / ASM_BN_RED off alone.  Each knob set runs in a process of its own with the variables set before
             the package is imported, so switches read at import and switches read later are treated alike;
  modes      step         training forward with a tape + backward
             train_fwd    training forward without a tape
             eval         inference forward without a tape: batch norm folded into the conv epilogue (the stem, whose
                          pre-BN output the walker always taps as 'initial_conv', takes the un-folded tap form)
             eval_taped   inference forward with a tape: moving-statistics batch norm as its own pass in every layer

  python tools/host_trace.py [--configs a,b] [--knobs fused,plain,...] [--modes ...] [--jobs N] [--threads N]
"""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ['a-r50-d', 'a-r50-beta1-d', 'se-proj', 'r50v1', 'r50v1-d', 'r101v1-gem-emb']
SWITCHES = ['ASM_BN_DUAL', 'ASM_BN_DEFER', 'ASM_LAZY_DZ', 'ASM_POOL_FUSE', 'ASM_BN_RED', 'ASM_DENSE_SMALL', 'ASM_SK_FUSED']
ALONE = SWITCHES[:5]
KNOB_SETS = ['fused', 'plain'] + [k + '=0' for k in ALONE]
MODES = ['step', 'train_fwd', 'eval', 'eval_taped']
BATCH, SIZE = 2, 64


def knob_env(knob_set):
  env = {k: ('0' if knob_set == 'plain' else '1') for k in SWITCHES}
  if knob_set.endswith('=0'):
    env[knob_set[:-2]] = '0'
  return env


class LoggingLibrary(object):
  """forwards every asm_* call to the wrapped provider and logs it"""

  def __init__(self, inner, signatures):
    self._inner, self._sigs, self.log = inner, signatures, []

  def _arg(self, a, ctype):
    if hasattr(a, '_obj'):                        # ctypes.byref(struct)
      a = a._obj
    if isinstance(a, C.Structure):
      return '{%s}' % ','.join('%s=%d' % (f[0], getattr(a, f[0])) for f in a._fields_)
    if isinstance(a, C.Array):
      return 'array'
    if ctype is C.c_void_p or a is None:
      return 'ptr' if a else 'null'
    if isinstance(a, float):
      return a.hex()
    if isinstance(a, (bool, int)):
      return '%d' % a
    raise TypeError('host_trace: argument of type %s' % type(a).__name__)

  def __getattr__(self, name):
    fn = getattr(self._inner, name)
    if not name.startswith('asm_') or not callable(fn):
      return fn
    argtypes = self._sigs[name][1]

    def call(*args, **kwargs):
      if len(args) + len(kwargs) != len(argtypes):
        raise TypeError('host_trace: %s called with %d arguments, declared with %d' % (name, len(args) + len(kwargs), len(argtypes)))
      vals = list(args) + [kwargs[k] for k in sorted(kwargs)]
      self.log.append('%s(%s)' % (name, ' '.join(self._arg(a, t) for a, t in zip(vals, argtypes))))
      return fn(*args, **kwargs)
    return call


def sha(*chunks):
  h = hashlib.sha256()
  for c in chunks:
    h.update(c)
  return h.hexdigest()[:16]


def run_case(name, mode):
  import torch
  from assembled_cnn_amd import lib, ops
  from tests import model_parity as MP
  from tests.cpu_double import CpuDouble
  sigs = dict(lib.SIGNATURES)
  sigs.update(lib.DEBUG_SIGNATURES)
  proxy = LoggingLibrary(CpuDouble(), sigs)
  ops.set_library(proxy, is_double=True)
  ops.refresh_tuning()
  _, pm = MP.make_pair(name, 'cpu', BATCH, SIZE)
  _, x, _ = MP.inputs(BATCH, SIZE)
  del proxy.log[:]                               # the case starts after the model is built and its weights are loaded
  training = mode in ('step', 'train_fwd')
  taped = mode in ('step', 'eval_taped')
  logits = pm(x, training, use_resnet_d=MP.uses_d(name), record_tape=taped)
  if mode == 'step':
    dl = torch.zeros((BATCH, 1, 1, pm.ldc), dtype=torch.bfloat16)
    dl[:, 0, 0, :1001] = (torch.softmax(logits.float(), 1) / BATCH).to(torch.bfloat16)
    pm.backward(dl)
  a = pm.arena
  data = [t.detach().float().contiguous().numpy().tobytes() for t in (logits, a.g32, a.w32, a.state)]
  return len(proxy.log), sha('\n'.join(proxy.log).encode()), sha(*data)


def child(knob_set, configs, modes, threads):
  import torch
  torch.set_num_threads(threads)
  sys.path.insert(0, ROOT)
  for name in configs:
    for mode in modes:
      n, calls, data = run_case(name, mode)
      print('| %-15s | %-15s | %-10s | %5d | %s | %s |' % (name, knob_set, mode, n, calls, data), flush=True)


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--configs', default=','.join(CONFIGS))
  ap.add_argument('--knobs', default=','.join(KNOB_SETS))
  ap.add_argument('--modes', default=','.join(MODES))
  ap.add_argument('--jobs', type=int, default=4, help='knob sets run side by side')
  ap.add_argument('--threads', type=int, default=1, help='torch intra-op threads (fixed: the CPU sums are then reproducible)')
  ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
  args = ap.parse_args()
  configs, modes = args.configs.split(','), args.modes.split(',')
  if args.child is not None:
    return child(args.child, configs, modes, args.threads)
  print('| config          | knobs           | mode       | calls | sha256(call log) | sha256(logits, g32, w32, state) |')
  print('|---|---|---|---|---|---|')
  pending = args.knobs.split(',')
  running = []
  failed = False
  while pending or running:
    while pending and len(running) < max(1, args.jobs):
      ks = pending.pop(0)
      env = dict(os.environ, OMP_NUM_THREADS=str(args.threads), **knob_env(ks))
      cmd = [sys.executable, os.path.abspath(__file__), '--child', ks, '--configs', args.configs, '--modes', args.modes,
             '--threads', str(args.threads)]
      running.append((ks, subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)))
    ks, p = running.pop(0)                        # in the order they were started: the table's order is fixed
    out, _ = p.communicate()
    sys.stdout.write(out)
    sys.stdout.flush()
    if p.returncode != 0:
      print('host_trace: knob set %s failed (exit status %d)' % (ks, p.returncode), file=sys.stderr)
      failed = True
  return 1 if failed else 0


if __name__ == '__main__':
  sys.exit(main() or 0)
