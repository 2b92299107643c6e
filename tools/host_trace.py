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
             trainer      (on request: --modes trainer; --configs is not used) two train.Trainer.train_step calls of three
                          trainers: a plain one, one with KD + mixup type 2, one made with recorded=True that runs DropBlock
                          from its static buffers with given draws; the digest covers both steps' loss rows and the arenas

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
DROPBLOCK = dict(resnet_version=2, use_sk_block=True, anti_alias_type='sconv', anti_alias_filter_size=3, use_resnet_d=True,
                 use_dropblock=True, dropblock_kp=[0.9, 0.6], train_epochs=1, num_images_train=8)
TRAINERS = {'plain': dict(resnet_version=1), 'kd-mixup2': dict(resnet_version=1, kd_temp=2.0, mixup_type=2),
            'dropblock': DROPBLOCK}


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


def run_trainer(name):
  import torch
  from assembled_cnn_amd import lib, ops
  from assembled_cnn_amd.train import HParams, Trainer
  from tests import model_parity as MP
  from tests.cpu_double import CpuDouble
  sigs = dict(lib.SIGNATURES)
  sigs.update(lib.DEBUG_SIGNATURES)
  proxy = LoggingLibrary(CpuDouble(), sigs)
  ops.set_library(proxy, is_double=True)
  ops.refresh_tuning()
  g = torch.Generator().manual_seed(7)
  B, size = (8, 64) if name == 'kd-mixup2' else (2, 224 if name == 'dropblock' else 64)    # DropBlock: maps >= 7 x 7
  hp = HParams(batch_size=B, learning_rate_decay_type='fixed', base_learning_rate=0.01, **TRAINERS[name])
  img, _, labels = MP.inputs(B, size)
  args, kwargs = [(img, labels)] * 2, [{}, {}]
  if name == 'kd-mixup2':
    soft = torch.cat([torch.nn.functional.one_hot(labels.long(), hp.num_classes).float(),
                      torch.randn((B, hp.num_classes), generator=g) * 2.0], 1)
    args = [(img, soft, torch.rand(B // 2, generator=g), torch.rand(B // 2, generator=g)) for _ in range(2)]
  if name == 'dropblock':       # a throw-away trainer discovers the shapes of the draws (creation order)
    probe = Trainer(hp, seed=0, device='cpu', recorded=True)
    probe.train_step(img, labels)
    kwargs = [{'dropblock_uniforms': [torch.rand(tuple(u.shape), generator=g) for (u, _, _, _) in probe._db.slots]}
              for _ in range(2)]
  tr = Trainer(hp, seed=0, device='cpu', recorded=True if name == 'dropblock' else None)
  del proxy.log[:]                               # the case starts after the model is built and its weights are loaded
  losses = [tr.train_step(*a, **k).clone() for a, k in zip(args, kwargs)]
  a = tr.model.arena
  data = [t.detach().float().contiguous().numpy().tobytes() for t in losses + [a.g32, a.w32, a.m32, a.state]]
  return len(proxy.log), sha('\n'.join(proxy.log).encode()), sha(*data)


def child(knob_set, configs, modes, threads):
  import torch
  torch.set_num_threads(threads)
  sys.path.insert(0, ROOT)
  for name in configs:
    for mode in [m for m in modes if m != 'trainer']:
      n, calls, data = run_case(name, mode)
      print('| %-15s | %-15s | %-10s | %5d | %s | %s |' % (name, knob_set, mode, n, calls, data), flush=True)
  for name in TRAINERS if 'trainer' in modes else ():
    n, calls, data = run_trainer(name)
    print('| %-15s | %-15s | %-10s | %5d | %s | %s |' % (name, knob_set, 'trainer', n, calls, data), flush=True)


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
