#!/usr/bin/env python
"""Micro-benchmark of the batch-norm kernels on the workload's tensor shapes (GPU only): effective TB/s.

--digest: no timing; for a fixed seeded input per (op, shape) print a sha256 of every output tensor, so that two builds of
the library (ASM_HIP_LIB=<other build>) can be compared bit for bit."""
import argparse, hashlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from assembled_cnn_amd import ops
from assembled_cnn_amd.ops import L, _ptr, _stream, check

SHAPES = [(256 * 112 * 112, 64), (256 * 112 * 112, 32), (256 * 56 * 56, 128), (256 * 56 * 56, 256), (256 * 56 * 56, 64),
          (256 * 28 * 28, 512), (256 * 28 * 28, 256), (256 * 14 * 14, 1024), (256 * 14 * 14, 512), (256 * 7 * 7, 2048),
          (256 * 7 * 7, 512)]
SMALL_SHAPE = (256, 32)          # bn_small_fwd / bwd   (tests/test_gpu_ops.py: test_bn_small_fused)
SK_SHAPE = (4, 14, 14, 64)       # N, H, W, F of an SK unit   (test_sk_unit_with_bn_applied_on_the_fly_equals_materialised_path)

# (name, bytes per element) of the timed kernels, in the order of the columns
TIMED = [('bn_stats', 2.0), ('bwd_reduce', 4.125), ('bwd_apply', 6.125), ('apply+relu', 4.125), ('apply+res+relu', 6.125),
         ('bwd_reduce2', 6.125), ('bwd_apply2', 10.125), ('apply2+relu', 6.125)]


def timeit(fn, iters=10):
  fn(); fn()
  torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(iters):
    fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) / iters * 1e3


class Case:
  """seeded inputs of one [M, C] shape and the batch-norm calls on them; every call returns its output tensors"""

  def __init__(self, M, Cn):
    g = torch.Generator(device='cuda').manual_seed(0)
    self.M, self.Cn = M, Cn
    rnd = lambda *shape: torch.randn(shape, generator=g, device='cuda')
    self.x, self.dy, self.res = rnd(M, Cn).to(torch.bfloat16), rnd(M, Cn).to(torch.bfloat16), rnd(M, Cn).to(torch.bfloat16)
    self.gamma, self.beta = torch.ones(Cn, device='cuda'), torch.zeros(Cn, device='cuda')
    self.co = rnd(6, Cn)
    self.part = ops.bn_stats(self.x, M, Cn)
    self.mean, self.invstd, self.scale, self.shift = ops.bn_finalize(self.part, M, Cn, self.gamma, self.beta, 1e-5, 0.997, None, None)
    _, self.mask = ops.bn_apply(self.x, M, Cn, self.scale, self.shift, relu=True, want_mask=True)
    self.blocks = L().asm_bn_stats_blocks(M, Cn)
    self.p2, self.p3 = (torch.empty((self.blocks, 2, Cn), device='cuda') for _ in range(2))
    self.dx, self.dx2 = torch.empty_like(self.x), torch.empty_like(self.x)

  def bn_stats(self):
    return (ops.bn_stats(self.x, self.M, self.Cn),)

  def bwd_reduce(self, relu=2):
    yout = (None, self.res, self.mask)[relu]
    check(L().asm_bn_bwd_reduce(_ptr(self.dy), _ptr(self.x), _ptr(yout), relu, self.M, self.Cn, _ptr(self.mean), _ptr(self.invstd),
                                _ptr(self.p2), _stream()), 'bn_bwd_reduce')
    return (self.p2,)

  def bwd_apply(self, relu=2):
    yout, co = (None, self.res, self.mask)[relu], self.co
    check(L().asm_bn_bwd_apply(_ptr(self.dy), _ptr(self.x), _ptr(yout), relu, self.M, self.Cn, _ptr(co[0]), _ptr(co[1]), _ptr(co[2]),
                               _ptr(self.dx), None, _stream()), 'bn_bwd_apply')
    return (self.dx,)

  def apply_relu(self):
    return ops.bn_apply(self.x, self.M, self.Cn, self.scale, self.shift, relu=True, want_mask=True)

  def apply_res_relu(self):
    return ops.bn_apply(self.x, self.M, self.Cn, self.scale, self.shift, residual=self.res, res_mode=1, relu=True, want_mask=True)

  def bwd_reduce2(self):
    check(L().asm_bn_bwd_reduce2(_ptr(self.dy), _ptr(self.x), _ptr(self.res), _ptr(self.mask), self.M, self.Cn, _ptr(self.mean),
                                 _ptr(self.invstd), _ptr(self.shift), _ptr(self.scale), _ptr(self.p2), _ptr(self.p3), _stream()),
          'bn_bwd_reduce2')
    return self.p2, self.p3

  def bwd_apply2(self):
    check(L().asm_bn_bwd_apply2(_ptr(self.dy), _ptr(self.x), _ptr(self.res), _ptr(self.mask), self.M, self.Cn, _ptr(self.co),
                                _ptr(self.dx), _ptr(self.dx2), _stream()), 'bn_bwd_apply2')
    return self.dx, self.dx2

  def apply2_relu(self):
    co = self.co
    return ops.bn_apply_dual(self.x, self.res, self.M, self.Cn, co[0], co[1], co[2], co[3], True, want_mask=True)

  def timed(self):
    return [self.bn_stats, self.bwd_reduce, self.bwd_apply, self.apply_relu, self.apply_res_relu, self.bwd_reduce2,
            self.bwd_apply2, self.apply2_relu]

  def finalize(self):
    mm, mv = torch.zeros(self.Cn, device='cuda'), torch.ones(self.Cn, device='cuda')
    return ops.bn_finalize(self.part, self.M, self.Cn, self.gamma, self.beta, 1e-5, 0.997, mm, mv) + (mm, mv)

  def bwd_finalize(self, raw):
    out = torch.empty((5, self.Cn), device='cuda')       # dgamma, dbeta, A, B, C
    ops._bn_bwd_coeffs(self.bwd_reduce()[0], self.M, self.Cn, self.gamma, self.mean, self.invstd, out[0], out[1], out[2:], raw=raw)
    return (out,)


def sha(t):
  return hashlib.sha256(t.contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def emit(op, shape, outs):
  for i, t in enumerate(outs):
    if t is not None:
      print('%-22s %-20s out%d %s' % (op, 'x'.join(str(s) for s in shape), i, sha(t)), flush=True)


def digest():
  for M, Cn in SHAPES + [SMALL_SHAPE]:
    c = Case(M, Cn)
    for (name, _), fn in zip(TIMED, c.timed()):
      emit(name, (M, Cn), fn())
    for relu in (0, 1):
      emit('bwd_reduce relu=%d' % relu, (M, Cn), c.bwd_reduce(relu))
      emit('bwd_apply relu=%d' % relu, (M, Cn), c.bwd_apply(relu))
    emit('bn_finalize', (M, Cn), c.finalize())
    emit('bn_bwd_finalize', (M, Cn), c.bwd_finalize(False))
    emit('bn_bwd_finalize_raw', (M, Cn), c.bwd_finalize(True))
    if M <= L().asm_bn_small_max_rows():
      mm, mv = torch.zeros(Cn, device='cuda'), torch.ones(Cn, device='cuda')
      y, mask, mean, invstd = ops.bn_small_fwd(c.x, M, Cn, c.gamma, c.beta, 1e-5, 0.997, mm, mv, True, True)
      emit('bn_small_fwd', (M, Cn), (y, mask, mean, invstd, mm, mv))
      dg, db = torch.empty(Cn, device='cuda'), torch.empty(Cn, device='cuda')
      emit('bn_small_bwd', (M, Cn), (ops.bn_small_bwd(c.dy, c.x, mask, M, Cn, c.gamma, mean, invstd, dg, db), dg, db))
  # the SK unit's batch-norm backward: reduce + finalize + apply, and the factorised form (sk_bn_bwd_finalize + apply)
  N, H, W, F_ = SK_SHAPE
  C2, M = 2 * F_, N * H * W
  g = torch.Generator(device='cuda').manual_seed(0)
  y = (torch.randn((N, H, W, C2), generator=g, device='cuda') * 1.5 + 0.2).to(torch.bfloat16)
  gamma = torch.rand(C2, generator=g, device='cuda') + 0.5
  beta = torch.randn(C2, generator=g, device='cuda') * 0.3
  att = torch.randn((N, 1, 1, C2), generator=g, device='cuda') * 2
  dv = torch.randn((N, H, W, F_), generator=g, device='cuda').to(torch.bfloat16)
  ds = torch.randn((N, 1, 1, F_), generator=g, device='cuda').to(torch.bfloat16)
  mean, invstd, scale, shift = ops.bn_finalize(ops.bn_stats(y.view(M, C2), M, C2), M, C2, gamma, beta, 1e-5, 0.997, None, None)
  part = torch.empty((L().asm_sk_bn_bwd_blocks(N, H * W, F_), 2, C2), device='cuda')
  check(L().asm_sk_bn_bwd_reduce(_ptr(dv), _ptr(att), _ptr(ds), _ptr(y), _ptr(scale), _ptr(shift), _ptr(mean), _ptr(invstd), N,
                                 H * W, F_, _ptr(part), _stream()), 'sk_bn_bwd_reduce')
  emit('sk_bn_bwd_reduce', SK_SHAPE, (part,))
  dg, db = torch.empty(C2, device='cuda'), torch.empty(C2, device='cuda')
  emit('sk_bn_bwd (reduce)', SK_SHAPE, (ops.sk_bn_bwd(dv, att, ds, y, scale, shift, gamma, mean, invstd, dg, db, F_), dg, db))
  _, mst = ops.sk_gap_bn(y, scale, shift, F_, mean, invstd)
  _, gst = ops.sk_select_bn_bwd_att(y, scale, shift, dv, att, F_, mean, invstd)
  emit('sk_bn_bwd (finalize)', SK_SHAPE,
       (ops.sk_bn_bwd(dv, att, ds, y, scale, shift, gamma, mean, invstd, dg, db, F_, gst, mst), dg, db))


def bench():
  print('%-18s' % 'M x C' + ''.join(' | %-22s' % ('%s (%gB/el)' % t) for t in TIMED))
  tot = [0.0] * len(TIMED)
  for M, Cn in SHAPES:
    c = Case(M, Cn)
    ts = [timeit(fn) for fn in c.timed()]
    print('%9d x %-6d' % (M, Cn) + ''.join(' | %7.1f us %5.2f TB/s' % (t, b * M * Cn / t / 1e6) for t, (_, b) in zip(ts, TIMED)))
    tot = [a + t for a, t in zip(tot, ts)]
  print('sum us:', ['%s %.0f' % (name, t) for (name, _), t in zip(TIMED, tot)])


if __name__ == '__main__':
  ap = argparse.ArgumentParser(description=__doc__)
  ap.add_argument('--digest', action='store_true', help='print sha256 digests of every output instead of times')
  if ap.parse_args().digest:
    digest()
  else:
    bench()
