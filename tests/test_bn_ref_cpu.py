"""tests/bn_ref.py against oracle/assembled_oracle.py (batch_norm in its float32 mode, and autograd through it) on the same
inputs: the references tests/test_gpu_bn_edges.py trusts are proved on the CPU first.  The oracle evaluates in float32, the
references in float64, so the allowed difference is a few float32 roundings of the largest term involved -- the comparison
of tests/test_rows_ref_cpu.py (``_close``)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import assembled_oracle as O
from tests import bn_ref as B
from tests import rows_ref as R
from tests.test_rows_ref_cpu import _close

EPS, MOM = 1e-5, 0.9


def _nchw(a, N, H, W):
  """[N H W, C] numpy -> [N, C, H, W] float32 tensor"""
  return torch.from_numpy(np.asarray(a, np.float32)).view(N, H, W, -1).permute(0, 3, 1, 2).clone()


def _rows(t):
  """[N, C, H, W] tensor -> [N H W, C] float64"""
  return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double().numpy()


def _layer(vs, C, name, r):
  vs.begin_call()
  gamma, beta, mm, mv, mm_name, mv_name = vs.bn_vars(C, False, name)
  with torch.no_grad():
    gamma.copy_(torch.from_numpy(r.uniform(0.5, 1.5, C)))
    beta.copy_(torch.from_numpy(r.standard_normal(C) * 0.5))
    mm.copy_(torch.from_numpy(r.standard_normal(C)))
    mv.copy_(torch.from_numpy(r.uniform(0.5, 1.5, C)))
  return gamma, beta, mm, mv, mm_name, mv_name


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('res_mode', [0, 1, 2])
@pytest.mark.parametrize('N,H,W,C', [(1, 2, 2, 8), (3, 2, 6, 24), (2, 4, 2, 72)])
def test_fwd_and_bwd_against_oracle_autograd(N, H, W, C, res_mode, relu):
  r = R.rng(201, N, H, W, C, res_mode, relu)
  M = N * H * W
  x = (r.standard_normal((M, C)) * 2 + 0.5).astype(np.float32)
  dy = r.standard_normal((M, C)).astype(np.float32)
  res = None if res_mode == 0 else r.standard_normal((M if res_mode == 1 else M // 4, C)).astype(np.float32)
  vs = O.VarStore(0)
  ctx = O.Ctx(vs)
  gamma, beta, mm, mv, mm_name, mv_name = _layer(vs, C, 'bn', r)
  vs.begin_call()
  xt = _nchw(x, N, H, W).requires_grad_(True)
  rt = None
  if res_mode == 1:
    rt = _nchw(res, N, H, W).requires_grad_(True)
    r_in = rt
  elif res_mode == 2:
    rt = _nchw(res, N, H // 2, W // 2).requires_grad_(True)
    r_in = F.interpolate(rt, scale_factor=2, mode='nearest')
  else:
    r_in = None
  yo = O.batch_norm(ctx, xt, True, momentum=MOM, epsilon=EPS, relu=relu, residual=r_in, layer_name='bn')
  grads = torch.autograd.grad(yo, [xt, gamma, beta] + ([rt] if rt is not None else []), _nchw(dy, N, H, W))
  gn, bt = gamma.detach().numpy(), beta.detach().numpy()
  f = B.fwd(x, gn, bt, EPS, MOM, mm.numpy(), mv.numpy(), res, res_mode, relu, H, W)
  s0, s1 = B.stats(x)
  _close(s0 / M, xt.detach().mean(dim=(0, 2, 3)), 8, mag=float(np.abs(x).max()), what='mean')
  _close(f['mean'], s0 / M, 1e-6, mag=1.0, what='mean of fwd')
  _close(f['invstd'], 1.0 / np.sqrt(np.maximum(s1 / M - (s0 / M) ** 2, 0) + np.float32(EPS)), 1e-6, mag=1.0, what='invstd')
  mag = float(np.abs(f['pre']).max()) + float(np.abs(x).max()) * float(np.abs(f['scale']).max())
  _close(f['y'], _rows(yo), 16, mag=mag, what='y')
  _close(f['moving_mean'], vs.pending_updates[mm_name], 8, what='moving mean')
  _close(f['moving_var'], vs.pending_updates[mv_name], 16, what='moving variance')
  # the mask bits are the forward output's sign wherever the float32 oracle is not within its round-off of zero
  yo_rows = _rows(O.batch_norm(O.Ctx(vs), xt, True, momentum=MOM, epsilon=EPS, relu=False, residual=r_in, layer_name='bn'))
  clear = np.abs(f['pre']) > 64 * 2.0 ** -24 * mag
  assert clear.mean() > 0.99 and np.array_equal(f['bits'][clear], (yo_rows > 0)[clear])
  if relu:
    assert (f['y'][~f['bits']] == 0).all() and (f['y'][f['bits']] > 0).all()
  # backward: the three mask kinds give one gate
  gate = None
  if relu:
    gate = B.gate_of(1, f['y'], C)
    assert np.array_equal(gate, B.gate_of(2, B.pack_mask(f['bits']), C)) and np.array_equal(gate, f['bits'].astype(np.float64))
  b = B.bwd(dy, x, gate, gn, f['mean'], f['invstd'], M)
  d64 = dy.astype(np.float64)
  xhat = (x.astype(np.float64) - f['mean']) * f['invstd']
  _close(b['dbeta'], grads[2], 8 * np.log2(M) + 8, mag=float(np.abs(d64).sum(0).max()), what='dbeta')
  _close(b['dgamma'], grads[1], 8 * np.log2(M) + 8, mag=float(np.abs(d64 * xhat).sum(0).max()) * 4, what='dgamma')
  _close(b['dx'], _rows(grads[0]), 64, mag=float(np.abs(b['A']).max() * np.abs(d64).max() * 4), what='dx')
  if res_mode == 1:
    _close(b['dz'], _rows(grads[3]), 4, what='residual gradient')
  elif res_mode == 2:
    _close(R.upsample2x_bwd(b['dz'].reshape(N, H, W, C)).reshape(-1, C), _rows(grads[3]), 8, what='upsampled residual gradient')
  # bwd_dx / bwd_sums are what bwd is made of
  sums = B.bwd_sums(dy, x, gate, f['mean'], f['invstd'])
  assert np.array_equal(sums[0], b['dbeta']) and np.array_equal(sums[1], b['dgamma'])
  assert np.array_equal(B.bwd_dx(b['dz'], x, b['A'], b['B'], b['C']), b['dx'])


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('N,H,W,C', [(1, 2, 2, 8), (3, 2, 6, 24), (2, 4, 2, 72)])
def test_dual_forms_against_oracle_autograd(N, H, W, C, relu):
  """out = [relu](bn_a(xa) + bf16(bn_b(xb))): the oracle's batch norm of xb, rounded to bf16 with the gradient passed
  straight through, is the residual of the oracle's batch norm of xa"""
  r = R.rng(202, N, H, W, C, relu)
  M = N * H * W
  xa = (r.standard_normal((M, C)) * 2 + 0.5).astype(np.float32)
  xb = (r.standard_normal((M, C)) * 0.5 - 1).astype(np.float32)
  dy = r.standard_normal((M, C)).astype(np.float32)
  vs = O.VarStore(0)
  ctx = O.Ctx(vs)
  la, lb = _layer(vs, C, 'a', r), _layer(vs, C, 'b', r)
  vs.begin_call()
  ta, tb = _nchw(xa, N, H, W).requires_grad_(True), _nchw(xb, N, H, W).requires_grad_(True)
  short = O.batch_norm(ctx, tb, True, momentum=MOM, epsilon=EPS, layer_name='b')
  rounded = short + (short.bfloat16().float() - short).detach()       # the bf16 value, the gradient straight through
  assert torch.equal(rounded, short.bfloat16().float())
  yo = O.batch_norm(ctx, ta, True, momentum=MOM, epsilon=EPS, relu=relu, residual=rounded, layer_name='a')
  ga, gga, gba, gb, ggb, gbb = torch.autograd.grad(yo, [ta, la[0], la[1], tb, lb[0], lb[1]], _nchw(dy, N, H, W))
  fa = B.fwd(xa, la[0].detach().numpy(), la[1].detach().numpy(), EPS)
  fb = B.fwd(xb, lb[0].detach().numpy(), lb[1].detach().numpy(), EPS)
  y, bits = B.apply_dual(xa, xb, fa['scale'], fa['shift'], fb['scale'], fb['shift'], relu)
  # the shortcut the oracle rounded (float32) and the one the reference rounded (float64) may land on two sides of a bf16
  # rounding boundary: the comparison is made where they agree, which is everywhere but a stray element
  same = R.to_bf16(fb['y']) == _rows(short.bfloat16().float())
  assert same.mean() > 0.99
  mag = float(np.abs(xa).max() * np.abs(fa['scale']).max() + np.abs(fa['shift']).max() + np.abs(fb['y']).max())
  _close(np.where(same, y, 0), np.where(same, _rows(yo), 0), 16, mag=mag, what='y')
  gate = bits.astype(np.float64) if relu else None
  ba, bb = B.bwd2(dy, xa, xb, gate, (la[0].detach().numpy(), fa['mean'], fa['invstd']),
                  (lb[0].detach().numpy(), fb['mean'], fb['invstd']), M)
  assert np.array_equal(ba['dbeta'], bb['dbeta'])          # both hold sum g
  d64 = dy.astype(np.float64)
  for name, b, f, x, (gx, gg, gbeta) in (('a', ba, fa, xa, (ga, gga, gba)), ('b', bb, fb, xb, (gb, ggb, gbb))):
    xhat = (x.astype(np.float64) - f['mean']) * f['invstd']
    _close(b['dbeta'], gbeta, 8 * np.log2(M) + 8, mag=float(np.abs(d64).sum(0).max()), what='dbeta ' + name)
    _close(b['dgamma'], gg, 8 * np.log2(M) + 8, mag=float(np.abs(d64 * xhat).sum(0).max()) * 4, what='dgamma ' + name)
    _close(b['dx'], _rows(gx), 64, mag=float(np.abs(b['A']).max() * np.abs(d64).max() * 4), what='dx ' + name)


def test_mask_packing_and_upsampling_are_the_layout_comments():
  bits = np.zeros((2, 16), np.uint8)
  bits[0, [0, 2]] = 1
  bits[1, 15] = 1
  assert B.pack_mask(bits).tolist() == [[0b00000101, 0], [0, 0b10000000]]
  assert np.array_equal(R.unpack_mask(B.pack_mask(bits), 16), bits)
  res = np.arange(2 * 1 * 2 * 8, dtype=np.float64).reshape(4, 8)          # N = 2, 1 x 2 low-resolution pixels
  up = B.upsample2x(res, 2, 2, 4).reshape(2, 2, 4, 8)
  for n in range(2):
    for h in range(2):
      for w in range(4):
        assert np.array_equal(up[n, h, w], res[n * 2 + w // 2])
  # zeros of either sign gate off
  assert B.gate_of(1, np.array([[0.0, -0.0, -1.0, 2.0, 0, 0, 0, 0]]), 8).tolist() == [[0, 0, 0, 1, 0, 0, 0, 0]]


def test_constant_channel_has_zero_variance_and_the_clamp_holds():
  """a constant integer channel: variance exactly 0, invstd = 1 / sqrt(eps), y = beta; a constant non-dyadic one in float32:
  E[x^2] - mean^2 cancels to a tiny value of either sign and the clamp keeps invstd <= 1 / sqrt(eps)"""
  M = 37
  x = np.stack([np.full(M, 3.0), R.to_bf16(np.full(M, 0.1, np.float32)).astype(np.float64)], axis=1)
  x = np.concatenate([x] * 4, axis=1)
  gamma, beta = np.full(8, 1.5), np.arange(8) * 0.25
  for dt in (np.float64, np.float32):
    f = B.fwd(x, gamma, beta, EPS, dtype=dt)
    top = 1.0 / np.sqrt(np.float64(np.float32(EPS)))
    assert (np.asarray(f['invstd'], np.float64) <= top * (1 + 2.0 ** -22)).all()
    _close(f['invstd'][0::2], np.full(4, top), 4, what='invstd of the integer constant')
    _close(f['y'][:, 0::2], np.broadcast_to(beta[0::2], (M, 4)), 4, what='y of the integer constant')
