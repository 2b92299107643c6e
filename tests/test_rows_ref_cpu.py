"""tests/rows_ref.py against oracle/assembled_oracle.py on the same inputs, to the float32 round-off of the oracle: the
references the GPU module (tests/test_gpu_rows_edges.py) trusts are proved on the CPU first.  The oracle evaluates in float32,
the references in float64, so the allowed difference is a few float32 roundings of the largest term involved.

``-s`` prints the reference floors (max |float64 reference - float32 reference| per bf16-output case) that
profiles/rows_edges_tolerances.md records."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import assembled_oracle as O
from tests import rows_ref as R

U = 2.0 ** -24


def _close(ref, got, k, mag=None, what=''):
  """|got - ref| <= k float32 half-ulps of ``mag`` (default: max |ref|, the size of the terms the oracle summed)"""
  ref, got = np.asarray(ref, np.float64), np.asarray(got.detach().numpy() if torch.is_tensor(got) else got, np.float64)
  m = float(np.max(np.abs(ref))) if mag is None else mag
  err = float(np.max(np.abs(ref - got))) if ref.size else 0.0
  assert err <= k * U * m, '%s: %.3e > %.3e' % (what, err, k * U * m)


@pytest.mark.parametrize('B,C,soft', [(1, 1, False), (17, 5, True), (33, 257, True), (9, 1001, False)])
def test_sigmoid_ce_reference(B, C, soft):
  z, y = R.sigmoid_inputs(B, C, soft)
  loss, tot, dz = R.sigmoid_ce(z, y, 4.0)
  zt = torch.from_numpy(z).requires_grad_(True)
  lo = O.get_sup_loss(zt, torch.from_numpy(y), 'sigmoid')
  (g,) = torch.autograd.grad(lo * 4.0, zt)
  _close(loss, lo, 8 * np.log2(B * C + 2), what='loss')         # a float32 tree sum of B C terms
  _close(dz, g, 16, what='dz')
  assert abs(tot - float(y.astype(np.float64).sum())) == 0.0


@pytest.mark.parametrize('B,C,eps,T,offset', [(1, 1, 0.0, 0.0, 0), (5, 7, 0.1, 2.0, 1e4), (4, 257, 0.1, 0.0, 1e4),
                                              (3, 1001, 0.0, 1.0, 0)])
def test_softmax_ce_reference(B, C, eps, T, offset):
  z, y, t = R.softmax_inputs(B, C, offset)
  rows, dz = R.softmax_ce(z, y, t if T else None, eps, T, 3.0)
  zt = torch.from_numpy(z).requires_grad_(True)
  lo = O.softmax_cross_entropy(zt, torch.from_numpy(y), eps)
  if T:
    lo = lo + O.kd_loss(zt, torch.from_numpy(t), T)
  (g,) = torch.autograd.grad(lo * 3.0, zt)
  # log_softmax of the oracle carries the rounding of z - max, |z - max| <= ~40: the terms are that large
  span = float(np.max(z.max(1) - z.min(1))) + 1.0
  _close(rows.mean(), lo, 16 * (1 + T * T), mag=span, what='loss')
  _close(dz, g, 16 * (1 + T), mag=3.0 / B, what='dz')


def test_eval_rows_reference_rules():
  """the two tie rules and the label guard against torch (argmax = first maximum) and the in_top_k sentence itself"""
  r = R.rng(7)
  z = np.round(r.standard_normal((40, 9)) * 2)            # integers: many ties
  labels = r.integers(-1, 10, 40)
  pred, conf, top1, top5 = R.eval_rows(z, labels)
  for b in range(40):
    first = int(np.flatnonzero(z[b] == z[b].max())[0])
    assert pred[b] == first and top1[b] == float(first == labels[b])
    ok = 0 <= labels[b] < 9
    assert top5[b] == float(ok and (z[b] > z[b, labels[b] if ok else 0]).sum() < 5)
  _close(conf, torch.softmax(torch.from_numpy(z), 1).max(1).values, 4, what='conf')
  # stated cases: 4 strictly larger and ties with the label -> hit; 5 strictly larger -> miss
  row = np.array([[9, 8, 7, 6, 1, 1, 1, 0.], [9, 8, 7, 6, 5, 1, 1, 0.]])
  assert R.eval_rows(row, [5, 5])[3].tolist() == [1.0, 0.0]


@pytest.mark.parametrize('N,HW,C,p', [(1, 1, 8, 3.0), (2, 9, 24, 2.5), (2, 12, 40, 3.0)])
def test_gem_reference(N, HW, C, p):
  x, dy = R.gem_inputs(N, HW, C)
  y, s, dx = R.gem(x, p, dy)
  xt = torch.from_numpy(x).permute(0, 2, 1).reshape(N, C, HW, 1).clone().requires_grad_(True)
  yo = O.generalized_mean_pooling(xt, p)
  (g,) = torch.autograd.grad(yo, xt, torch.from_numpy(dy).view(N, C, 1, 1))
  _close(y, yo.view(N, C), 16, what='y')
  _close(dx, g.view(N, C, HW).permute(0, 2, 1), 32, what='dx')
  assert (dx[x <= 0] == 0).all() and (dx[:, :, C // 2] == 0).all() and (s[:, C // 2] == R.GEM_EPS).all()


@pytest.mark.parametrize('bs', [1, 2, 4, 6, 7])
@pytest.mark.parametrize('kind', ['none', 'mid'])
def test_dropblock_reference(bs, kind):
  """keep and scale against O.dropblock, even block sizes (asymmetric padding) included.  gamma = 0 through keep_prob 1 - 0:
  the oracle returns early at keep_prob == 1.0 exactly, so 'none' uses a gamma_scale that makes gamma tiny instead."""
  for H, W in [(7, 7), (9, 12), (bs, bs), (bs, bs + 3)]:
    C = 8
    gs = 1.0 if kind == 'mid' else 1e-30
    gamma = np.float32(gs * 0.2 * (W * H) / (bs ** 2) / ((W - bs + 1) * (H - bs + 1)))
    u = R.dropblock_uniform(H, W, C, bs, gamma)
    keep = R.dropblock_keep(u, gamma, H, W, bs)
    scale = R.dropblock_scale(keep)
    x = np.ones((1, C, H, W), np.float32)
    yo = O.dropblock(torch.from_numpy(x), 0.8, bs, gs, True, torch.from_numpy(u).permute(2, 0, 1)[None])
    _close(np.transpose(keep, (2, 0, 1))[None] * float(scale), yo, 4, what='keep * scale %dx%d' % (H, W))
    if kind == 'none':
      assert keep.min() == 1.0 and scale == 1.0
  # drop everything: gamma = 2 exceeds every draw
  keep = R.dropblock_keep(R.rng(3).random((8 - bs, 8 - bs, 8)), 2.0, 7, 7, bs)
  assert keep.max() == 0.0 and R.dropblock_scale(keep) == np.float32(392) / np.float32(1e-8)


def test_upsample_reference():
  r = R.rng(9)
  dy = R.bf16_randn(r, (2, 6, 10, 16))
  mask = r.integers(0, 256, (2 * 6 * 10, 2), dtype=np.uint8)
  g = torch.from_numpy(dy).permute(0, 3, 1, 2)
  _close(R.upsample2x_bwd(dy), (F.avg_pool2d(g, 2) * 4).permute(0, 2, 3, 1), 4, what='plain')
  bits = torch.from_numpy(R.unpack_mask(mask, 16).reshape(2, 6, 10, 16)).permute(0, 3, 1, 2).float()
  _close(R.upsample2x_bwd(dy, mask), (F.avg_pool2d(g * bits, 2) * 4).permute(0, 2, 3, 1), 4, what='masked')
  assert R.unpack_mask(np.array([[0b00000101]], np.uint8), 8).tolist() == [[1, 0, 1, 0, 0, 0, 0, 0]]


@pytest.mark.parametrize('N,HW,C,blocks', [(4, 9, 8, 5), (3, 25, 24, 2)])
def test_bn_references_against_oracle_autograd(N, HW, C, blocks):
  """partials of a real tensor -> bn_finalize / bn_bwd_finalize (plain and raw) vs O.batch_norm and its autograd; the
  compaction of the partials changes nothing"""
  r = R.rng(11, N, HW, C)
  M = N * HW
  x = (r.standard_normal((M, C)) * 2 + 0.5).astype(np.float32)
  dy = r.standard_normal((M, C)).astype(np.float32)
  vs = O.VarStore(0)
  ctx = O.Ctx(vs)
  vs.begin_call()
  gamma, beta, mm, mv, mm_name, mv_name = vs.bn_vars(C, False, 'bn')
  with torch.no_grad():
    gamma.copy_(torch.from_numpy(r.uniform(0.5, 1.5, C)))
    beta.copy_(torch.from_numpy(r.standard_normal(C)))
    mm.copy_(torch.from_numpy(r.standard_normal(C)))
    mv.copy_(torch.from_numpy(r.uniform(0.5, 1.5, C)))
  vs.begin_call()
  xt = torch.from_numpy(x).view(N, HW, 1, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
  yo = O.batch_norm(ctx, xt, True, momentum=0.9, epsilon=1e-5, layer_name='bn')
  gx, gg, gb = torch.autograd.grad(yo, [xt, gamma, beta], torch.from_numpy(dy).view(N, HW, 1, C).permute(0, 3, 1, 2))
  chunks = np.array_split(np.arange(M), blocks)
  x64, d64 = x.astype(np.float64), dy.astype(np.float64)
  part = np.stack([np.stack([x64[i].sum(0), (x64[i] ** 2).sum(0)]) for i in chunks])
  gn, bt = gamma.detach().numpy(), beta.detach().numpy()
  f = R.bn_finalize(part, M, gn, bt, 1e-5, 0.9, mm.numpy(), mv.numpy())
  f2 = R.bn_finalize(R.compact(part, 2), M, gn, bt, 1e-5, 0.9, mm.numpy(), mv.numpy())
  for k in ('mean', 'invstd', 'scale', 'shift', 'moving_mean', 'moving_var'):
    _close(f[k], f2[k], 1e-6, mag=1.0, what='compact ' + k)
  y = x64 * f['scale'] + f['shift']
  _close(y, yo.permute(0, 2, 3, 1).reshape(M, C), 16, what='y')
  _close(f['moving_mean'], vs.pending_updates[mm_name], 8, what='moving mean')
  _close(f['moving_var'], vs.pending_updates[mv_name], 16, what='moving variance')
  xhat = (x64 - f['mean']) * f['invstd']
  pb = np.stack([np.stack([d64[i].sum(0), (d64[i] * xhat[i]).sum(0)]) for i in chunks])
  praw = np.stack([np.stack([d64[i].sum(0), (d64[i] * x64[i]).sum(0)]) for i in chunks])
  for raw, p in ((False, pb), (True, praw)):
    b = R.bn_bwd_finalize(p, M, gn, f['mean'], f['invstd'], raw=raw)
    _close(b['dbeta'], gb, 8 * np.log2(M), what='dbeta')
    _close(b['dgamma'], gg, 8 * np.log2(M), mag=float(np.abs(d64 * xhat).max()) * 4, what='dgamma')
    dx = b['A'] * d64 + b['B'] * x64 + b['C']
    _close(dx, gx.permute(0, 2, 3, 1).reshape(M, C), 64, what='dx')


@pytest.mark.parametrize('mixup_type', [0, 1, 2])
@pytest.mark.parametrize('Bin,H,W', [(2, 1, 4), (6, 3, 5)])
def test_mixup_meansub_and_labels_reference(Bin, H, W, mixup_type):
  r = R.rng(15, Bin, H, W, mixup_type)
  img = r.integers(0, 256, (Bin, H, W, 3)).astype(np.float32)
  y = np.eye(11, dtype=np.float32)[r.integers(0, 11, Bin)]
  lam1, lam2 = r.random(Bin // 2).astype(np.float32), r.random(Bin // 2).astype(np.float32)
  x = O.mean_image_subtraction(torch.from_numpy(img))
  if mixup_type == 0:
    xr, yr = x, torch.from_numpy(y)
  else:
    xr, yr, _ = O.mixup(x, torch.from_numpy(y), torch.from_numpy(lam1), keep_batch_size=(mixup_type == 2),
                        lam2=torch.from_numpy(lam2))
  out = R.mixup_meansub(img, mixup_type, lam1, lam2)
  assert out.shape == (xr.shape[0], H + 6, W + 6, 4)
  _close(out[:, 3:3 + H, 3:3 + W, :3], xr, 8, mag=256.0, what='mixed images')
  halo = out.copy()
  halo[:, 3:3 + H, 3:3 + W, :3] = 0
  assert (halo == 0).all()
  _close(sum(R.mixup_terms(y, mixup_type, lam1, lam2)), yr, 4, mag=1.0, what='mixed labels')
  if mixup_type:      # lambda = 1 gives the first operand, lambda = 0 the second
    one, zero = np.ones(Bin // 2, np.float32), np.zeros(Bin // 2, np.float32)
    fa, fb, _ = R.mixup_operands(img, mixup_type, lam1, lam2)
    assert np.array_equal(sum(R.mixup_terms(img, mixup_type, one, one)), fa)
    assert np.array_equal(sum(R.mixup_terms(img, mixup_type, zero, zero)), fb)
    if mixup_type == 2:
      assert np.array_equal(fb[Bin // 2:], img[Bin // 2:][::-1]) and np.array_equal(fa[Bin // 2:], img[:Bin // 2])


@pytest.mark.parametrize('wd,gs', [(1e-4, 1.0 / 128), (0.0, 1.0)])
def test_sgd_reference(wd, gs):
  r = R.rng(16)
  n = 1027
  w, a = r.standard_normal(n).astype(np.float32), (r.standard_normal(n) * 0.1).astype(np.float32)
  g = (r.standard_normal(n) / gs).astype(np.float32)
  ta, tw = R.sgd_terms(w, a, g, 0.1, 0.9, wd, gs)
  wr, ar = torch.from_numpy(w.copy()), torch.from_numpy(a.copy())
  O.momentum_step([wr], [torch.from_numpy(g) * np.float32(gs) + np.float32(wd) * torch.from_numpy(w)], [ar], 0.1, 0.9)
  _close(sum(ta), ar, 8, what='accum')
  _close(sum(tw), wr, 8, what='w')


def test_layout_references():
  r = R.rng(13)
  w = r.standard_normal((5, 2, 3, 8)).astype(np.float32)
  wt = R.filter_transpose(w, 8)
  assert wt.shape == (8, 2, 3, 8) and (wt[..., 5:] == 0).all()
  assert np.array_equal(wt[..., :5], torch.from_numpy(w).permute(3, 1, 2, 0).numpy())
  for k in (3, 7):
    ws = r.standard_normal((4, k, k, 3)).astype(np.float32)
    p = R.stem_pack(ws)
    L = R.stem_lanes(k)
    assert p.shape == (4, k, L) and L % 8 == 0 and L >= 4 * k
    # the packed row is the [s][4] image of the master row: channel 3 and the lanes past 4 k are zero
    q = p[:, :, :4 * k].reshape(4, k, k, 4)
    assert np.array_equal(q[..., :3], torch.from_numpy(ws).bfloat16().float().numpy())
    assert (q[..., 3] == 0).all() and (p[:, :, 4 * k:] == 0).all()
    assert np.array_equal(R.stem_unpack(p, k), q[..., :3])
  x = r.standard_normal(4096).astype(np.float32) * 10.0 ** r.uniform(-20, 20, 4096).astype(np.float32)
  assert np.array_equal(R.to_bf16(x), torch.from_numpy(x).bfloat16().float().numpy())


def test_reference_floors():
  """the floors the GPU module adds (x 4) to one bf16 ulp: reported with -s, and small against the outputs they bound"""
  rows = []
  for B, C in [(1, 1), (17, 5), (600, 257), (600, 1001)]:
    z, y = R.sigmoid_inputs(B, C, True)
    rows.append(('sigmoid_ce dz B=%d C=%d' % (B, C), R.floor_of(lambda dt: R.sigmoid_ce(z, y, 4.0, dt)[2]),
                 np.abs(R.sigmoid_ce(z, y, 4.0)[2]).max()))
  for B, C in [(1, 7), (5, 257)]:
    z, y, t = R.softmax_inputs(B, C, 1e4)
    rows.append(('softmax_ce dz B=%d C=%d' % (B, C), R.floor_of(lambda dt: R.softmax_ce(z, y, t, 0.1, 2.0, 3.0, dt)[1]),
                 np.abs(R.softmax_ce(z, y, t, 0.1, 2.0, 3.0)[1]).max()))
  for (N, HW, C), p in [((3, 49, 256), 3.0), ((2, 9, 24), 2.5)]:
    x, dy = R.gem_inputs(N, HW, C)
    rows.append(('gem y p=%g' % p, R.floor_of(lambda dt: R.gem(x, p, None, dt)[0]), np.abs(R.gem(x, p)[0]).max()))
    rows.append(('gem dx p=%g' % p, R.floor_of(lambda dt: R.gem(x, p, dy, dt)[2]), np.abs(R.gem(x, p, dy)[2]).max()))
  for bs, H, W, C, kind in [(2, 9, 12, 72, 'mid'), (6, 7, 7, 72, 'all')]:
    gamma = R.dropblock_gamma(kind, H, W, bs)
    keep = R.dropblock_keep(R.dropblock_uniform(H, W, C, bs, gamma), gamma, H, W, bs)
    sc = float(R.dropblock_scale(keep))
    x = R.bf16_randn(R.rng(8, bs, H, W, C), (3, H, W, C))
    rows.append(('dropblock_apply bs=%d gamma %s' % (bs, kind), R.floor_of(lambda dt: R.dropblock_apply(x, keep, sc, dtype=dt)),
                 np.abs(R.dropblock_apply(x, keep, sc)).max()))
  dy = R.bf16_randn(R.rng(1), (2, 6, 10, 72))
  rows.append(('upsample2x_bwd', R.floor_of(lambda dt: R.upsample2x_bwd(dy, None, dt)), np.abs(R.upsample2x_bwd(dy)).max()))
  for name, fl, mx in rows:
    print('\nreference floor  %-28s %.3e   (max |ref| %.3e)' % (name, fl, mx), end='')
  for name, fl, mx in rows:
    assert fl <= 2.0 ** -16 * mx, name       # far below the bf16 ulp it is added to
