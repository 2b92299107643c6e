"""tests/pool_ref.py against oracle/assembled_oracle.py and its autograd on the same float64 inputs: the references the GPU
module (tests/test_gpu_pool_edges.py) trusts are proved on the CPU first.  Both sides evaluate in float64, so they agree to a
few float64 roundings; 0/1 decisions (which tap of a max-pool window gets the gradient) agree exactly.

The max-pool cases use the tie inputs of the GPU module (post-ReLU grid values, a constant map): "the first maximum in
(r, s) scan order wins" is shown to be the oracle's rule for y and for dx.  Every pooling reference sees non-square maps.

``-s`` prints the reference floors (max |float64 reference - float32 reference| per case) that
profiles/pool_edges_tolerances.md records."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import assembled_oracle as O
from tests import pool_ref as P
from tests import rows_ref as R

EPS = 2.0 ** -52


def _nchw(a):
  return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
  return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def _close(ref, got, k=64, what=''):
  """|got - ref| <= k float64 ulps of the largest reference value (both sides are float64 sums of a few terms)"""
  ref, got = np.asarray(ref, np.float64), np.asarray(got.detach().numpy() if torch.is_tensor(got) else got, np.float64)
  assert ref.shape == got.shape, '%s: shape %s vs %s' % (what, ref.shape, got.shape)
  m = float(np.max(np.abs(ref))) if ref.size else 0.0
  err = float(np.max(np.abs(ref - got))) if ref.size else 0.0
  assert err <= k * EPS * max(m, 1e-30), '%s: %.3e > %.3e' % (what, err, k * EPS * m)


def _floor(what, fn):
  fl = R.floor_of(fn)
  print('\npool-ref floor %-52s %.3e' % (what, fl), end='')
  return fl


def maxpool_input(kind, shape):
  r = R.rng(11, *shape)
  if kind == 'grid':
    return P.grid(r, shape, relu=True)
  if kind == 'const':
    return np.full(shape, 1.5, np.float32)
  return R.bf16_randn(r, shape)


@pytest.mark.parametrize('kind', ['grid', 'const', 'random'])
@pytest.mark.parametrize('shape', P.MAXPOOL_SHAPES)
def test_maxpool_reference_and_first_maximum_rule(shape, kind):
  x = maxpool_input(kind, shape)
  dy = P.grid(R.rng(12, *shape), P.maxpool3x3s2(x)[0].shape)
  y, code = P.maxpool3x3s2(x)
  dx = P.maxpool3x3s2_bwd(dy, code, shape)
  xt = _nchw(x).requires_grad_(True)
  yo = O.max_pool_same(xt, 3, 2)
  (g,) = torch.autograd.grad(yo, xt, _nchw(dy))
  assert np.array_equal(y, _nhwc(yo)), 'y'
  assert np.array_equal(dx, _nhwc(g)), 'dx: the oracle sends the gradient of a tie to another tap'
  if kind == 'const':      # a full tie: the first VALID tap, which for odd H is r = 1 at ho = 0 (one row of padding before)
    N, H, W, C = shape
    first_r = 1 if P.same_pad(H, 3, 2)[1] else 0
    first_s = 1 if P.same_pad(W, 3, 2)[1] else 0
    assert (code[:, 0, 0] == first_r * 3 + first_s).all()
    assert (code[:, -1, -1] == (0 if code.shape[1] > 1 else first_r) * 3 + (0 if code.shape[2] > 1 else first_s)).all()


def _oracle_avgpool(xt, k, stride, count_valid):
  return O.avg_pool_same(xt, k, stride) if count_valid else O.avg_pool_valid(O.fixed_padding(xt, k), k, stride)


@pytest.mark.parametrize('form', P.AVG_FORMS)
@pytest.mark.parametrize('shape', P.AVG_SHAPES)
def test_avgpool_reference(shape, form):
  k, stride, pad, cv = form
  N, H, W, C = shape
  (Ho, ph), (Wo, pw) = P.avgpool_geometry(H, k, stride, cv), P.avgpool_geometry(W, k, stride, cv)
  assert ph == pad and pw == pad
  r = R.rng(21, *shape, k, stride, False)      # the random inputs of the GPU module's case: its floor is printed below
  x, dy, add = R.bf16_randn(r, shape), R.bf16_randn(r, (N, Ho, Wo, C)), R.bf16_randn(r, shape)
  xt = _nchw(x).requires_grad_(True)
  yo = _oracle_avgpool(xt, k, stride, cv)
  assert tuple(yo.shape) == (N, C, Ho, Wo)
  (g,) = torch.autograd.grad(yo, xt, _nchw(dy))
  _close(P.avgpool(x, k, stride, pad, Ho, Wo, cv), _nhwc(yo), what='y')
  _close(P.avgpool_bwd(dy, shape, k, stride, pad, cv), _nhwc(g), what='dx')
  _close(P.avgpool_bwd(dy, shape, k, stride, pad, cv, addend=add), _nhwc(g) + add.astype(np.float64), what='dx + addend')
  _floor('avgpool %s k%d s%d cv%d' % (shape, k, stride, cv), lambda dt: (
      P.avgpool(x, k, stride, pad, Ho, Wo, cv, dt), P.avgpool_bwd(dy, shape, k, stride, pad, cv, add, dt)))


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('shape,ks', P.BLUR_CASES)
def test_blurpool_reference(shape, ks, stride):
  ctx = O.Ctx(O.VarStore(dtype=torch.float64))
  for k in ks:
    N, H, W, C = shape
    r = R.rng(31, *shape, k, stride, False)      # the random inputs of the GPU module's case
    x = R.bf16_randn(r, shape)
    y = P.blurpool(x, k, stride)
    assert y.shape[1:3] == (P.blur_out(H, k, stride), P.blur_out(W, k, stride))
    dy = R.bf16_randn(r, y.shape)
    xt = _nchw(x).requires_grad_(True)
    yo = O.anti_aliased_downsample(ctx, xt, k, stride)
    (g,) = torch.autograd.grad(yo, xt, _nchw(dy))
    _close(y, _nhwc(yo), what='y k=%d' % k)
    _close(P.blurpool_bwd(dy, shape, k, stride), _nhwc(g), what='dx k=%d' % k)
    # the definition itself, independent of the oracle's function: reflect pad, then a depthwise convolution
    pad = (k - 1) // 2
    a = torch.tensor(P.BINOMIAL[k], dtype=torch.float64)
    w = (a[:, None] * a[None, :] / a.sum() ** 2).view(1, 1, k, k).repeat(C, 1, 1, 1)
    yd = F.conv2d(F.pad(_nchw(x), (pad, pad, pad, pad), mode='reflect') if pad else _nchw(x), w, stride=stride, groups=C)
    _close(y, _nhwc(yd), what='y against pad + conv k=%d' % k)
    _floor('blurpool %s k%d s%d' % (shape, k, stride),
           lambda dt: (P.blurpool(x, k, stride, dt), P.blurpool_bwd(dy, shape, k, stride, dt)))


ROW_SHAPES = [(2, 1, 8), (3, 5, 24), (3, 49, 40), (2, 33, 264), (2, 513, 72), (2, 641, 256)]


@pytest.mark.parametrize('N,HW,C', ROW_SHAPES)
def test_gap_sk_and_se_references(N, HW, C):
  r = R.rng(41, N, HW, C)
  t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))      # noqa: E731
  # global average pool and its adjoint
  x, dy = R.bf16_randn(r, (N, HW, C)), R.bf16_randn(r, (N, C))
  xt = t64(x).requires_grad_(True)
  yo = xt.mean(dim=1)
  (g,) = torch.autograd.grad(yo, xt, t64(dy))
  _close(P.gap(x), yo, what='gap')
  _close(P.gap_bwd(dy, (N, HW, C)), g, what='gap_bwd')
  _floor('gap HW=%d C=%d' % (HW, C), lambda dt: P.gap(x, dt))
  # selective kernel (nets/blocks.py:130-152 as the oracle's sk_conv2d writes them), gates at 0, +-30, +-100 among random ones
  Fh = C
  f, dv, ds = R.bf16_randn(r, (N, HW, 2 * Fh)), R.bf16_randn(r, (N, HW, Fh)), R.bf16_randn(r, (N, Fh))
  att = P.sk_logits(r, N, Fh)
  ft, at = t64(f).requires_grad_(True), t64(att).requires_grad_(True)
  f0, f1 = ft[:, :, :Fh], ft[:, :, Fh:]
  s = (f0 + f1).mean(dim=1)
  a = torch.softmax(torch.stack([at[:, :Fh], at[:, Fh:]], dim=0), dim=0)
  v = f0 * a[0][:, None] + f1 * a[1][:, None]
  gf, ga = torch.autograd.grad([v, s], [ft, at], [t64(dv), t64(ds)], allow_unused=True)
  _close(P.sk_gap(f, Fh), s, what='sk_gap')
  _close(P.sk_select(f, att), v, what='sk_select')
  _close(P.sk_select_bwd_att(f, dv, att), ga, k=64 * HW, what='sk_select_bwd_att')
  _close(P.sk_select_bwd_f(dv, att, ds), gf, what='sk_select_bwd_f')
  a0, a1 = P.sk_gates(att, Fh)
  hard = np.abs(att[:, :Fh] - att[:, Fh:]) == 100
  # float64 keeps exp(-100) = 3.7e-44, which float32 arithmetic loses against 1: the gates are 0 or 1 to that
  assert hard.any() and (np.minimum(a0[hard], a1[hard]) < 1e-43).all() and (np.maximum(a0[hard], a1[hard]) == 1.0).all()
  _floor('sk_gap HW=%d F=%d' % (HW, Fh), lambda dt: P.sk_gap(f, Fh, dt))
  _floor('sk_select HW=%d F=%d' % (HW, Fh), lambda dt: P.sk_select(f, att, dt))
  _floor('sk_select_bwd_att HW=%d F=%d' % (HW, Fh), lambda dt: P.sk_select_bwd_att(f, dv, att, dt))
  _floor('sk_select_bwd_f HW=%d F=%d' % (HW, Fh), lambda dt: P.sk_select_bwd_f(dv, att, ds, dt))
  # squeeze-excite (nets/blocks.py:182-183), e = +-100 among random ones
  e = P.se_logits(r, N, C)
  et = t64(e).requires_grad_(True)
  xt = t64(x).requires_grad_(True)
  g2 = R.bf16_randn(r, (N, HW, C))
  yo = xt * torch.sigmoid(et)[:, None]
  sq = xt.mean(dim=1)
  gx, ge = torch.autograd.grad([yo, sq], [xt, et], [t64(g2), t64(dy)], allow_unused=True)
  _close(P.se_scale(x, e), yo, what='se_scale')
  _close(P.se_scale_bwd_e(x, g2, e), ge, k=64 * HW, what='se_scale_bwd_e')
  _close(P.se_scale_bwd_x(g2, e, dy), gx, what='se_scale_bwd_x')
  sg = P.sigmoid(e)[np.abs(e) == 100]
  assert ((sg < 1e-43) | (sg == 1.0)).all()
  _floor('se_scale HW=%d C=%d' % (HW, C), lambda dt: P.se_scale(x, e, dt))
  _floor('se_scale_bwd_e HW=%d C=%d' % (HW, C), lambda dt: P.se_scale_bwd_e(x, g2, e, dt))
  _floor('se_scale_bwd_x HW=%d C=%d' % (HW, C), lambda dt: P.se_scale_bwd_x(g2, e, dy, dt))


@pytest.mark.parametrize('N,HW,Fh', [(1, 1, 8), (3, 3, 8), (1, 41, 24), (3, 29, 40)])
def test_fused_sk_reference_is_the_oracle_chain(N, HW, Fh):
  """batch_norm(relu=True) under bf16 storage emulation (f is rounded where the un-fused path stores it), the SK
  expressions of sk_conv2d on it, and autograd for dy, dgamma, dbeta and datt (df is never rounded: straight-through)"""
  d = P.fused_random_inputs(R.rng(51, N, HW, Fh), N, HW, Fh)
  C2 = 2 * Fh
  t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))      # noqa: E731
  # float64 statistics of y: the oracle derives its own, the reference takes them as inputs
  y64 = d['y'].astype(np.float64)
  mean = y64.mean(axis=(0, 1))
  invstd = 1.0 / np.sqrt(((y64 - mean) ** 2).mean(axis=(0, 1)) + 1e-5)
  gamma, beta = d['gamma'].astype(np.float64), d['beta'].astype(np.float64)
  scale = gamma * invstd
  shift = beta - mean * scale
  fwd = P.sk_fused_fwd(y64, scale, shift, d['att'])
  bwd = P.sk_fused_bwd(y64, scale, shift, gamma, mean, invstd, d['att'], d['dv'], d['ds'])

  vs = O.VarStore(dtype=torch.float64)
  ctx = O.Ctx(vs, emulate_bf16=True)
  yt = t64(y64).permute(0, 2, 1).reshape(N, C2, HW, 1).contiguous().requires_grad_(True)     # NCHW with W = 1
  O.batch_norm(ctx, yt, True, relu=True, layer_name='bn')            # creates gamma and beta
  names = list(vs.trainable)
  with torch.no_grad():
    vs.trainable[names[0]].copy_(t64(gamma))
    vs.trainable[names[1]].copy_(t64(beta))
  vs.begin_call()
  x = O.batch_norm(ctx, yt, True, relu=True, layer_name='bn')
  at = t64(d['att']).requires_grad_(True)
  f0, f1 = x[:, :Fh], x[:, Fh:]
  s = (f0 + f1).mean(dim=(2, 3))
  a = torch.softmax(torch.stack([at[:, :Fh], at[:, Fh:]], dim=0), dim=0)
  v = f0 * a[0][:, :, None, None] + f1 * a[1][:, :, None, None]
  dv_t = t64(d['dv']).permute(0, 2, 1).reshape(N, Fh, HW, 1)
  gy, gg, gb, ga = torch.autograd.grad([v, s], [yt, vs.trainable[names[0]], vs.trainable[names[1]], at],
                                       [dv_t, t64(d['ds'])])
  rows = lambda t: t.detach().reshape(N, -1, HW).permute(0, 2, 1).numpy()      # noqa: E731
  # 2^12 float64 ulps: xhat carries the cancellation of y - mean and the sums run over N HW terms
  assert np.array_equal(P.sk_fused_f(y64, scale, shift)[1], rows(x) > 0), 'mask'
  _close(fwd[0], s, k=4096, what='s')
  _close(fwd[1], rows(v), k=4096, what='V')
  _close(bwd['datt'], ga, k=4096 * HW, what='datt')
  _close(bwd['dbeta'], gb, k=4096 * N * HW, what='dbeta')
  _close(bwd['dgamma'], gg, k=4096 * N * HW, what='dgamma')
  _close(bwd['dy'], rows(gy), k=4096 * N * HW, what='dy')
  # the statistics are plain masked sums
  m = P.sk_fused_f(y64, scale, shift)[1]
  assert np.array_equal(fwd[2][:, 0], m.sum(axis=1)) and np.allclose(fwd[2][:, 1], (m * y64).sum(axis=1), rtol=0, atol=1e-12)
  dv2 = np.concatenate([d['dv'], d['dv']], axis=2).astype(np.float64)
  assert np.allclose(bwd['gstats'][:, 0], (m * dv2).sum(axis=1), rtol=0, atol=1e-12)
  assert np.allclose(bwd['gstats'][:, 1], (m * dv2 * y64).sum(axis=1), rtol=0, atol=1e-11)
  _floor('fused dy N=%d HW=%d F=%d' % (N, HW, Fh), lambda dt: P.sk_fused_bwd(
      d['y'], d['scale'], d['shift'], d['gamma'], d['mean'], d['invstd'], d['att'], d['dv'], d['ds'], dt)['dy'])


def test_fused_grid_inputs_hit_zero_exactly():
  """the grid inputs of the GPU module: t = y scale + shift is exact in float32, at least a fifth of it is exactly 0, and the
  mask leaves those elements out"""
  y, scale, shift, att = P.fused_grid_inputs(R.rng(61), 3, 29, 24)
  t32 = y * scale + shift
  t64 = y.astype(np.float64) * scale + shift
  assert np.array_equal(t32.astype(np.float64), t64)
  assert (t64 == 0).mean() >= 0.2
  f, m = P.sk_fused_f(y, scale, shift)
  assert not m[t64 == 0].any() and (f[t64 == 0] == 0).all() and m[t64 > 0].all()
  a0, a1 = P.sk_gates(att, 24)
  assert ((a0 < 1e-43) | (a0 == 0.5) | (a0 == 1.0)).all() and np.array_equal(a0 + a1, np.ones_like(a0))


def test_floors_of_the_fused_gpu_cases():
  """the floor of dy on the very inputs of every random fused case of the GPU module (same generator, same key)"""
  worst = 0.0
  for N, HW, Fh in P.FUSED_CASES:
    d = P.fused_random_inputs(R.rng(52, N, HW, Fh), N, HW, Fh)
    fl = _floor('fused dy N=%d HW=%d F=%d (GPU case)' % (N, HW, Fh), lambda dt: P.sk_fused_bwd(
        d['y'], d['scale'], d['shift'], d['gamma'], d['mean'], d['invstd'], d['att'], d['dv'], d['ds'], dt)['dy'])
    worst = max(worst, fl)
  assert worst < 2.0 ** -16, 'the bf16 ulp no longer dominates the bound of dy'
