"""The strided selective-kernel unit's folded blur pool (csrc/sk_fused.hip) against the chains it replaces, bit for bit:

  asm_sk_select_bn_blur_fwd            ==  asm_sk_select_bn_fwd -> asm_blurpool_fwd
  asm_sk_select_bn_bwd_att_stats_blur  ==  asm_blurpool_bwd -> asm_sk_select_bn_bwd_att_stats   (datt, both statistics rows)
  asm_sk_bn_bwd_apply_blur             ==  asm_blurpool_bwd -> asm_sk_bn_bwd_apply              (dy)

Random inputs: the claim is that every sum keeps its terms, their order and its rounding points, which an input on a grid of
exactly representable sums would not notice.  Shapes, the smallest at which each path can go wrong: 2x2 one output pixel,
both REFLECT terms and no i + 1 neighbour (the chain's blur backward is the GENERIC kernel there: the order claim is
checked against it too); 4x6 and 6x10 more columns than rows, and 6 = one band of the forward kernel (two output rows, four
input rows) plus two rows, i.e. a last band of one output row; 24x24 HW >= 512, the 1024-thread per-image form of the
gate-gradient pass.  F: 8 one vector column, 24 a column count that does not divide 256 (idle threads), 64.
Inputs sit between NaN flanks and outputs between 0xA5 flanks (tests/gpu_guard.py).
"""
import numpy as np
import pytest
import torch

from tests.gpu_guard import BF, PATTERN, In, Out, _abi, _release_inputs, call  # noqa: F401

pytestmark = pytest.mark.gpu

F32 = torch.float32
N = 3
SHAPES = [(2, 2), (4, 6), (6, 10), (24, 24)]
CHANNELS = [8, 24, 64]


def _inputs(H, W, F_, seed):
  r = np.random.default_rng(seed)
  C2 = 2 * F_
  return dict(
      y=In(r.standard_normal((N, H, W, C2)).astype(np.float32)),
      scale=In(r.uniform(0.5, 1.5, C2).astype(np.float32), F32),
      shift=In((0.5 * r.standard_normal(C2)).astype(np.float32), F32),
      mean=In(r.standard_normal(C2).astype(np.float32), F32),
      invstd=In(r.uniform(0.5, 2.0, C2).astype(np.float32), F32),
      att=In(r.standard_normal((N, C2)).astype(np.float32), F32),
      dpool=In(r.standard_normal((N, H // 2, W // 2, F_)).astype(np.float32)),
      ds=In(r.standard_normal((N, F_)).astype(np.float32)),
      cA=In(r.uniform(0.5, 1.5, C2).astype(np.float32), F32),
      cB=In((0.1 * r.standard_normal(C2)).astype(np.float32), F32),
      cC=In((0.1 * r.standard_normal(C2)).astype(np.float32), F32))


def _bits(o):
  o.np()                                            # flanks intact, no NaN / huge value (a read outside an input)
  t = o.t.detach().cpu().contiguous()
  return t.view(torch.int16 if t.dtype == BF else torch.int32).numpy()


def _same(what, fused, chain):
  a, b = _bits(fused), _bits(chain)
  assert a.shape == b.shape and np.array_equal(a, b), '%s: %d of %d elements differ' % (what, int((a != b).sum()), a.size)
  assert not bool((fused.t.view(torch.uint8) == PATTERN).all()), '%s: nothing was written' % what


@pytest.mark.parametrize('F_', CHANNELS)
@pytest.mark.parametrize('H,W', SHAPES)
def test_forward_equals_select_then_blur(hip_lib, H, W, F_):
  i = _inputs(H, W, F_, 11)
  v, chain, fused = Out((N, H, W, F_), BF), Out((N, H // 2, W // 2, F_), BF), Out((N, H // 2, W // 2, F_), BF)
  call('asm_sk_select_bn_fwd', i['y'].p, i['scale'].p, i['shift'].p, i['att'].p, v.p, N, H * W, F_)
  call('asm_blurpool_fwd', v.p, chain.p, N, H, W, F_, 3, 2)
  call('asm_sk_select_bn_blur_fwd', i['y'].p, i['scale'].p, i['shift'].p, i['att'].p, fused.p, N, H, W, F_, 3, 2)
  _same('blurred V', fused, chain)


@pytest.mark.parametrize('F_', CHANNELS)
@pytest.mark.parametrize('H,W', SHAPES)
def test_backward_equals_blur_backward_then_the_dv_passes(hip_lib, H, W, F_):
  i = _inputs(H, W, F_, 13)
  C2 = 2 * F_
  dv = Out((N, H, W, F_), BF)
  call('asm_blurpool_bwd', i['dpool'].p, dv.p, N, H, W, F_, 3, 2)
  datt = [Out((N, C2), BF) for _ in range(2)]
  gst = [Out((N, 2, C2), F32) for _ in range(2)]
  dy = [Out((N, H, W, C2), BF) for _ in range(2)]
  call('asm_sk_select_bn_bwd_att_stats', i['y'].p, i['scale'].p, i['shift'].p, i['mean'].p, i['invstd'].p, dv.p, i['att'].p,
       datt[0].p, gst[0].p, N, H * W, F_)
  call('asm_sk_select_bn_bwd_att_stats_blur', i['y'].p, i['scale'].p, i['shift'].p, i['mean'].p, i['invstd'].p, i['dpool'].p,
       i['att'].p, datt[1].p, gst[1].p, N, H, W, F_, 3, 2)
  _same('datt', datt[1], datt[0])
  _same('gradient statistics (both rows)', gst[1], gst[0])
  call('asm_sk_bn_bwd_apply', dv.p, i['att'].p, i['ds'].p, i['y'].p, i['scale'].p, i['shift'].p, i['cA'].p, i['cB'].p,
       i['cC'].p, dy[0].p, N, H * W, F_)
  call('asm_sk_bn_bwd_apply_blur', i['dpool'].p, i['att'].p, i['ds'].p, i['y'].p, i['scale'].p, i['shift'].p, i['cA'].p,
       i['cB'].p, i['cC'].p, dy[1].p, N, H, W, F_, 3, 2)
  _same('dy', dy[1], dy[0])


def test_refusals_launch_nothing(hip_lib):
  """odd H or W, a filter size other than 3, a stride other than 2 and null pointers: the library's error, no launch, no
  output written"""
  L = _abi().L()
  H, W, F_ = 4, 4, 8
  i = _inputs(H, W, F_, 17)
  C2 = 2 * F_
  out, datt, gst, dy = Out((N, H, W, F_), BF), Out((N, C2), BF), Out((N, 2, C2), F32), Out((N, H, W, C2), BF)

  def fwd(h=H, w=W, k=3, s=2, y=i['y'].p, o=None):
    call('asm_sk_select_bn_blur_fwd', y, i['scale'].p, i['shift'].p, i['att'].p, out.p if o is None else o, N, h, w, F_, k, s)

  def att(h=H, w=W, k=3, s=2, g=i['dpool'].p, st=None):
    call('asm_sk_select_bn_bwd_att_stats_blur', i['y'].p, i['scale'].p, i['shift'].p, i['mean'].p, i['invstd'].p, g,
         i['att'].p, datt.p, gst.p if st is None else st, N, h, w, F_, k, s)

  def app(h=H, w=W, k=3, s=2, g=i['dpool'].p, o=None):
    call('asm_sk_bn_bwd_apply_blur', g, i['att'].p, i['ds'].p, i['y'].p, i['scale'].p, i['shift'].p, i['cA'].p, i['cB'].p,
         i['cC'].p, dy.p if o is None else o, N, h, w, F_, k, s)

  n0 = L.asm_launch_count()
  for fn in (fwd, att, app):
    for kw in (dict(h=3), dict(w=3), dict(k=5), dict(k=2), dict(s=1), dict(s=3)):
      with pytest.raises(ValueError):
        fn(**kw)
  for fn, kw in ((fwd, dict(y=0)), (fwd, dict(o=0)), (att, dict(g=0)), (att, dict(st=0)), (app, dict(g=0)), (app, dict(o=0))):
    with pytest.raises(ValueError):
      fn(**kw)                                    # 0: a null pointer
  assert L.asm_launch_count() == n0, 'a refused call launched a kernel'
  for o in (out, datt, gst, dy):
    o.check_flanks()
    assert bool((o.t.view(torch.uint8) == PATTERN).all()), 'a refused call wrote an output'
