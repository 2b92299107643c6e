"""Host logic of the two folded resampling steps, on the CPU double (no GPU):

  * a strided selective-kernel bottleneck -- conv1 -> SK unit -> blur pool (3 taps, stride 2) -> conv3 -- whose V is left to
    nn.blur_pool, which runs select + blur as one call and hands the pooled gradient back to the unit's backward passes;
  * a BigLittle merge -- conv -> BN (+ upsampled big branch) -> ReLU -- whose backward apply also writes the 2x2 block sums.

The double of tests/cpu_double.py does not have the new entry points; the subclass below adds them by COMPOSING the
double's own methods (select -> blur pool, blur-pool backward -> gate gradient / apply, block sum + apply), so a fused host
path that wires a tensor, a shape or an order wrongly cannot give the bits of the un-fused one.
"""
import pytest
import torch

from tests.cpu_double import CpuDouble

N, H, W, CIN, F_ = 2, 8, 8, 16, 16
NEW = ('asm_sk_select_bn_blur_fwd', 'asm_sk_select_bn_bwd_att_stats_blur', 'asm_sk_bn_bwd_apply_blur',
       'asm_bn_bwd_apply_blocksum')


class FoldedDouble(CpuDouble):
  def __init__(self):
    super().__init__()
    self.calls = dict.fromkeys(NEW, 0)

  @staticmethod
  def _tmp(*shape):
    return torch.empty(shape, dtype=torch.bfloat16)

  def asm_sk_select_bn_blur_fwd(self, y, scale, shift, att, out, N, H, W, F, k, stride, stream):
    self.calls['asm_sk_select_bn_blur_fwd'] += 1
    v = self._tmp(N, H, W, F)
    rc = self.asm_sk_select_bn_fwd(y, scale, shift, att, v.data_ptr(), N, H * W, F, stream)
    return rc or self.asm_blurpool_fwd(v.data_ptr(), out, N, H, W, F, k, stride, stream)

  def asm_sk_select_bn_bwd_att_stats_blur(self, y, scale, shift, mean, invstd, dpool, att, datt, gst, N, H, W, F, k, stride,
                                          stream):
    self.calls['asm_sk_select_bn_bwd_att_stats_blur'] += 1
    dv = self._tmp(N, H, W, F)
    rc = self.asm_blurpool_bwd(dpool, dv.data_ptr(), N, H, W, F, k, stride, stream)
    return rc or self.asm_sk_select_bn_bwd_att_stats(y, scale, shift, mean, invstd, dv.data_ptr(), att, datt, gst, N, H * W, F,
                                                     stream)

  def asm_sk_bn_bwd_apply_blur(self, dpool, att, ds, y, scale, shift, cA, cB, cC, dy, N, H, W, F, k, stride, stream):
    self.calls['asm_sk_bn_bwd_apply_blur'] += 1
    dv = self._tmp(N, H, W, F)
    rc = self.asm_blurpool_bwd(dpool, dv.data_ptr(), N, H, W, F, k, stride, stream)
    return rc or self.asm_sk_bn_bwd_apply(dv.data_ptr(), att, ds, y, scale, shift, cA, cB, cC, dy, N, H * W, F, stream)

  def asm_bn_bwd_apply_blocksum(self, dy, x, mask, N, H, W, Cn, cA, cB, cC, dx, bsum, stream):
    self.calls['asm_bn_bwd_apply_blocksum'] += 1
    rc = self.asm_upsample2x_bwd_masked(dy, mask, bsum, N, H // 2, W // 2, Cn, stream)
    return rc or self.asm_bn_bwd_apply(dy, x, mask, 2, N * H * W, Cn, cA, cB, cC, dx, 0, stream)


def _walk(nn, ctx, x):
  """one strided SK bottleneck (its main branch) feeding, as the big branch, one BigLittle merge"""
  L = ctx.layer
  c1, b1 = L(lambda: nn.ConvKernel(ctx, 1, CIN, F_)), L(lambda: nn.BatchNorm(ctx, F_))
  h = nn.conv_bn(ctx, x, c1, b1, 1, relu=True)
  h = L(lambda: nn.SKUnit(ctx, F_, F_))(ctx, h, 1)
  h = nn.blur_pool(ctx, h, 3, 2)
  c3, b3 = L(lambda: nn.ConvKernel(ctx, 1, F_, 32)), L(lambda: nn.BatchNorm(ctx, 32))
  big = nn.conv_bn(ctx, h, c3, b3, 1, relu=False)                                    # [N, H/2, W/2, 32]
  cl, bl = L(lambda: nn.ConvKernel(ctx, 1, CIN, 32)), L(lambda: nn.BatchNorm(ctx, 32))
  merged = nn.conv_bn(ctx, x, cl, bl, 1, relu=True, residual=big, res_mode=2)        # the merge, at full resolution
  c4, b4 = L(lambda: nn.ConvKernel(ctx, 1, 32, 16)), L(lambda: nn.BatchNorm(ctx, 16))
  return nn.conv_bn(ctx, merged, c4, b4, 1, relu=False)


def _run(provider, monkeypatch, **env):
  from assembled_cnn_amd import nn, ops
  for k in ('ASM_SK_BLUR', 'ASM_BL_SUM'):
    monkeypatch.delenv(k, raising=False)
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  ops.set_library(provider, is_double=True)
  ops.refresh_tuning()
  try:
    arena, layers = nn.ParamArena(), []
    _walk(nn, nn.Ctx(arena, True, True, 0.9, 'cpu', False, layers), nn.Var(None, (N, H, W, CIN)))
    arena.finalize('cpu', 3)
    g = torch.Generator().manual_seed(5)
    x = nn.Var(torch.randn((N, H, W, CIN), generator=g).to(torch.bfloat16))
    ctx = nn.Ctx(arena, True, False, 0.9, 'cpu', True, layers)
    out = _walk(nn, ctx, x)
    out.set_grad(torch.randn(out.shape, generator=g).to(torch.bfloat16), False)
    ctx.backward()
    return dict(out=out.data.clone(), dx=x.grad.clone(), grads=arena.g32.clone(), state=arena.state.clone())
  finally:
    for k in env:
      monkeypatch.delenv(k, raising=False)
    ops.refresh_tuning()              # (on a double: forgets the cached knobs, nothing else)
    ops.set_library(None, is_double=False)


def _same(a, b):
  for k in a:
    assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
    assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), '%s differs' % k


def test_folded_host_path_is_bit_identical_to_the_chain(monkeypatch):
  fused_lib, plain_lib = FoldedDouble(), FoldedDouble()
  fused = _run(fused_lib, monkeypatch)
  plain = _run(plain_lib, monkeypatch, ASM_SK_BLUR='0', ASM_BL_SUM='0')
  assert all(fused_lib.calls[k] == 1 for k in NEW), fused_lib.calls          # one strided unit, one merge: one call each
  assert not any(plain_lib.calls.values()), plain_lib.calls
  assert float(fused['grads'].abs().sum()) > 0 and float(fused['dx'].float().abs().sum()) > 0
  _same(fused, plain)


@pytest.mark.parametrize('knob', ['ASM_SK_BLUR', 'ASM_BL_SUM'])
def test_each_knob_switches_its_own_part(monkeypatch, knob):
  lib = FoldedDouble()
  _run(lib, monkeypatch, **{knob: '0'})
  sk = sum(lib.calls[k] for k in NEW[:3])
  assert (sk, lib.calls[NEW[3]]) == ((0, 1) if knob == 'ASM_SK_BLUR' else (3, 0)), lib.calls


def test_provider_without_the_entry_points_keeps_the_chain(monkeypatch):
  """the plain double: the un-fused path runs (nothing to call), with the same result"""
  assert not any(hasattr(CpuDouble, k) for k in NEW)
  ref = _run(FoldedDouble(), monkeypatch, ASM_SK_BLUR='0', ASM_BL_SUM='0')
  _same(_run(CpuDouble(), monkeypatch), ref)
