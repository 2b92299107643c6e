"""asm_bn_bwd_apply_blocksum (csrc/bn.hip) -- the batch-norm backward apply of a BigLittle merge layer that also writes the
2x2 block sums of the masked gradient -- against the two launches it replaces, bit for bit:

  dx         ==  asm_bn_bwd_apply(relu = 2, no dz)
  block_sum  ==  asm_upsample2x_bwd_masked

Random inputs and random masks (the block sum's order, r then s, and its single rounding are the claim), plus the all-zero
and the all-ones mask.  Hs x Ws: 1x1 one quad per image; 3x5 odd, more columns than rows; 7x7 more than one workgroup at
C = 64.  C: 8 one vector column; 24 three columns, which do not divide the grid stride (the coefficients are reloaded per
trip); 64.  Inputs sit between NaN (mask: 0xFF) flanks, outputs between 0xA5 flanks (tests/gpu_guard.py).
"""
import numpy as np
import pytest
import torch

from tests.gpu_guard import BF, PATTERN, In, Out, _abi, _release_inputs, call  # noqa: F401

pytestmark = pytest.mark.gpu

F32 = torch.float32
U8 = torch.uint8
N = 2


def _bits(o):
  o.np()
  return o.t.detach().cpu().contiguous().view(torch.int16).numpy()


def _case(Hs, Ws, C, mask_kind, seed=23):
  r = np.random.default_rng(seed)
  H, W = 2 * Hs, 2 * Ws
  M = N * H * W
  dy = In(r.standard_normal((M, C)).astype(np.float32))
  x = In(r.standard_normal((M, C)).astype(np.float32))
  bits = {'random': r.integers(0, 256, (M, C // 8)), 'zeros': np.zeros((M, C // 8)), 'ones': np.full((M, C // 8), 255)}[mask_kind]
  mask = In(bits.astype(np.uint8), U8, 0xFF)
  co = [In(v.astype(np.float32), F32) for v in (r.uniform(0.5, 1.5, C), 0.1 * r.standard_normal(C), 0.1 * r.standard_normal(C))]
  dx = [Out((M, C), BF) for _ in range(2)]
  bs = [Out((N, Hs, Ws, C), BF) for _ in range(2)]
  call('asm_upsample2x_bwd_masked', dy.p, mask.p, bs[0].p, N, Hs, Ws, C)
  call('asm_bn_bwd_apply', dy.p, x.p, mask.p, 2, M, C, co[0].p, co[1].p, co[2].p, dx[0].p, None)
  call('asm_bn_bwd_apply_blocksum', dy.p, x.p, mask.p, N, H, W, C, co[0].p, co[1].p, co[2].p, dx[1].p, bs[1].p)
  for what, (chain, fused) in (('dx', dx), ('block sum', bs)):
    a, b = _bits(fused), _bits(chain)
    assert np.array_equal(a, b), '%s: %d of %d elements differ' % (what, int((a != b).sum()), a.size)
  return bs[1]


@pytest.mark.parametrize('C', [8, 24, 64])
@pytest.mark.parametrize('Hs,Ws', [(1, 1), (3, 5), (7, 7)])
def test_equals_block_sum_then_apply(hip_lib, Hs, Ws, C):
  bs = _case(Hs, Ws, C, 'random')
  assert float(bs.t.float().abs().sum()) > 0


def test_all_zero_mask(hip_lib):
  bs = _case(3, 5, 24, 'zeros')
  assert not bool(bs.t.view(torch.int16).any()), 'a fully masked gradient has +0 block sums'


def test_all_ones_mask(hip_lib):
  _case(3, 5, 24, 'ones')


def test_refusals_launch_nothing(hip_lib):
  """odd H, odd W, C % 8 != 0 and null pointers: ASM_EINVAL, no launch, no output written"""
  L = _abi().L()
  C = 8
  a = In(np.ones((N * 4 * 4, C), np.float32))
  m = In(np.zeros((N * 4 * 4, 1), np.uint8), U8, 0xFF)
  f = In(np.ones(C, np.float32), F32)
  dx, bs = Out((N * 4 * 4, C), BF), Out((N, 2, 2, C), BF)
  n0 = L.asm_launch_count()
  for Hb, Wb, Cb in ((3, 4, C), (4, 3, C), (4, 4, 12), (0, 4, C)):
    with pytest.raises(ValueError):
      call('asm_bn_bwd_apply_blocksum', a.p, a.p, m.p, N, Hb, Wb, Cb, f.p, f.p, f.p, dx.p, bs.p)
  for args in ((None, a.p, m.p, dx.p, bs.p), (a.p, a.p, None, dx.p, bs.p), (a.p, a.p, m.p, None, bs.p), (a.p, a.p, m.p, dx.p, None)):
    with pytest.raises(ValueError):
      call('asm_bn_bwd_apply_blocksum', args[0], args[1], args[2], N, 4, 4, C, f.p, f.p, f.p, args[3], args[4])
  assert L.asm_launch_count() == n0, 'a refused call launched a kernel'
  for o in (dx, bs):
    o.check_flanks()
    assert bool((o.t.view(U8) == PATTERN).all()), 'a refused call wrote an output'
