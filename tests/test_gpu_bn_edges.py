"""Edge shapes, known answers and guard bands of the batch-norm kernels (csrc/bn.hip: the row reducers behind row_reduce, the
apply passes behind for_each_vec, bn_small) against the plain float64 references of tests/bn_ref.py, which
tests/test_bn_ref_cpu.py proves against the oracle on the CPU.

Rules of every case (those of tests/test_gpu_rows_edges.py):
* element-wise bounds, never a norm.  Inputs on integer grids have exactly representable sums and results: equal bits.
  bf16 outputs of random data: |out - ref| <= 2^-8 |ref| + 4 * floor, floor = rows_ref.floor_of of that case (the float64
  reference against its own float32 evaluation).  float32 sums of n terms: n 2^-24 sum |terms|.  What a kernel rounds once
  from float64: the float32 next to the reference, 1 ulp.
* every output sits between two 4 KiB flanks of the byte 0xA5 and starts as 0xA5 itself; every tensor input sits between two
  flanks of NaN (0xFF for mask bytes), so a read outside the tensor reaches an output, where Out.np() rejects it.
* ``-s`` prints the worst error of every case next to its bound (profiles/bn_edges_tolerances.md records the worst of each
  kernel family).

The tiling table: C -> what make_tiling gives it (rpb = 256 / vcb row lanes; a row tile is 2 rpb rows):
  8 rpb 256 | 24 rpb 85, 1 idle thread | 64 | 72 rpb 28, 4 idle threads | 128 2 slices | 136 2 slices of 9 and 8 columns |
  520 8 slices of 9, the last holds 2 | 1008 8 slices of 16, the last holds 14 | 2048 | 16448 vc_slice 257 > 256: two column
  groups, rpb 1 (M 1 and 9 only).
"""
import numpy as np
import pytest
import torch

from tests import bn_ref as B
from tests import rows_ref as R
from tests import util
from tests.gpu_guard import (BF, PATTERN, In, Out, _abi, _release_inputs, call, close_bf16, close_sum,  # noqa: F401
                             close_terms, close_ulp, exact)

pytestmark = pytest.mark.gpu

F32 = torch.float32
U8 = torch.uint8
EPS, MOM = 1e-5, 0.9
UNWRITTEN = np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0]      # a float32 output element nobody stored


def tiling(M, C, bn_rows):
  """make_tiling of csrc/bn.hip: (blocks, slices, vc_slice, rpb)"""
  sl = max(1, min(8, C // 64))
  vc_slice = -(-(C // 8) // sl)
  rpb = 256 // min(vc_slice, 256)
  rows = max(-(-(-(-M // max(bn_rows // sl, 1))) // rpb) * rpb, 4 * rpb)
  return -(-M // rows), sl, vc_slice, rpb


def _rows_of(C):
  rpb = tiling(1, C, 1024)[3]
  return [1, 9] if C == 16448 else sorted({1, 2 * rpb - 1, 2 * rpb, 2 * rpb + 1, 4099})


TABLE = (8, 24, 64, 72, 128, 136, 520, 1008, 2048, 16448)
REDUCE_CASES = [(C, M) for C in TABLE for M in _rows_of(C)]
APPLY_CASES = [(C, M) for C in (8, 72, 520, 2048) for M in _rows_of(C)]
KNOBS = (1, 1024)


def test_the_tiling_table_is_what_the_docstring_says():
  """the states the sweep is there for, from the Python copy of make_tiling that every reducer case checks against
  asm_bn_stats_blocks: idle threads, short last slices, a second column group"""
  t = {C: tiling(4099, C, 1024) for C in TABLE}
  assert [t[C][3] for C in (8, 24, 72, 136, 520)] == [256, 85, 28, 28, 28] and 256 - 85 * 3 == 1 and 256 - 28 * 9 == 4
  assert t[128][1] == 2 and t[136][1:3] == (2, 9) and 17 - 9 == 8
  assert t[520][1:3] == (8, 9) and 65 - 7 * 9 == 2 and t[1008][1:3] == (8, 16) and 126 - 7 * 16 == 14
  assert t[16448][2] == 257 and t[16448][3] == 1
  assert tiling(4099, 2048, 1024)[0] == 103 and tiling(9, 16448, 1024)[0] == 3


def grid(r, shape, lo, hi):
  return r.integers(lo, hi + 1, shape).astype(np.float32)


def quarters(r, shape, most=8):
  """multiples of 0.25 in [-most / 4, most / 4]"""
  return (r.integers(-most, most + 1, shape) * 0.25).astype(np.float32)


def _summed(out):
  """[blocks][2][C] partials, every element written, summed over the blocks in float64"""
  assert not bool((out.t.view(torch.int32) == int(UNWRITTEN)).any()), 'a partial element was never written'
  return out.np().sum(axis=0)


def _blocks(monkeypatch, knob, M, C):
  util.set_knob(monkeypatch, 'ASM_BN_ROWS', knob)
  blocks = _abi().L().asm_bn_stats_blocks(M, C)
  want, _, _, rpb = tiling(M, C, knob)
  assert blocks == want, 'asm_bn_stats_blocks(%d, %d) = %d, make_tiling predicts %d' % (M, C, blocks, want)
  if knob == 1:
    assert blocks == 1                       # one block walks every row tile
  elif M > 4 * rpb:
    assert blocks > 1                        # many blocks
  return blocks


# ---- reducers ----------------------------------------------------------------------------------------------------------
def _reducer_inputs(C, M, kind):
  r = R.rng(301, C, M, kind == 'grid')
  d = {}
  if kind == 'grid':
    d['x'], d['xb'], d['dy'] = grid(r, (M, C), -4, 4), grid(r, (M, C), -4, 4), grid(r, (M, C), -2, 2)
    for k in ('mean', 'mean_b'):
      d[k] = r.choice([-1.0, 0.0, 1.0], C).astype(np.float32)
    for k in ('invstd', 'invstd_b'):
      d[k] = r.choice([0.5, 1.0, 2.0], C).astype(np.float32)
    d['yout'] = r.choice(np.array([-1.5, -0.0, 0.0, 1.0, 2.0], np.float32), (M, C))
  else:
    # bf16 data; means on a grid of 1/16 and power-of-two invstd: (x - mean) invstd is then exact in float32 and every term
    # carries ONE rounding, so a sum of n terms is within n half-ulps of sum |terms| whatever its order -- for n = 1 too
    d['x'], d['xb'], d['dy'] = R.bf16_randn(r, (M, C)), R.bf16_randn(r, (M, C), 2.0), R.bf16_randn(r, (M, C))
    for k in ('mean', 'mean_b'):
      d[k] = (r.integers(-16, 17, C) / 16.0).astype(np.float32)
    for k in ('invstd', 'invstd_b'):
      d[k] = r.choice([0.5, 1.0, 2.0, 4.0], C).astype(np.float32)
    d['yout'] = R.bf16_randn(r, (M, C))
    d['yout'].reshape(-1)[::5] = 0.0
    d['yout'].reshape(-1)[1::7] = -0.0
  d['mask'] = r.integers(0, 256, (M, C // 8), dtype=np.uint8)
  return d


def _sums_and_magnitudes(dy, x, gate, mean, invstd):
  dz = B.gated(dy, gate)
  xhat = (x.astype(np.float64) - mean) * invstd
  return np.stack(B.bwd_sums(dy, x, gate, mean, invstd)), np.stack([np.abs(dz).sum(0), np.abs(dz * xhat).sum(0)])


@pytest.mark.parametrize('C,M', REDUCE_CASES)
def test_reducers_known_answer_and_random(hip_lib, monkeypatch, C, M):
  """asm_bn_stats, asm_bn_bwd_reduce (mask kinds 0, 1, 2) and asm_bn_bwd_reduce2 over the tiling table, one block of many
  trips (ASM_BN_ROWS = 1) and many blocks (1024).  Integer grids: every product and every partial sum in any order is an
  exact float32 (asserted on the reference: sum |terms| < 2^24 halves), so the partials summed in float64 ARE the float64
  reference.  Random bf16 data: n 2^-24 sum |terms| per channel."""
  for kind in ('grid', 'random'):
    d = _reducer_inputs(C, M, kind)
    ref, mag = {}, {}
    x64 = d['x'].astype(np.float64)
    ref['stats'], mag['stats'] = np.stack(B.stats(d['x'])), np.stack([np.abs(x64).sum(0), (x64 * x64).sum(0)])
    gates = {0: None, 1: B.gate_of(1, d['yout'], C), 2: B.gate_of(2, d['mask'], C)}
    assert not gates[1][d['yout'] == 0].any()        # zeros of either sign gate off
    for k in (0, 1, 2):
      ref[k], mag[k] = _sums_and_magnitudes(d['dy'], d['x'], gates[k], d['mean'], d['invstd'])
    ref['a'], mag['a'] = ref[2], mag[2]
    ref['b'], mag['b'] = _sums_and_magnitudes(d['dy'], d['xb'], gates[2], d['mean_b'], d['invstd_b'])
    if kind == 'grid':
      for k in mag:
        assert mag[k].max() * 2 < 2 ** 24, 'the grid no longer keeps every partial sum exact'
    t = {k: In(d[k]) for k in ('x', 'xb', 'dy', 'yout')}
    t.update({k: In(d[k], F32) for k in ('mean', 'mean_b', 'invstd', 'invstd_b')})
    t['mask'] = In(d['mask'], U8, 0xFF)

    def judge(case, got, key):
      if kind == 'grid':
        exact(case, got, ref[key])
      else:
        close_sum(case, got, ref[key], M, mag[key])

    for knob in KNOBS:
      blocks = _blocks(monkeypatch, knob, M, C)
      case = '%s C=%d M=%d rows=%d ' % (kind, C, M, knob)
      p = Out((blocks, 2, C), F32)
      call('asm_bn_stats', t['x'].p, M, C, p.p)
      judge(case + 'stats', _summed(p), 'stats')
      for k in (0, 1, 2):
        p = Out((blocks, 2, C), F32)
        yout = None if k == 0 else t['yout'].p if k == 1 else t['mask'].p
        call('asm_bn_bwd_reduce', t['dy'].p, t['x'].p, yout, k, M, C, t['mean'].p, t['invstd'].p, p.p)
        judge(case + 'bwd_reduce kind %d' % k, _summed(p), k)
      pa, pb = Out((blocks, 2, C), F32), Out((blocks, 2, C), F32)
      call('asm_bn_bwd_reduce2', t['dy'].p, t['x'].p, t['xb'].p, t['mask'].p, M, C, t['mean'].p, t['invstd'].p, t['mean_b'].p,
           t['invstd_b'].p, pa.p, pb.p)
      sa, sb = _summed(pa), _summed(pb)
      judge(case + 'bwd_reduce2 a', sa, 'a')
      judge(case + 'bwd_reduce2 b', sb, 'b')
      exact(case + 'bwd_reduce2: row 0 of both partials holds sum g', pa.np()[:, 0], pb.np()[:, 0])
    _release_now()


def _release_now():
  from tests import gpu_guard
  del gpu_guard._ALIVE[:]


# ---- apply passes --------------------------------------------------------------------------------------------------------
POW2 = np.array([-1.0, 0.5, 1.0, 2.0], np.float32)
RES_GRID = np.array([-2, -1, -0.5, -0.25, 0, 0, 0, 0.25, 0.5, 1, 2], np.float32)


def _fwd_inputs(C, M, Mres, kind, seed):
  r = R.rng(302, C, M, seed, kind == 'grid')
  if kind == 'grid':
    x, xb = grid(r, (M, C), -4, 4), grid(r, (M, C), -4, 4)
    sc, sc_b = r.choice(POW2, C), r.choice(POW2, C)
    # most shifts cancel an integer x exactly (pre-activations of exactly 0), the rest are any multiple of 0.25; row 0 of the
    # cancelling channels is planted on that integer with a zero residual, so the smallest tensors hold exact zeros too
    cancel = r.random(C) < 0.7
    cancel[0] = True
    k, kb = grid(r, C, -2, 2), grid(r, C, -2, 2)
    sh = np.where(cancel, -sc * k, quarters(r, C)).astype(np.float32)
    sh_b = np.where(cancel, -sc_b * kb, quarters(r, C)).astype(np.float32)
    res = r.choice(RES_GRID, (Mres, C))
    x[0, cancel], xb[0, cancel], res[0, cancel] = k[cancel], kb[cancel], 0.0
  else:
    x, xb = R.bf16_randn(r, (M, C)), R.bf16_randn(r, (M, C), 2.0)
    sc, sc_b = (r.uniform(0.5, 2.0, C) * r.choice([-1, 1], C)).astype(np.float32), r.uniform(0.25, 1.0, C).astype(np.float32)
    sh, sh_b = r.standard_normal(C).astype(np.float32), r.standard_normal(C).astype(np.float32)
    res = R.bf16_randn(r, (Mres, C))
  return x, xb, sc, sh, sc_b, sh_b, res


def _judge_fwd(case, kind, relu, y, mask, ref_y, ref_bits, ref_pre, floor, C):
  got = y.np()
  if kind == 'grid':
    exact(case, got, R.to_bf16(ref_y).astype(np.float64))
    zero = ref_pre == 0
    assert zero.mean() >= 0.01, case + ': the grid gives too few pre-activations of exactly 0'
    if relu:
      assert (got[zero] == 0).all()
    if mask is not None:
      assert not ref_bits[zero].any()
      exact(case + ' mask', mask.np(), B.pack_mask(ref_bits))
  else:
    close_bf16(case, got, ref_y, floor)
    if mask is not None:
      exact(case + ' mask == (own output > 0)', mask.np(), B.pack_mask(got > 0))


def _apply_all_forms(C, M, geometry, kinds=('grid', 'random')):
  """asm_bn_apply: res_mode (0, 1 and -- with a geometry -- 2) x relu x with / without the mask"""
  N, H, W = geometry or (0, 0, 0)
  for kind in kinds:
    x, _, sc, sh, _, _, res = _fwd_inputs(C, M, M // 4 if geometry else M, kind, 1)
    xt, sct, sht, rt = In(x), In(sc, F32), In(sh, F32), In(res)
    for res_mode in ((2,) if geometry else (0, 1)):
      args = (res if res_mode else None, res_mode)
      for relu in (False, True):
        ref_y, ref_bits, ref_pre = B.apply(x, sc, sh, *args, relu, H, W)
        floor = 0.0 if kind == 'grid' else R.floor_of(lambda dt: B.apply(x, sc, sh, *args, relu, H, W, dt)[0])
        for with_mask in (False, True):
          case = 'bn_apply %s C=%d M=%d res %d relu %d mask %d' % (kind, C, M, res_mode, relu, with_mask)
          y, mask = Out((M, C), BF), Out((M, C // 8), U8) if with_mask else None
          call('asm_bn_apply', xt.p, y.p, M, C, sct.p, sht.p, rt.p if res_mode else None, res_mode, int(relu), H, W,
               mask.p if mask else None)
          if relu:
            _judge_fwd(case, kind, relu, y, mask, ref_y, ref_bits, ref_pre, floor, C)
          else:
            _judge_fwd(case, kind, relu, y, None, ref_y, ref_bits, ref_pre, floor, C)
            if mask is not None:
              assert (mask.np() == PATTERN).all(), case + ': no ReLU, no mask'
    _release_now()


@pytest.mark.parametrize('C,M', APPLY_CASES)
def test_apply_forms(hip_lib, C, M):
  """the grid-stride skeleton at one vector, ragged tiles and (4099 x 2048) a second trip; coefficient rows kept across trips
  (C / 8 divides the stride) and re-loaded (C = 72, 520)"""
  _apply_all_forms(C, M, None)


@pytest.mark.parametrize('N,H,W', [(1, 2, 2), (3, 2, 6), (2, 4, 2)])
@pytest.mark.parametrize('C', [8, 72, 520, 2048])
def test_apply_upsampled_residual(hip_lib, C, N, H, W):
  """res_mode 2: the residual of pixel (n, h, w) is the low-resolution pixel (n, h / 2, w / 2)"""
  _apply_all_forms(C, N * H * W, (N, H, W))


@pytest.mark.parametrize('C,M', APPLY_CASES)
def test_apply2_forms(hip_lib, C, M):
  """out = [relu](bn_a(xa) + bf16(bn_b(xb)))"""
  for kind in ('grid', 'random'):
    xa, xb, sa, ha, sb, hb, _ = _fwd_inputs(C, M, 1, kind, 2)
    t = [In(xa), In(xb)] + [In(v, F32) for v in (sa, ha, sb, hb)]
    for relu in (False, True):
      ref_y, ref_bits = B.apply_dual(xa, xb, sa, ha, sb, hb, relu)
      ref_pre = B.apply_dual(xa, xb, sa, ha, sb, hb, False)[0]
      floor = 0.0 if kind == 'grid' else R.floor_of(lambda dt: B.apply_dual(xa, xb, sa, ha, sb, hb, relu, dt)[0])
      for with_mask in (False, True):
        case = 'bn_apply2 %s C=%d M=%d relu %d mask %d' % (kind, C, M, relu, with_mask)
        y, mask = Out((M, C), BF), Out((M, C // 8), U8) if with_mask else None
        call('asm_bn_apply2', t[0].p, t[1].p, y.p, M, C, t[2].p, t[3].p, t[4].p, t[5].p, int(relu), mask.p if mask else None)
        _judge_fwd(case, kind, relu, y, mask if relu else None, ref_y, ref_bits, ref_pre, floor, C)
        if mask is not None and not relu:
          assert (mask.np() == PATTERN).all(), case + ': no ReLU, no mask'
    _release_now()


def _bwd_inputs(C, M, kind):
  r = R.rng(303, C, M, kind == 'grid')
  if kind == 'grid':
    dy, x, xb = grid(r, (M, C), -2, 2), grid(r, (M, C), -4, 4), grid(r, (M, C), -4, 4)
    co = np.stack([r.choice(POW2, C), r.choice(POW2, C), quarters(r, C), r.choice(POW2, C), r.choice(POW2, C), quarters(r, C)])
    yout = r.choice(np.array([-1.5, -0.0, 0.0, 1.0, 2.0], np.float32), (M, C))
  else:
    dy, x, xb = R.bf16_randn(r, (M, C)), R.bf16_randn(r, (M, C)), R.bf16_randn(r, (M, C), 2.0)
    co = r.standard_normal((6, C)).astype(np.float32)
    yout = R.bf16_randn(r, (M, C))
    yout.reshape(-1)[::5] = 0.0
    yout.reshape(-1)[1::7] = -0.0
  return dy, x, xb, co.astype(np.float32), yout, r.integers(0, 256, (M, C // 8), dtype=np.uint8)


def _judge_dx(case, kind, out, dz, x, A, Bc, Cc):
  ref = B.bwd_dx(dz, x, A, Bc, Cc)
  if kind == 'grid':
    exact(case, out.np(), R.to_bf16(ref).astype(np.float64))
  else:
    close_bf16(case, out.np(), ref, R.floor_of(lambda dt: B.bwd_dx(dz, x, A, Bc, Cc, dt)))


@pytest.mark.parametrize('C,M', APPLY_CASES)
def test_bwd_apply_forms(hip_lib, C, M):
  """dx = A dz + B x + C for the three mask kinds, with and without the gated gradient written out (dz_out == dy gated, bit
  for bit: a gated-off element is +0.0), and the two-norm form"""
  for kind in ('grid', 'random'):
    dy, x, xb, co, yout, maskb = _bwd_inputs(C, M, kind)
    dyt, xt, xbt, yt, mt = In(dy), In(x), In(xb), In(yout), In(maskb, U8, 0xFF)
    cot = [In(c, F32) for c in co]
    co6 = In(co, F32)
    for k in (0, 1, 2):
      gate = B.gate_of(k, yout if k == 1 else maskb, C)
      dz = B.gated(dy, gate)
      if k:
        assert (dz[gate == 0] == 0).all() and (k == 2 or not gate[yout == 0].any())
      for with_dz in (False, True):
        case = 'bn_bwd_apply %s C=%d M=%d kind %d dz %d' % (kind, C, M, k, with_dz)
        dx, dzo = Out((M, C), BF), Out((M, C), BF) if with_dz else None
        call('asm_bn_bwd_apply', dyt.p, xt.p, None if k == 0 else yt.p if k == 1 else mt.p, k, M, C, cot[0].p, cot[1].p,
             cot[2].p, dx.p, dzo.p if dzo else None)
        _judge_dx(case, kind, dx, dz, x, co[0], co[1], co[2])
        if dzo is not None:
          exact(case + ' dz_out', dzo.np(), dz)
          if k:
            assert (dzo.t.view(torch.int16).cpu().numpy()[gate == 0] == 0).all(), case + ': a gated-off element is +0.0'
    gate = B.gate_of(2, maskb, C)
    dz = B.gated(dy, gate)
    dxa, dxb = Out((M, C), BF), Out((M, C), BF)
    call('asm_bn_bwd_apply2', dyt.p, xt.p, xbt.p, mt.p, M, C, co6.p, dxa.p, dxb.p)
    _judge_dx('bn_bwd_apply2 %s C=%d M=%d a' % (kind, C, M), kind, dxa, dz, x, co[0], co[1], co[2])
    _judge_dx('bn_bwd_apply2 %s C=%d M=%d b' % (kind, C, M), kind, dxb, dz, xb, co[3], co[4], co[5])
    _release_now()


# ---- constant and near-constant channels -------------------------------------------------------------------------------------
def _general_chain(x, M, C, gamma, beta):
  """bn_stats -> asm_bn_finalize -> bn_apply through the raw entry points -> (y, mean, invstd, summed partials)"""
  xt, gt, bt = In(x), In(gamma, F32), In(beta, F32)
  blocks = _abi().L().asm_bn_stats_blocks(M, C)
  p = Out((blocks, 2, C), F32)
  call('asm_bn_stats', xt.p, M, C, p.p)
  o = {k: Out((C,), F32) for k in ('mean', 'invstd', 'scale', 'shift')}
  call('asm_bn_finalize', p.p, blocks, M, C, gt.p, bt.p, EPS, MOM, None, None, o['mean'].p, o['invstd'].p, o['scale'].p,
       o['shift'].p)
  y = Out((M, C), BF)
  call('asm_bn_apply', xt.p, y.p, M, C, o['scale'].p, o['shift'].p, None, 0, 0, 0, 0, None)
  return y.np(), o['mean'].np(), o['invstd'].np(), _summed(p)


def _small_chain(x, M, C, gamma, beta):
  xt, gt, bt = In(x), In(gamma, F32), In(beta, F32)
  y, mean, invstd = Out((M, C), BF), Out((C,), F32), Out((C,), F32)
  call('asm_bn_small_fwd', xt.p, y.p, M, C, gt.p, bt.p, EPS, MOM, None, None, mean.p, invstd.p, 0, None)
  return y.np(), mean.np(), invstd.np(), None


CHAINS = (('general', _general_chain), ('bn_small', _small_chain))


@pytest.mark.parametrize('M', [37, 300, 4096])
def test_constant_channels(hip_lib, M):
  """channels that alternate between the constant 3.0 (variance exactly 0: invstd = 1 / sqrt(eps), y = beta), the constant
  bf16(0.1) (non-dyadic: E[x^2] - mean^2 cancels to a tiny value of either sign before the clamp) and integer-valued random
  data, through the general chain and bn_small_fwd"""
  C = 72
  r = R.rng(304, M)
  x = grid(r, (M, C), -4, 4)
  x[:, 0::3] = 3.0
  x[:, 1::3] = R.to_bf16(np.float32(0.1))
  gamma = r.uniform(0.5, 1.5, C).astype(np.float32)
  beta = (r.uniform(0.5, 1.5, C) * r.choice([-1, 1], C)).astype(np.float32)
  ref = B.fwd(x, gamma, beta, EPS)
  top = 1.0 / np.sqrt(np.float64(np.float32(EPS)))
  assert (ref['invstd'][0::3] == top).all()
  nd = slice(1, None, 3)
  floor_nd = R.floor_of(lambda dt: B.fwd(x[:, nd], gamma[nd], beta[nd], EPS, dtype=dt)['y'])
  whole = np.ones(C, bool)
  whole[nd] = False
  floor = R.floor_of(lambda dt: B.fwd(x[:, whole], gamma[whole], beta[whole], EPS, dtype=dt)['y'])
  for name, chain in CHAINS:
    y, mean, invstd, _ = chain(x, M, C, gamma, beta)
    case = 'constant channels %s M=%d ' % (name, M)
    close_ulp(case + 'mean', mean[whole], ref['mean'][whole])
    close_ulp(case + 'invstd', invstd[whole], ref['invstd'][whole])
    close_bf16(case + 'y', y[:, whole], ref['y'][:, whole], floor)
    close_bf16(case + 'y of the constant 3.0 is beta', y[:, 0::3], np.broadcast_to(beta[0::3].astype(np.float64), (M, C // 3)),
               floor)
    top32 = np.float32(top)
    assert (invstd[nd] <= np.float64(top32) + R.ulp32(top32)).all(), case + 'invstd of the non-dyadic constant above 1 / sqrt(eps)'
    close_bf16(case + 'y of the non-dyadic constant', y[:, nd], np.broadcast_to(beta[nd].astype(np.float64), (M, C // 3)),
               floor_nd)
    _release_now()


@pytest.mark.parametrize('M', [300, 4096])
def test_shifted_channels(hip_lib, M):
  """mean / std = 16 (x = bf16(8 + 0.5 randn)): the sums within n 2^-24 sum |terms|, y within one bf16 ulp plus four times
  the floor of a reference that evaluates E[x^2] - mean^2 in float32.  The kernels keep float32 partial sums and finish in
  float64; profiles/bn_edges_tolerances.md records how much of the bound they use."""
  C = 64
  r = R.rng(305, M)
  x = R.to_bf16((8.0 + 0.5 * r.standard_normal((M, C))).astype(np.float32))
  gamma = r.uniform(0.5, 1.5, C).astype(np.float32)
  beta = r.standard_normal(C).astype(np.float32)
  ref = B.fwd(x, gamma, beta, EPS)
  floor = R.floor_of(lambda dt: B.fwd(x, gamma, beta, EPS, dtype=dt)['y'])
  x64 = x.astype(np.float64)
  for name, chain in CHAINS:
    y, mean, invstd, sums = chain(x, M, C, gamma, beta)
    case = 'shifted channels %s M=%d ' % (name, M)
    if sums is not None:
      close_sum(case + 'sums', sums, np.stack(B.stats(x)), M, np.stack([np.abs(x64).sum(0), (x64 * x64).sum(0)]))
    close_bf16(case + 'y', y, ref['y'], floor)
    _release_now()


# ---- bn_small ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('C', [8, 64, 72])
def test_bn_small_row_boundaries(hip_lib, C, relu):
  """the register-kept path (M <= 256) and the loop path (257, 4096), M around its 32 row lanes, M = 1, one live vector column
  of eight (C = 8) and a half-filled second workgroup (C = 72), on integer grids.  mean, invstd: 1 ulp.  Moving statistics:
  old * momentum + new * (1 - momentum) with ``new`` rounded once -> 4 roundings (test_bn_finalize_kernels_on_synthetic_partials).
  dbeta: exact.  dgamma: every term (dz ((x - mean) invstd)) carries 3 roundings, a row lane adds ceil(M / 32) of them in
  float32, the rest is float64 and one final rounding -> 4 + ceil(M / 32) half-ulps of sum |terms|."""
  for M in (1, 31, 32, 33, 255, 256, 257, 4096):
    r = R.rng(306, M, C, relu)
    x, dy = grid(r, (M, C), -4, 4), grid(r, (M, C), -2, 2)
    gamma = r.uniform(0.5, 1.5, C).astype(np.float32)
    beta = r.standard_normal(C).astype(np.float32)
    mm0, mv0 = r.standard_normal(C).astype(np.float32), r.uniform(0.5, 1.5, C).astype(np.float32)
    ref = B.fwd(x, gamma, beta, EPS, MOM, mm0, mv0, relu=relu)
    floor = R.floor_of(lambda dt: B.fwd(x, gamma, beta, EPS, MOM, relu=relu, dtype=dt)['y'])
    xt, gt, bt = In(x), In(gamma, F32), In(beta, F32)
    outs = []
    for moving in (True, False):
      o = dict(y=Out((M, C), BF), mean=Out((C,), F32), invstd=Out((C,), F32), mask=Out((M, C // 8), U8),
               mm=Out((C,), F32, init=In(mm0, F32).t), mv=Out((C,), F32, init=In(mv0, F32).t))
      call('asm_bn_small_fwd', xt.p, o['y'].p, M, C, gt.p, bt.p, EPS, MOM, o['mm'].p if moving else None,
           o['mv'].p if moving else None, o['mean'].p, o['invstd'].p, int(relu), o['mask'].p)
      outs.append(o)
    o, o2 = outs
    case = 'bn_small M=%d C=%d relu %d ' % (M, C, relu)
    close_ulp(case + 'mean', o['mean'].np(), ref['mean'])
    close_ulp(case + 'invstd', o['invstd'].np(), ref['invstd'])
    if M == 1:
      assert (ref['mv_terms'][1] == 0).all() and (ref['invstd'] == 1.0 / np.sqrt(np.float64(np.float32(EPS)))).all()
    close_terms(case + 'moving_mean', o['mm'].np(), ref['mm_terms'], 4)
    close_terms(case + 'moving_var', o['mv'].np(), ref['mv_terms'], 4)
    got = o['y'].np()
    close_bf16(case + 'y', got, ref['y'], floor)
    if relu:
      exact(case + 'mask == (own output > 0)', o['mask'].np(), B.pack_mask(got > 0))
    else:
      assert (o['mask'].np() == PATTERN).all()
    # without moving statistics: identical outputs, the moving statistics keep their bits
    for k in ('y', 'mean', 'invstd', 'mask'):
      exact(case + k + ' (no moving statistics)', o2[k].np(), o[k].np())
    exact(case + 'moving_mean untouched', o2['mm'].np().astype(np.float32), mm0)
    exact(case + 'moving_var untouched', o2['mv'].np().astype(np.float32), mv0)
    # backward from the kernel's own float32 statistics
    mean32, invstd32 = o['mean'].np().astype(np.float32), o['invstd'].np().astype(np.float32)
    maskb = o['mask'].np().astype(np.uint8) if relu else None
    gate = B.gate_of(2, maskb, C) if relu else None
    b = B.bwd(dy, x, gate, gamma, mean32, invstd32, M)
    fdx = R.floor_of(lambda dt: B.bwd_dx(b['dz'], x, b['A'], b['B'], b['C'], dt))
    dyt, mt, it = In(dy), In(mean32, F32), In(invstd32, F32)
    dg, db, dx = Out((C,), F32), Out((C,), F32), Out((M, C), BF)
    call('asm_bn_small_bwd', dyt.p, xt.p, In(maskb, U8, 0xFF).p if relu else None, M, C, gt.p, mt.p, it.p, dg.p, db.p, dx.p)
    exact(case + 'dbeta', db.np(), b['dbeta'])
    xhat = (x.astype(np.float64) - mean32) * invstd32
    close_sum(case + 'dgamma', dg.np(), b['dgamma'], 4 + -(-M // 32), np.abs(b['dz'] * xhat).sum(0))
    close_bf16(case + 'dx', dx.np(), b['dx'], fdx)
    _release_now()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(hip_lib):
  """C % 8 != 0 and M = 0 for each entry point, res_mode 2 with an odd H, mask kinds 1 and 2 without their operand, bn_small
  above its row limit: ASM_EINVAL before anything is launched (the library's own launch counter stands still)"""
  L = _abi().L()
  M, C = 8, 16
  r = R.rng(307)
  a = In(grid(r, (M, C), -2, 2))
  f = In(np.ones(6 * C, np.float32), F32)
  m = In(np.zeros((M, C // 8), np.uint8), U8, 0xFF)
  y, y2, p, p2 = Out((M, C), BF), Out((M, C), BF), Out((8, 2, C), F32), Out((8, 2, C), F32)
  n0 = L.asm_launch_count()
  assert L.asm_bn_stats_blocks(0, C) < 0 and L.asm_bn_stats_blocks(M, 12) < 0 and L.asm_bn_stats_blocks(M, 0) < 0
  for Mb, Cb in ((0, C), (M, 12), (M, 0)):
    refused = [
        ('asm_bn_stats', a.p, Mb, Cb, p.p),
        ('asm_bn_apply', a.p, y.p, Mb, Cb, f.p, f.p, None, 0, 1, 0, 0, m.p),
        ('asm_bn_bwd_reduce', a.p, a.p, None, 0, Mb, Cb, f.p, f.p, p.p),
        ('asm_bn_bwd_apply', a.p, a.p, None, 0, Mb, Cb, f.p, f.p, f.p, y.p, None),
        ('asm_bn_bwd_reduce2', a.p, a.p, a.p, m.p, Mb, Cb, f.p, f.p, f.p, f.p, p.p, p2.p),
        ('asm_bn_bwd_apply2', a.p, a.p, a.p, m.p, Mb, Cb, f.p, y.p, y2.p),
        ('asm_bn_apply2', a.p, a.p, y.p, Mb, Cb, f.p, f.p, f.p, f.p, 1, None),
        ('asm_bn_small_fwd', a.p, y.p, Mb, Cb, f.p, f.p, EPS, MOM, None, None, p.p, p2.p, 0, None),
        ('asm_bn_small_bwd', a.p, a.p, None, Mb, Cb, f.p, f.p, f.p, p.p, p2.p, y.p),
    ]
    for args in refused:
      with pytest.raises(ValueError):
        call(*args)
  with pytest.raises(ValueError):          # M = N H W with an odd H
    call('asm_bn_apply', a.p, y.p, 6, C, f.p, f.p, a.p, 2, 0, 3, 2, None)
  with pytest.raises(ValueError):          # ... and an odd W
    call('asm_bn_apply', a.p, y.p, 6, C, f.p, f.p, a.p, 2, 0, 2, 3, None)
  with pytest.raises(ValueError):          # residual mode without a residual
    call('asm_bn_apply', a.p, y.p, M, C, f.p, f.p, None, 1, 0, 0, 0, None)
  for k in (1, 2):
    with pytest.raises(ValueError):
      call('asm_bn_bwd_reduce', a.p, a.p, None, k, M, C, f.p, f.p, p.p)
    with pytest.raises(ValueError):
      call('asm_bn_bwd_apply', a.p, a.p, None, k, M, C, f.p, f.p, f.p, y.p, None)
  big = In(np.zeros((4097, 8), np.float32))
  ybig = Out((4097, 8), BF)
  assert L.asm_bn_small_max_rows() == 4096
  with pytest.raises(ValueError):
    call('asm_bn_small_fwd', big.p, ybig.p, 4097, 8, f.p, f.p, EPS, MOM, None, None, p.p, p2.p, 0, None)
  with pytest.raises(ValueError):
    call('asm_bn_small_bwd', big.p, big.p, None, 4097, 8, f.p, f.p, f.p, p.p, p2.p, ybig.p)
  assert L.asm_launch_count() == n0, 'a refused call launched a kernel'
  for o in (y, y2, p, p2, ybig):
    o.check_flanks()
    assert bool((o.t.view(U8) == PATTERN).all()), 'a refused call wrote an output'
