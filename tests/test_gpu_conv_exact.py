"""Exact, guard-banded tests of the convolution kernels: every family of the forward / input-gradient kernels (general, igemm1
ring-GEMM, igemm2, igemm3, igemm8, conv_halo, the parity classes and the one-launch form of the stride-2 input gradient,
dense_small) and every form of the weight gradient, called through the C ABI on small integer operands for which the kernels'
arithmetic is exact (tests/conv_ref.py states the argument and its conditions, tests/test_conv_ref_cpu.py asserts them).  The
reference is an exact convolution rounded once to the output type and every comparison is array_equal: there is no tolerance in
this module.  Outputs lie between 0xA5 flanks and start as 0xA5, inputs lie between NaN flanks (tests/gpu_guard.py), the weight
gradient's workspace has exactly the bytes the library asks for, and every case asserts the kernel family (or weight-gradient form
and split count) it was written for, so a change of plan cannot quietly move a case to another kernel.

Contracts pinned here, with where they are stated:
  * asm_conv2d_dgrad: "addend may alias dx" (include/asm_hip.h, asm_conv2d_dgrad; csrc/igemm_common.h igemm_epilogue: "a thread
    only ever re-reads the addresses it writes itself, so in-place accumulation stays exact") -- with ASM_IGEMM_PFA 0 and 1;
  * a fused addend / pooled gradient / folded batch norm joins the accumulator AFTER its rounding to bf16 and the sum is rounded
    again (igemm_epilogue: "fused inference BN on the bf16-rounded conv tile (== the two-pass numerics)"; asm_hip.h,
    asm_conv2d_fprop_bn) -- conv_ref.dgrad_out / fprop_bn; dense_small_kernel adds in fp32 and rounds once;
  * the 1x1 / stride-2 input gradient writes one parity class: "the classes the one launch does not write are zero, or just the
    addend" (csrc/conv_igemm.hip, dgrad_impl);
  * a padded output row (ldy > K): dense_small_kernel writes the pad columns as zeros ("pad columns N .. ldo-1 of a padded output
    row are written as zeros", csrc/dense_small.hip); the convolution kernels store whole 4-column (f32) / 8-column (bf16) vectors,
    so they write nothing from column (K + 3) & ~3 resp. (K + 7) & ~7 on (igemm_epilogue: n < co4, n0 < co8) and zeros below it;
  * fused statistics / batch-norm backward sums: one [2][K] partial per 128 rows (asm_conv2d_stats_blocks), each an exact integer
    here, summing to the sums of the stored bf16 values.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import conv_ref as CR
from tests import rows_ref as R
from tests import util
from tests.gpu_guard import In, Out, Work, call, exact, _release_inputs  # noqa: F401  (the fixture is autouse)

pytestmark = pytest.mark.gpu

BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8


def _set(monkeypatch, knobs):
  for name, value in knobs.items():
    util.set_knob(monkeypatch, name, value)


def _desc(shape, **kw):
  from assembled_cnn_amd import ops
  N, H, W, Cn, K, k, stride = shape
  return ops.make_conv_desc(N, H, W, Cn, K, k, k, stride, **kw)


def _ran_on(hip_lib, family, what):
  got = hip_lib.asm_debug_last_conv_kernel()
  assert got == family, '%s ran on kernel family %d, the case is written for family %d' % (what, got, family)


def _in(a, *args):
  """the shared references are read-only: the device copy is made from a private one"""
  return In(np.array(a), *args)


def _t(a):
  return torch.from_numpy(np.array(a))


def _mask(a):
  return _in(a, U8, 0xFF)


def _wt(w, ldk=0):
  """the input gradient's filter [C][R][S][ldk], permuted on the CPU: asm_filter_transpose stays out of the chain"""
  return _in(R.filter_transpose(w, ldk))


# ---- forward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CR.CONV_CASES, ids=CR.case_id)
def test_forward(hip_lib, case, monkeypatch):
  """asm_conv2d_fprop with and without the fused statistics, and asm_conv2d_fprop_bn where the family has it"""
  _set(monkeypatch, case.knobs)
  ref = CR.conv_reference(case.shape)
  d, M, K = _desc(case.shape), ref['M'], case.shape[4]
  x, w = _in(ref['x']), _in(ref['w'])
  want = CR.round_bf16(ref['acc_f'])
  blocks = hip_lib.asm_conv2d_stats_blocks(C.byref(d))
  assert blocks == -(-M // CR.STATS_BM)
  y, part = Out((M, K), BF), Out((blocks, 2, K), F32)
  call('asm_conv2d_fprop', C.byref(d), x.p, w.p, y.p, part.p)
  _ran_on(hip_lib, case.fam_f, 'forward + statistics')
  exact('forward (+ statistics)', y.np(), want)
  sums = part.np()      # flanks intact, nothing NaN; the values are exact integers only under condition 3 of conv_ref
  if ref['Lf'] <= CR.STATS_L:
    CR.exact_partials('fused statistics', sums, CR.stats(want))
  y = Out((M, K), BF)
  call('asm_conv2d_fprop', C.byref(d), x.p, w.p, y.p, 0)
  _ran_on(hip_lib, case.fam_f, 'forward')
  exact('forward', y.np(), want)
  if 'bn' not in case.flags:
    return
  scale, shift, res = _in(ref['scale'], F32), _in(ref['shift'], F32), _in(ref['residual'])
  for with_res, relu in ((False, True), (True, True), (True, False), (False, False)):
    y = Out((M, K), BF)
    call('asm_conv2d_fprop_bn', C.byref(d), x.p, w.p, y.p, scale.p, shift.p, res.p if with_res else 0, 1 if relu else 0)
    _ran_on(hip_lib, case.fam_f, 'forward + folded batch norm')
    exact('folded batch norm, residual %d, relu %d' % (with_res, relu), y.np(),
          CR.fprop_bn(ref['acc_f'], ref['scale'], ref['shift'], ref['residual'] if with_res else None, relu))


# ---- input gradient -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CR.CONV_CASES, ids=CR.case_id)
def test_input_gradient(hip_lib, case, monkeypatch):
  """asm_conv2d_dgrad plain, with an addend, in place (addend == dx) under both addend epilogues, and asm_conv2d_dgrad_masked"""
  _set(monkeypatch, case.knobs)
  ref = CR.conv_reference(case.shape)
  d, Mi, Cn = _desc(case.shape), ref['Mi'], case.shape[3]
  dy, wt, addend, mask = _in(ref['dy']), _wt(ref['w']), _in(ref['addend']), _mask(ref['mask'])
  dx = Out((Mi, Cn), BF)
  call('asm_conv2d_dgrad', C.byref(d), dy.p, wt.p, 0, dx.p)
  _ran_on(hip_lib, case.fam_d, 'input gradient')
  plain = dx.np()
  exact('input gradient', plain, CR.dgrad_out(ref['acc_d']))
  want = CR.dgrad_out(ref['acc_d'], ref['addend'])
  dx = Out((Mi, Cn), BF)
  call('asm_conv2d_dgrad', C.byref(d), dy.p, wt.p, addend.p, dx.p)
  _ran_on(hip_lib, case.fam_d, 'input gradient + addend')
  exact('input gradient + addend', dx.np(), want)
  if 'nomask' not in case.flags:
    dx = Out((Mi, Cn), BF)
    call('asm_conv2d_dgrad_masked', C.byref(d), dy.p, wt.p, addend.p, mask.p, dx.p)
    _ran_on(hip_lib, case.fam_d, 'input gradient + masked addend')
    exact('input gradient + masked addend', dx.np(), CR.dgrad_out(ref['acc_d'], ref['addend'], ref['mask']))
  for pfa in ('0', '1'):      # both addend epilogues (a family without the prefetching one runs its only one twice)
    util.set_knob(monkeypatch, 'ASM_IGEMM_PFA', pfa)
    dx = Out((Mi, Cn), BF, init=_t(ref['addend']))
    call('asm_conv2d_dgrad', C.byref(d), dy.p, wt.p, dx.p, dx.p)
    _ran_on(hip_lib, case.fam_d, 'input gradient in place')
    inplace = dx.np()
    exact('input gradient in place, ASM_IGEMM_PFA=%s' % pfa, inplace, want)
  if case.shape[5] == 1 and case.shape[6] == 2:
    # one parity class is computed; the other three quarters of dx are exact zeros, or exactly the addend
    N, H, W = case.shape[:3]
    other = np.ones((N, H, W), bool)
    other[:, ::2, ::2] = False
    assert not plain.reshape(N, H, W, Cn)[other].any()
    exact('the addend alone', inplace.reshape(N, H, W, Cn)[other], ref['addend'].reshape(N, H, W, Cn)[other].astype(np.float64))


POOL_CASES = [c for c in CR.CONV_CASES if 'pool' in c.flags]
BNRED_CASES = [c for c in CR.CONV_CASES if 'bnred' in c.flags]


@pytest.mark.parametrize('geometry', [(2, 2, False), (2, 2, True), (2, 1, False), (2, 1, True)],
                         ids=lambda g: 'k%d-s%d-%s' % (g[0], g[1], 'valid' if g[2] else 'kk'))
@pytest.mark.parametrize('case', POOL_CASES, ids=CR.case_id)
def test_input_gradient_with_the_pooled_gradient_gathered(hip_lib, case, geometry, monkeypatch):
  """asm_conv2d_dgrad_pooled (2 x 2 average pool of stride 1 or 2, divisor 4 or the taps inside the map), without an addend and
  with a masked one"""
  _set(monkeypatch, case.knobs)
  ref = CR.conv_reference(case.shape)
  N, H, W, Cn = case.shape[:4]
  k, stride, cv = geometry
  d, Mi = _desc(case.shape), ref['Mi']
  ps = CR.pool_shape((N, H, W, Cn), k, stride, cv)
  g = CR.pooled_of(R.rng(CR.seed_of('pool', case.shape, geometry)), ps)
  share = CR.pool_bwd(g, (N, H, W, Cn), k, stride, cv)
  dy, wt, addend, mask, pdy = _in(ref['dy']), _wt(ref['w']), _in(ref['addend']), _mask(ref['mask']), _in(g)
  for masked in (False, True):
    dx = Out((Mi, Cn), BF)
    call('asm_conv2d_dgrad_pooled', C.byref(d), dy.p, wt.p, addend.p if masked else 0, mask.p if masked else 0, pdy.p, k, stride, 0,
         ps[1], ps[2], 1 if cv else 0, dx.p)
    _ran_on(hip_lib, case.fam_d, 'pooled input gradient')
    exact('pooled input gradient, masked addend %d' % masked, dx.np(),
          CR.dgrad_out(ref['acc_d'], ref['addend'] if masked else None, ref['mask'] if masked else None, pool=share))


@pytest.mark.parametrize('case', BNRED_CASES, ids=CR.case_id)
def test_input_gradient_with_the_batch_norm_backward_sums(hip_lib, case, monkeypatch):
  """asm_conv2d_dgrad_bnred: dx as asm_conv2d_dgrad[_masked] writes it, the partials (sum dz, sum dz y) exact, with and without the
  ReLU mask"""
  _set(monkeypatch, case.knobs)
  ref = CR.conv_reference(case.shape)
  d, Mi, Cn = _desc(case.shape), ref['Mi'], case.shape[3]
  blocks = hip_lib.asm_conv2d_dgrad_bnred_blocks(C.byref(d))
  assert blocks == -(-Mi // CR.STATS_BM)
  dy, wt, addend, mask = _in(ref['dy']), _wt(ref['w']), _in(ref['addend']), _mask(ref['mask'])
  bn_y, relu_mask = _in(ref['bn_y']), _mask(ref['relu_mask'])
  for fan_in, relu in ((False, False), (True, True), (False, True)):
    dx, part = Out((Mi, Cn), BF), Out((blocks, 2, Cn), F32)
    call('asm_conv2d_dgrad_bnred', C.byref(d), dy.p, wt.p, addend.p if fan_in else 0, mask.p if fan_in else 0, bn_y.p,
         relu_mask.p if relu else 0, part.p, dx.p)
    _ran_on(hip_lib, case.fam_d, 'input gradient + batch-norm sums')
    want = CR.dgrad_out(ref['acc_d'], ref['addend'] if fan_in else None, ref['mask'] if fan_in else None)
    exact('dx, fan-in %d' % fan_in, dx.np(), want)
    CR.exact_partials('batch-norm backward sums, fan-in %d, relu %d' % (fan_in, relu), part.np(),
                      CR.bn_sums(want, ref['bn_y'], ref['relu_mask'] if relu else None))


# ---- dense [N,1,1,C] layers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dense_small', ['1', '0'], ids=['dense_small', 'conv-kernels'])
@pytest.mark.parametrize('case', CR.DENSE_CASES, ids=lambda c: 'x'.join(map(str, c[:4])))
def test_dense_layer(hip_lib, case, dense_small, monkeypatch):
  """forward (bf16 and f32 out, padded rows), input gradient (plain, addend, in place) and weight gradient of a [N,1,1,C] layer: on
  dense_small.hip's products (family 6) where the direction's reduction is a multiple of 16, and on the convolution kernels
  otherwise and with ASM_DENSE_SMALL=0"""
  util.set_knob(monkeypatch, 'ASM_DENSE_SMALL', dense_small)
  N, Cn, K, ld = case[:4]
  fam_f, fam_d = (case.fam_f, case.fam_d) if dense_small == '1' else (case.fam_f0, case.fam_d0)
  ref = CR.dense_reference(case)
  ldy = ld or K
  x, w = _in(ref['x']), _in(ref['w'])
  for out_f32 in (False, True):
    d = _desc((N, 1, 1, Cn, K, 1, 1), ldy=ld, out_f32=out_f32)
    y = Out((N, ldy), F32 if out_f32 else BF)
    call('asm_conv2d_fprop', C.byref(d), x.p, w.p, y.p, 0)
    _ran_on(hip_lib, fam_f, 'forward of a [N,1,1,C] layer')
    got = y.np()
    want = ref['acc_f'] if out_f32 else CR.round_bf16(ref['acc_f'])
    if fam_f == CR.DENSE:
      # dense_small.hip: "pad columns N .. ldo-1 of a padded output row are written as zeros"
      CR.exact_rows('dense forward, f32 %d' % out_f32, got, want, 0.0)
    else:
      # igemm_epilogue stores whole vectors of 4 floats / 8 bf16 (n < co4, n0 < co8): zeros up to that boundary, nothing beyond
      edge = min((K + 3) & ~3 if out_f32 else (K + 7) & ~7, ldy)
      CR.exact_rows('forward, f32 %d' % out_f32, got[:, :edge], want, 0.0)
      CR.exact_rows('forward, f32 %d: beyond the last vector' % out_f32, got[:, edge:], want[:, :0],
                    CR.FILL_F32 if out_f32 else CR.FILL_BF16)
  # weight gradient from a dy with padded rows (zeros in the pad columns): the dense form whatever the reduction, up to 1024 rows
  wref = CR.wgrad_reference((N, 1, 1, Cn, K, 1, 1), ld)
  d = _desc((N, 1, 1, Cn, K, 1, 1), ldy=ld)
  plan = (C.c_int32 * 6)()
  assert hip_lib.asm_conv2d_wgrad_plan(C.byref(d), C.byref(plan)) == 0
  rows = 32 if K < 33 else 64 if K < 65 else 128      # wgrad_kernel's dy tile
  assert list(plan)[:2] == ([K, -2] if dense_small == '1' else [rows, 128]) and plan[4] == 1, list(plan)
  ws = Work(hip_lib.asm_conv2d_wgrad_workspace_bytes(C.byref(d)))
  assert ws.nbytes == 0
  dw = Out((K, Cn), F32)
  call('asm_conv2d_wgrad', C.byref(d), _in(wref['x']).p, _in(wref['dy']).p, dw.p, ws.p, ws.nbytes)
  exact('dense weight gradient', dw.np(), wref['dw'].reshape(K, Cn))
  ws.check_flanks()
  # input gradient; asm_conv2d_dgrad takes K % 8 == 0, so K = 100 runs padded to 104: zero columns in dy, zero rows in the filter
  Kp = (K + 7) & ~7
  d = _desc((N, 1, 1, Cn, Kp, 1, 1))
  dyp = np.zeros((N, Kp), np.float32)
  dyp[:, :K] = ref['dy']
  dy, wt, addend = _in(dyp), _wt(ref['w'], Kp), _in(ref['addend'])
  # dense_small_kernel adds the addend to the fp32 sum and rounds once; with every sum below 256 that is the two-step form too
  for name in ('plain', 'addend', 'in place'):
    dx = Out((N, Cn), BF, init=_t(ref['addend']) if name == 'in place' else None)
    call('asm_conv2d_dgrad', C.byref(d), dy.p, wt.p, {'plain': 0, 'addend': addend.p, 'in place': dx.p}[name], dx.p)
    _ran_on(hip_lib, fam_d, 'input gradient of a [N,1,1,C] layer')
    exact('dense input gradient, ' + name, dx.np(), CR.dgrad_out(ref['acc_d'], None if name == 'plain' else ref['addend']))


# ---- stem: pitched input through nn.ConvKernel(stem=True) ---------------------------------------------------------------------
@pytest.mark.parametrize('case', CR.STEM_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_stem_layer(hip_lib, case):
  """the 7x7 / 2 and 3x3 / 2 first convolutions over the zero-haloed [N][H+6][W+6][4] buffer (R = k, S = 1, rows of 4-channel
  pixels): forward with statistics and weight gradient.  The buffer lies between NaN flanks: the view a k = 3 layer gets starts
  two rows in while the descriptor's extent is the whole buffer's, so a read beyond the halo would come back as NaN."""
  from assembled_cnn_amd import nn, ops
  N, H, W, k, K = case
  ref = CR.stem_reference(case)
  dev = torch.device('cuda')
  arena = nn.ParamArena()
  conv = nn.ConvKernel(nn.Ctx(arena, True, True, 0.997, dev, False), k, 3, K, stem=True)
  arena.finalize(dev, 0)
  arena.w(conv.name).copy_(_t(ref['w']))
  arena.refresh_shadows()
  exact('packed stem filter', conv.weight().float().cpu().numpy().reshape(K, k, -1), ref['wp'])
  d, rd = conv.desc(N, H, W, 2), ref['d']
  assert [getattr(d, f) for f in ('N', 'H', 'W', 'C', 'K', 'R', 'S', 'stride', 'pad', 'Ho', 'Wo', 'x_img_pitch', 'x_row_pitch', 'x_pix_pitch')] == \
         [getattr(rd, f) for f in ('N', 'H', 'W', 'C', 'K', 'R', 'S', 'stride', 'pad', 'Ho', 'Wo', 'x_img_pitch', 'x_row_pitch', 'x_pix_pitch')]
  xp = _in(ref['xp'])
  view = conv._stem_view(xp.t)
  assert view.data_ptr() - xp.t.data_ptr() == 2 * CR.stem_view_offset(W, k)
  M, blocks = ref['M'], -(-ref['M'] // CR.STATS_BM)
  want = CR.round_bf16(ref['acc_f'])
  for with_stats in (True, False):
    y, part = Out((M, K), BF), Out((blocks, 2, K), F32)
    call('asm_conv2d_fprop', C.byref(d), view.data_ptr(), conv.weight().data_ptr(), y.p, part.p if with_stats else 0)
    _ran_on(hip_lib, CR.IGEMM2, 'stem forward')
    exact('stem forward', y.np(), want)
    if with_stats:
      CR.exact_partials('stem statistics', part.np(), CR.stats(want))
    else:
      part.check_flanks()
      assert bool((part.buf.view(U8) == 0xA5).all()), 'statistics written without being asked for'
  plan = (C.c_int32 * 6)()
  assert hip_lib.asm_conv2d_wgrad_plan(C.byref(d), C.byref(plan)) == 0
  assert plan[1] == 128
  ws = Work(hip_lib.asm_conv2d_wgrad_workspace_bytes(C.byref(d)))
  assert ws.nbytes == (plan[4] * K * k * rd.C * 4 if plan[4] > 1 else 0)
  dwp = Out((K, k, rd.C), F32)
  call('asm_conv2d_wgrad', C.byref(d), view.data_ptr(), _in(ref['dy']).p, dwp.p, ws.p, ws.nbytes)
  exact('packed stem weight gradient', dwp.np(), ref['dwp'])
  ws.check_flanks()
  ops.stem_unpack_grad(dwp.t, arena.g(conv.name), K, k)
  exact('stem weight gradient', arena.g(conv.name).double().cpu().numpy(), ref['dw'])


# ---- weight gradient ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CR.WGRAD_CASES, ids=CR.case_id)
def test_weight_gradient(hip_lib, case, monkeypatch):
  """asm_conv2d_wgrad: dw (fp32) exact, pre-filled with the pattern; the workspace exactly asm_conv2d_wgrad_workspace_bytes
  between flanks; the form and the split count are the plan's.  The 256 x 256 form with a K tail (264 of 512 rows) is exact too:
  ASM_WGRAD_BIG=1 admits K >= 256 that is no multiple of 256, and wgrad8_kernel masks its loads and stores by K."""
  _set(monkeypatch, case.knobs)
  ref = CR.wgrad_reference(case.shape)
  N, H, W, Cn, K, k, stride = case.shape
  d = _desc(case.shape)
  plan = (C.c_int32 * 6)()
  assert hip_lib.asm_conv2d_wgrad_plan(C.byref(d), C.byref(plan)) == 0
  assert (plan[1], plan[4]) == (case.bcw, case.splits), 'planned %s' % list(plan)
  cols = k * k * Cn
  ws = Work(hip_lib.asm_conv2d_wgrad_workspace_bytes(C.byref(d)))
  slabs = case.splits if (case.bcw == -1 or case.splits > 1) else 0      # the halo form always sums slabs
  assert ws.nbytes == slabs * K * cols * 4
  dw = Out((K, k, k, Cn), F32)
  call('asm_conv2d_wgrad', C.byref(d), _in(ref['x']).p, _in(ref['dy']).p, dw.p, ws.p, ws.nbytes)
  exact('weight gradient', dw.np(), ref['dw'])
  ws.check_flanks()
