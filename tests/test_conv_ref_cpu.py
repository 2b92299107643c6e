"""tests/conv_ref.py on the CPU: its convolution references against torch.nn.functional.conv2d in float64 and autograd through
it, and against the oracle's _conv_raw; the conditions its exactness argument needs, for every case of every table; and the
sensitivity of the comparison helpers tests/test_gpu_conv_exact.py uses to the damages a kernel could do."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as CR
from tests import rows_ref as R

CONV_SHAPES = sorted({c.shape for c in CR.CONV_CASES} | {(c.N, 1, 1, c.C, c.K, 1, 1) for c in CR.DENSE_CASES})
WGRAD_SHAPES = sorted({c.shape for c in CR.WGRAD_CASES})
_id = lambda s: 'x'.join(map(str, s))     # noqa: E731


def _torch_conv(x_nhwc, w_krsc, stride, Ho, Wo):
  """F.conv2d in float64 with the descriptor's padding: (k - 1) // 2 before, after whatever Ho / Wo imply"""
  k = w_krsc.shape[1]
  H, W = x_nhwc.shape[1:3]
  pb = (k - 1) // 2
  pa_h, pa_w = (Ho - 1) * stride + k - H - pb, (Wo - 1) * stride + k - W - pb
  xp = F.pad(x_nhwc.permute(0, 3, 1, 2), (pb, max(pa_w, 0), pb, max(pa_h, 0)))
  y = F.conv2d(xp, w_krsc.permute(0, 3, 1, 2), stride=stride)
  assert y.shape[2:] == (Ho, Wo)
  return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize('shape', CONV_SHAPES, ids=_id)
def test_forward_and_input_gradient_against_conv2d_and_autograd(shape):
  ref = CR.conv_reference(shape)
  d = ref['d']
  x = torch.from_numpy(ref['x'].astype(np.float64)).requires_grad_(True)
  w = torch.from_numpy(ref['w'].astype(np.float64))
  y = _torch_conv(x, w, d.stride, d.Ho, d.Wo)
  assert np.array_equal(y.detach().numpy().reshape(ref['M'], d.K), ref['acc_f'])
  dy = torch.from_numpy(ref['dy'].astype(np.float64)).view(d.N, d.Ho, d.Wo, d.K)
  gx, = torch.autograd.grad(y, [x], dy)
  assert np.array_equal(gx.numpy().reshape(ref['Mi'], d.C), ref['acc_d'])


@pytest.mark.parametrize('shape', WGRAD_SHAPES, ids=_id)
def test_weight_gradient_against_autograd(shape):
  ref = CR.wgrad_reference(shape)
  d = ref['d']
  x = torch.from_numpy(ref['x'].astype(np.float64))
  w = torch.zeros((d.K, d.R, d.S, d.C), dtype=torch.float64, requires_grad=True)
  y = _torch_conv(x, w, d.stride, d.Ho, d.Wo)
  gw, = torch.autograd.grad(y, [w], torch.from_numpy(ref['dy'].astype(np.float64)).view(d.N, d.Ho, d.Wo, d.K))
  assert np.array_equal(gw.numpy(), ref['dw'])


def test_weight_gradient_ignores_the_pad_columns_of_a_padded_dy_row():
  N, C, K, ld = CR.DENSE_CASES[2][:4]
  ref = CR.wgrad_reference((N, 1, 1, C, K, 1, 1), ld)
  assert ref['dy'].shape == (N, ld) and not ref['dy'][:, K:].any()
  assert np.array_equal(ref['dw'].reshape(K, C), ref['dy'][:, :K].astype(np.float64).T @ ref['x'].reshape(N, C).astype(np.float64))


@pytest.mark.parametrize('case', CR.STEM_CASES, ids=_id)
def test_pitched_stem_layout_against_conv2d_and_autograd(case):
  """the stem descriptor (R = k, S = 1, lanes of 4-channel pixels over the haloed buffer) is the k x k / 2 convolution of the
  3-channel image, and no tap reads past the buffer (the reference puts NaN there)"""
  N, H, W, k, K = case
  ref = CR.stem_reference(case)
  d = ref['d']
  assert np.isfinite(ref['acc_f']).all() and np.isfinite(ref['dwp']).all()
  x = torch.from_numpy(ref['xp'][:, 3:3 + H, 3:3 + W, :3].astype(np.float64))
  w = torch.from_numpy(ref['w'].astype(np.float64)).requires_grad_(True)
  y = _torch_conv(x, w, 2, d.Ho, d.Wo)
  assert np.array_equal(y.detach().numpy().reshape(ref['M'], K), ref['acc_f'])
  gw, = torch.autograd.grad(y, [w], torch.from_numpy(ref['dy'].astype(np.float64)).view(N, d.Ho, d.Wo, K))
  assert np.array_equal(gw.numpy(), ref['dw'])
  # the lanes of the zero fourth channel carry no gradient
  assert not ref['dwp'][:, :, 3:4 * k:4].any()


@pytest.mark.parametrize('shape', [(2, 9, 9, 72, 40, 3, 1), (4, 15, 15, 64, 64, 3, 2), (2, 9, 11, 64, 96, 1, 2)], ids=_id)
def test_against_the_oracle(shape):
  from oracle import assembled_oracle as O
  ref = CR.conv_reference(shape)
  d = ref['d']
  x = torch.from_numpy(ref['x'].astype(np.float64)).permute(0, 3, 1, 2).requires_grad_(True)
  w = torch.from_numpy(ref['w'].astype(np.float64)).permute(1, 2, 3, 0).requires_grad_(True)      # KRSC -> HWIO
  y = O._conv_raw(x, w, d.R, d.stride)
  assert tuple(y.shape) == (d.N, d.K, d.Ho, d.Wo)
  assert np.array_equal(y.detach().permute(0, 2, 3, 1).numpy().reshape(ref['M'], d.K), ref['acc_f'])
  dy = torch.from_numpy(ref['dy'].astype(np.float64)).view(d.N, d.Ho, d.Wo, d.K).permute(0, 3, 1, 2)
  gx, gw = torch.autograd.grad(y, [x, w], dy)
  assert np.array_equal(gx.permute(0, 2, 3, 1).numpy().reshape(ref['Mi'], d.C), ref['acc_d'])
  wr = CR.wgrad(ref['x'], ref['dy'], d)
  assert np.array_equal(gw.permute(3, 0, 1, 2).numpy(), wr)


def test_descriptor_rules_are_the_products():
  from assembled_cnn_amd import ops
  for shape in CONV_SHAPES + WGRAD_SHAPES:
    N, H, W, C, K, k, stride = shape
    a, b = CR.desc_of(shape), ops.make_conv_desc(N, H, W, C, K, k, k, stride)
    assert (a.pad, a.Ho, a.Wo) == (b.pad, b.Ho, b.Wo), shape


# ---- number formats and epilogues ---------------------------------------------------------------------------------------------
def test_round_bf16_is_one_nearest_even_cast():
  v = np.concatenate([np.arange(-1100, 1101), np.arange(-2100, 2101) / 4.0])
  want = torch.from_numpy(v.astype(np.float32)).to(torch.bfloat16).double().numpy()
  assert np.array_equal(CR.round_bf16(v), want)
  ints = np.arange(-256, 257)
  assert np.array_equal(CR.round_bf16(ints), ints), 'bf16 holds every integer up to 256'
  even = np.arange(-512, 513, 2)
  assert np.array_equal(CR.round_bf16(even), even), 'and every even one up to 512'
  assert CR.round_bf16(np.array([257.0, 259.0])).tolist() == [256.0, 260.0]        # ties go to the even mantissa
  with pytest.raises(AssertionError):
    CR.round_bf16(np.array([1.0 + 2.0 ** -30]))


def test_mask_bit_order_and_the_epilogue_formulas():
  mask = np.array([[0b00000101, 0b10000000]], np.uint8)
  assert CR.mask_bits(mask, 16).tolist() == [[1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]]
  acc = np.array([[257.0, -3.0, 300.0, 7.0, 1.0, 1.0, 1.0, 1.0]])
  add = np.array([[1.0, 2.0, 3.0, 4.0, 0.0, 0.0, 0.0, 0.0]])
  # the accumulator is rounded before the addend joins it: 257 -> 256, + 1 = 257 -> 256; 300 -> 300, + 3 = 303 -> 304
  assert CR.dgrad_out(acc, add)[0, :4].tolist() == [256.0, -1.0, 304.0, 11.0]
  assert CR.dgrad_out(acc, add, np.array([[0b00001010]], np.uint8))[0, :4].tolist() == [256.0, -1.0, 300.0, 11.0]
  scale, shift = np.array([0.25] * 8, np.float32), np.array([-1.75] * 8, np.float32)
  assert CR.fprop_bn(acc, scale, shift, None, True)[0, :4].tolist() == [62.25, 0.0, 73.0, 0.0]
  assert CR.fprop_bn(acc, scale, shift, add, False)[0, :2].tolist() == [63.25, -0.5]
  y = np.array([[1.0, -2.0], [3.0, 4.0]])
  assert CR.stats(y).tolist() == [[4.0, 2.0], [10.0, 20.0]]
  dx, by = np.arange(16.0).reshape(2, 8), np.full((2, 8), 2.0)
  assert CR.bn_sums(dx, by)[1].tolist() == (2 * (dx[0] + dx[1])).tolist()
  assert CR.bn_sums(dx, by, np.array([[1], [255]], np.uint8))[0].tolist() == [8.0] + list(dx[1, 1:])


@pytest.mark.parametrize('k,stride,cv', [(2, 2, False), (2, 2, True), (2, 1, False), (2, 1, True)])
def test_pooled_gradient_reference_is_the_adjoint_of_the_average_pool(k, stride, cv):
  """pool_bwd against autograd through torch's average pool on an odd map; its weights are quarters, halves or ones, so with
  multiples of 4 coming in every share is an integer"""
  shape = (2, 7, 9, 8)
  N, H, W, C = shape
  ps = CR.pool_shape(shape, k, stride, cv)
  g = CR.pooled_of(R.rng(5), ps)
  got = CR.pool_bwd(g, shape, k, stride, cv)
  assert np.array_equal(got, np.rint(got))
  x = torch.zeros((N, C, H, W), dtype=torch.float64, requires_grad=True)
  xp = F.pad(x, (0, (ps[2] - 1) * stride + k - W, 0, (ps[1] - 1) * stride + k - H))
  y = F.avg_pool2d(xp, k, stride)
  if cv:      # the divisor counts the taps inside the map
    ones = F.pad(torch.ones((1, 1, H, W), dtype=torch.float64), (0, xp.shape[3] - W, 0, xp.shape[2] - H))
    y = y / F.avg_pool2d(ones, k, stride)
  gx, = torch.autograd.grad(y, [x], torch.from_numpy(g.astype(np.float64)).permute(0, 3, 1, 2))
  assert np.array_equal(gx.permute(0, 2, 3, 1).numpy().reshape(-1, C), got)


# ---- the conditions of the exactness argument ---------------------------------------------------------------------------------
def _share(acc):
  a = np.abs(acc)
  return float(a.max()), float((a > 256).mean())


@pytest.mark.parametrize('case', CR.CONV_CASES, ids=CR.case_id)
def test_conditions_of_a_forward_and_input_gradient_case(case):
  ref = CR.conv_reference(case.shape)
  for what, L, acc, fused in (('forward', ref['Lf'], ref['acc_f'], True), ('input gradient', ref['Ld'], ref['acc_d'], 'bnred' in case.flags)):
    worst, share = _share(acc)
    print('\nconv-exact %-44s %-14s L %5d  worst |sum| %4d  share above 256 %.2e' % (CR.case_id(case), what, L, worst, share), end='')
    assert 2 * L < 2 ** 24                                                    # condition 1
    assert share <= 0.01                                                      # condition 2
    if fused and L <= CR.STATS_L:                                             # condition 3
      assert worst <= 256 and share == 0.0
  if 'bnred' in case.flags:
    assert ref['Ld'] <= CR.STATS_L, 'a case that checks the batch-norm backward sums needs L <= 1152'
    # with the addend on top the stored values are still integers of at most 260, times |y| <= 3 over 128 rows: far below 2^24
    assert 128 * 3 * (256 + 4) < 2 ** 24
  for name in ('x', 'w', 'dy', 'addend', 'bn_y', 'scale'):
    assert np.all(ref[name] != 0), name + ' holds a zero'


@pytest.mark.parametrize('case', CR.DENSE_CASES, ids=lambda c: _id(c[:4]))
def test_conditions_of_a_dense_case(case):
  N, C, K, ld = case[:4]
  ref = CR.dense_reference(case)
  for what, L, acc in (('forward', C, ref['acc_f']), ('input gradient', K, ref['acc_d'])):
    worst, share = _share(acc)
    print('\nconv-exact dense %-38s %-14s L %5d  worst |sum| %4d  share above 256 %.2e' % (_id(case[:4]), what, L, worst, share), end='')
    assert 2 * L < 2 ** 24 and worst <= 256


@pytest.mark.parametrize('case', CR.STEM_CASES, ids=_id)
def test_conditions_of_a_stem_case(case):
  ref = CR.stem_reference(case)
  worst, share = _share(ref['acc_f'])
  print('\nconv-exact stem %-39s forward        L %5d  worst |sum| %4d  share above 256 %.2e' % (
      _id(case), ref['d'].R * ref['d'].C, worst, share), end='')
  assert worst <= 256                        # statistics are checked
  assert 6 * ref['M'] < 2 ** 24


@pytest.mark.parametrize('case', CR.WGRAD_CASES, ids=CR.case_id)
def test_conditions_of_a_weight_gradient_case(case):
  ref = CR.wgrad_reference(case.shape)
  print('\nconv-exact %-44s weight gradient M %5d  worst |sum| %5d' % (CR.case_id(case), ref['M'], np.abs(ref['dw']).max()), end='')
  assert 6 * ref['M'] < 2 ** 24              # |x| <= 3, |dy| <= 2: every partial sum of the fp32 output is an exact integer
  assert np.all(ref['x'] != 0) and np.all(ref['dy'][:, :ref['d'].K] != 0)


def test_every_family_and_form_is_in_the_tables():
  assert {c.fam_f for c in CR.CONV_CASES} | {c.fam_d for c in CR.CONV_CASES} == {0, 1, 2, 3, 4, 5, 8}     # dense (6): DENSE_CASES
  for fam in (0, 1, 2, 3, 4, 8):
    assert any(c.fam_f == fam for c in CR.CONV_CASES) and any(c.fam_d == fam for c in CR.CONV_CASES), fam
  assert {c.bcw for c in CR.WGRAD_CASES} == {128, 256, -1}
  assert {c.knobs.get('ASM_GEMM1') for c in CR.CONV_CASES if c.fam_f == CR.GEMM1} == set(map(str, CR.GEMM1_CODES))


# ---- sensitivity: what a kernel could do wrong must fail the helpers the GPU module uses ---------------------------------------------
SENSITIVE = [(2, 9, 9, 72, 40, 3, 1), (3, 7, 7, 256, 512, 3, 1), (5, 7, 7, 192, 136, 3, 1)]


@pytest.mark.parametrize('shape', SENSITIVE, ids=_id)
def test_one_product_removed_from_one_output_fails(shape):
  ref = CR.conv_reference(shape)
  good = CR.round_bf16(ref['acc_f'])
  CR.exact('undamaged', good, CR.round_bf16(ref['acc_f']))
  m, k = np.argwhere(np.abs(ref['acc_f']) < 200)[17]
  acc = ref['acc_f'].copy()
  acc[m, k] -= float(ref['x'].reshape(-1, shape[3])[0, 0]) * float(ref['w'][k, 1, 1, 0])      # one product: +-1 or +-2
  with pytest.raises(AssertionError):
    CR.exact('one product removed', CR.round_bf16(acc), good)
  # ... and from a fused sum: the statistics move by the same integer
  with pytest.raises(AssertionError):
    CR.exact_partials('one product removed', CR.stats(CR.round_bf16(acc))[None], CR.stats(good))


@pytest.mark.parametrize('shape', SENSITIVE, ids=_id)
def test_a_border_tap_read_from_the_wrapped_around_pixel_fails(shape):
  """output pixel (0, 1, 0): its taps s = 0 lie left of the map; a kernel that forgets the column test reads the last pixel of
  the row above instead of zero"""
  ref = CR.conv_reference(shape)
  d = ref['d']
  x, w = ref['x'].astype(np.float64), ref['w'].astype(np.float64)
  acc = ref['acc_f'].copy()
  m = 1 * d.Wo + 0
  for r in range(3):
    ih = 1 + r - 1
    acc[m] += x.reshape(-1, d.C)[ih * d.W - 1] @ w[:, r, 0, :].T
  with pytest.raises(AssertionError):
    CR.exact('wrapped tap', CR.round_bf16(acc), CR.round_bf16(ref['acc_f']))


@pytest.mark.parametrize('shape', SENSITIVE, ids=_id)
def test_a_row_of_a_ragged_tile_left_at_the_fill_pattern_fails(shape):
  ref = CR.conv_reference(shape)
  good = CR.round_bf16(ref['acc_f'])
  assert ref['M'] % 128, 'the last row tile of these cases is ragged'
  out = good.copy()
  out[ref['M'] - 1] = CR.FILL_BF16
  with pytest.raises(AssertionError):
    CR.exact('row left unwritten', out, good)
  part = np.stack([CR.stats(good[:128]), np.full((2, good.shape[1]), CR.FILL_F32)])        # the second partial never written
  with pytest.raises(AssertionError):
    CR.exact_partials('partial left unwritten', part, CR.stats(good))


@pytest.mark.parametrize('shape', SENSITIVE, ids=_id)
@pytest.mark.parametrize('fill', [CR.FILL_BF16, 0.0], ids=['keeps-the-pattern', 'written-as-zeros'])
def test_one_pad_column_written_fails(shape, fill):
  ref = CR.conv_reference(shape)
  good = CR.round_bf16(ref['acc_f'])
  out = np.full((ref['M'], good.shape[1] + 8), fill)
  out[:, :good.shape[1]] = good
  CR.exact_rows('undamaged', out, good, fill)
  out[ref['M'] // 2, good.shape[1] + 3] = good[0, 0]
  with pytest.raises(AssertionError):
    CR.exact_rows('pad column written', out, good, fill)
