"""Edge shapes, ties and guard bands of the row, loss, metric, DropBlock and bookkeeping kernels (csrc/extra.hip, the row
metrics of csrc/eval.hip, the row and element kernels of csrc/misc.hip, the partial-sum kernels of csrc/bn.hip) against the
plain float64 references of tests/rows_ref.py, which tests/test_rows_ref_cpu.py proves against the oracle on the CPU.

Rules of every case:
* element-wise bounds, never a norm.  bf16 outputs: |out - ref| <= 2^-8 |ref| + 4 * floor -- one bf16 ulp (half for the
  rounding, half for float32 accumulation) plus four times the case's reference floor (rows_ref.floor_of: the float64
  reference against its own float32 evaluation; measured on the reference, never on the kernel).  float32 sums of n terms:
  n 2^-24 sum |terms|.  float32 outputs through __expf / __logf / powf: the 1e-4 relative bound of
  test_eval_metric_kernels (torch.allclose(rtol=1e-4): |out - ref| <= 1e-4 |ref| + 1e-8).  0/1 outputs, casts and data
  movement: equal bits.
* every output is a slice of a larger tensor with 4 KiB of the byte 0xA5 on either side, which must survive the call; the
  output itself starts as 0xA5 too, so an element the kernel skips shows.  Padding columns of inputs with a leading dimension
  hold NaN or 1e30, and no output may hold a NaN or a huge value.
* ``-s`` prints the worst error of every case next to its bound (profiles/rows_edges_tolerances.md records the worst of each
  kernel family).
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import rows_ref as R
from tests.gpu_guard import (_ALIVE, BF, DEV, FLANK, PATTERN, Out, _abi, _release_inputs, _report, call,  # noqa: F401
                             close_bf16, close_rel, close_sum, close_terms, close_ulp, dev, exact, ptr)

pytestmark = pytest.mark.gpu


def padded(a, ld, fill):
  """[rows, C] -> [rows, ld] with the padding columns holding ``fill``"""
  out = np.full((a.shape[0], ld), fill, a.dtype)
  out[:, :a.shape[1]] = a
  return out


# ---- bias gradient / bias add ---------------------------------------------------------------------------------------------
def _bias_grad_in_kernel_order(dz):
  """bias_grad_kernel's documented, fixed summation order in float32: 8 row lanes, four chains per lane over rows
  m, m + 8, m + 16, m + 24 while m + 24 < M, the rest on the first chain, (s0 + s1) + (s2 + s3), then lanes 0 .. 7 in order.
  This is a REPLICA of the kernel's order, not a property of the operation: the kernel's comment promises only that the order
  is fixed.  It is here because a wrong trip condition of the four-chain loop (m + 32 < M) still sums every row, through the
  tail loop, and only the rounding tells.  Whoever re-orders the kernel's sum on purpose updates this replica with it; a
  mismatch alone is no reason to change the kernel."""
  M, C = dz.shape
  z = np.zeros(C, np.float32)
  red = []
  for ry in range(8):
    s = [z.copy() for _ in range(4)]
    m = ry
    while m + 24 < M:
      for j in range(4):
        s[j] = s[j] + dz[m + 8 * j]
      m += 32
    while m < M:
      s[0] = s[0] + dz[m]
      m += 8
    red.append((s[0] + s[1]) + (s[2] + s[3]))
  t = red[0]
  for r in range(1, 8):
    t = t + red[r]
  return t


@pytest.mark.parametrize('C,ld', [(1, 8), (10, 16), (32, 32), (33, 40), (1001, 1008)])
def test_bias_grad_row_counts(hip_lib, C, ld):
  """M below, at and above the four-chain loop's trip (rows m .. m + 24): the sum is right to M 2^-24 sum |terms|, and it is
  the kernel's documented fixed-order sum bit for bit (the comment promises a reproducible order: a row that moves from the
  four-chain loop to the tail loop changes the rounding, and this notices)"""
  for M in (1, 7, 8, 25, 32, 33, 57, 256, 300):
    dz = R.bf16_randn(R.rng(1, M, C), (M, C)) * np.float32(10.0) ** R.rng(2, M, C).integers(-2, 3, (M, 1)).astype(np.float32)
    dz = R.to_bf16(dz)
    out = Out((C,), torch.float32)
    call('asm_bias_grad_bf16', ptr(dev(padded(dz, ld, np.nan), BF)), M, C, ld, out.p)
    got = out.np()
    close_sum('bias_grad M=%d C=%d' % (M, C), got, dz.astype(np.float64).sum(0), M, np.abs(dz.astype(np.float64)).sum(0))
    exact('bias_grad order M=%d C=%d' % (M, C), got.astype(np.float32), _bias_grad_in_kernel_order(dz))


def test_bias_add_tail_and_padding(hip_lib):
  """M C = 259 is no multiple of the block: the last block's tail; ld > C: the padding columns keep their bits"""
  M, C, ld = 7, 37, 40
  r = R.rng(3)
  y0 = padded(r.standard_normal((M, C)).astype(np.float32), ld, np.float32(1e30))
  bias = r.standard_normal(C).astype(np.float32)
  y = Out((M, ld), torch.float32, init=dev(y0))
  call('asm_bias_add_f32', y.p, ptr(dev(bias)), M, C, ld)
  raw = y.t.detach().cpu().numpy()
  y.check_flanks()
  exact('bias_add', raw[:, :C], y0[:, :C] + bias[None])
  exact('bias_add padding', raw[:, C:].view(np.uint32), y0[:, C:].view(np.uint32))


# ---- sigmoid cross-entropy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [1, 5, 255, 256, 257, 1001])
def test_sigmoid_ce_shapes(hip_lib, C):
  """B on both sides of the total kernel's 256-thread stride, ld = C and ld > C (NaN padding), ld_out != ld with exactly
  zero padding, one-hot and mixed soft targets, logits at +/-80 (the stable log1p form), and the loss without a gradient"""
  for B in (1, 17, 256, 257, 600):
    for ld, ld_out, soft in ((C, C + 5, False), (C + 3, C, True), (C + 3, C + 5, False), (C, C + 8, True)):
      z, y = R.sigmoid_inputs(B, C, soft)
      loss, tot, g = R.sigmoid_ce(z, y, 4.0)
      floor = R.floor_of(lambda dt: R.sigmoid_ce(z, y, 4.0, dt)[2])
      zd, yd = dev(padded(z, ld, np.nan)), dev(y)
      rows, out, dz = Out((B, 2), torch.float32), Out((2,), torch.float32), Out((B, ld_out), BF)
      call('asm_sigmoid_ce', ptr(zd), ld, ptr(yd), B, C, 4.0, rows.p, out.p, dz.p, ld_out)
      case = 'sigmoid_ce B=%d C=%d %s' % (B, C, 'soft' if soft else 'onehot')
      o, d = out.np(), dz.np()
      rows.np()
      close_rel(case + ' loss', o[0], loss)
      if soft:
        close_sum(case + ' sum(t)', o[1], tot, B * C, np.abs(y.astype(np.float64)).sum())
      else:
        assert o[1] == B
      close_bf16(case + ' dz', d[:, :C], g, floor)
      assert (d[:, C:] == 0).all(), case + ': dz padding columns must be exactly zero'
      if not soft:          # loss only: dlogits = NULL
        out2 = Out((2,), torch.float32)
        call('asm_sigmoid_ce', ptr(zd), ld, ptr(yd), B, C, 4.0, rows.p, out2.p, None, 0)
        exact(case + ' loss only', out2.np(), o)


# ---- softmax cross-entropy, softmax, mean, one-hot ------------------------------------------------------------------------
@pytest.mark.parametrize('C', [1, 7, 255, 256, 257])
def test_softmax_ce_and_softmax_rows_shapes(hip_lib, C):
  """C below, at and above the 256-thread block (idle threads hold -inf and 0), one row and several, +1e4 on every entry of
  a row (the subtraction of the row maximum), label smoothing, and the teacher term at C = 7 and 257"""
  for B in (1, 5):
    z, y, t = R.softmax_inputs(B, C, 1e4)
    ld, ld_out = C + 3, (C + 7) // 8 * 8 + 8
    for T in ((0.0, 2.0) if C in (7, 257) else (0.0,)):
      teacher = t if T else None
      rows_ref, g = R.softmax_ce(z, y, teacher, 0.1, T, 3.0)
      floor = R.floor_of(lambda dt: R.softmax_ce(z, y, teacher, 0.1, T, 3.0, dt)[1])
      rows, dz = Out((B,), torch.float32), Out((B, ld_out), BF)
      call('asm_softmax_ce', ptr(dev(padded(z, ld, np.nan))), ld, ptr(dev(y)), ptr(dev(t)) if T else None, B, C, 0.1, T, 3.0,
           rows.p, dz.p, ld_out)
      case = 'softmax_ce B=%d C=%d%s' % (B, C, ' teacher' if T else '')
      d = dz.np()
      close_rel(case + ' loss', rows.np(), rows_ref)
      close_bf16(case + ' dz', d[:, :C], g, floor)
      assert (d[:, C:] == 0).all(), case + ': dz padding columns must be exactly zero'
    sm = Out((B, C), torch.float32)
    call('asm_softmax_rows', ptr(dev(z)), sm.p, B, C, 0.5)
    e = np.exp((z.astype(np.float64) - z.max(1, keepdims=True)) * 0.5)
    close_rel('softmax_rows B=%d C=%d' % (B, C), sm.np(), e / e.sum(1, keepdims=True))


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1000])
def test_mean_f32_lengths(hip_lib, n):
  x = (R.rng(5, n).standard_normal(n) * 3 + 1).astype(np.float32)
  out = Out((1,), torch.float32)
  call('asm_mean_f32', ptr(dev(x)), n, out.p)
  x64 = x.astype(np.float64)
  close_sum('mean_f32 n=%d' % n, out.np(), [x64.sum() / n], n, np.abs(x64 / n).sum())


@pytest.mark.parametrize('C', [1, 7, 255, 256, 257])
def test_onehot_out_of_range_labels_give_zero_rows(hip_lib, C):
  labels = np.array([-1, C, 0, C - 1, C // 2], np.int32)
  out = Out((5, C), torch.float32)
  call('asm_onehot', ptr(dev(labels, torch.int32)), out.p, 5, C)
  ref = np.zeros((5, C))
  for b, l in enumerate(labels):
    if 0 <= l < C:
      ref[b, l] = 1.0
  exact('onehot C=%d' % C, out.np(), ref)


# ---- evaluation rows ---------------------------------------------------------------------------------------------------------
def _eval_rows_case(C):
  """continuous rows, arg-max ties (the lowest index must win), the in_top_k boundary and labels outside [0, C)"""
  r = R.rng(6, C)
  rows, labels, names = [], [], []

  def add(name, z, lab):
    rows.append(z.astype(np.float32))
    labels.append(lab)
    names.append(name)

  for i in range(4):
    z = r.standard_normal(C) * 2
    add('random', z, int(r.integers(0, C)) if i else int(np.argmax(z)))
  # the maximum duplicated: two waves (300, 700), one thread's two trips (10, 266), the wave boundary (63, 64), two lanes of
  # one wave (5, 20), the row's ends (0, C - 1)
  for i, j in ((300, 700), (10, 266), (63, 64), (5, 20), (0, C - 1)):
    if i < j < C:
      for lab in (i, j):
        z = r.standard_normal(C) * 2
        z[i] = z[j] = 9.0
        add('tie (%d, %d)' % (i, j), z, lab)
  spread = [c for c in (3, 300, 600, 900, 1000, C - 1, 1, 0, 2, 4, 5, 6, 7) if c < C]
  spread = list(dict.fromkeys(spread))
  if C >= 8:
    lab, big, same = spread[0], spread[1:6], spread[6:8]
    for n_big, name in ((4, '4 larger + ties: hit'), (5, '5 larger: miss')):
      z = -1.0 - r.random(C)
      z[lab] = 1.0
      z[same] = 1.0                       # equal to the label's logit: not "larger"
      z[big[:n_big]] = 5.0 + np.arange(n_big)
      add(name, z, lab)
  elif C >= 6:
    for n_big, name in ((4, '4 larger: hit'), (5, '5 larger: miss')):
      z = np.arange(C, dtype=np.float64)
      z[0] = z[C - 1 - n_big] = C - 1 - n_big     # label 0 ties with one entry; n_big entries are larger
      add(name, z, 0)
  for lab in range(min(C, 5)) if C <= 5 else ():
    add('C <= 5: every label in range is a top-5 hit', r.standard_normal(C) * 2, lab)
  for lab in (-1, C):
    add('label %d' % lab, r.standard_normal(C) * 2, lab)
  return np.stack(rows), np.array(labels, np.int32), names


@pytest.mark.parametrize('C', [3, 5, 6, 64, 256, 257, 1001])
def test_eval_rows_ties_and_label_guard(hip_lib, C):
  z, labels, names = _eval_rows_case(C)
  B, ld = z.shape[0], C + 5
  pred_r, conf_r, top1_r, top5_r = R.eval_rows(z, labels)
  # what the references must say for the stated rows, spelled out
  for b, name in enumerate(names):
    if name.startswith('tie'):
      i, j = [int(v) for v in re.findall(r'\d+', name)]
      assert pred_r[b] == i and top1_r[b] == float(labels[b] == i)
    if 'hit' in name:
      assert top5_r[b] == 1.0
    if 'miss' in name:
      assert top5_r[b] == 0.0
    if name.startswith('label'):
      assert top1_r[b] == 0.0 and top5_r[b] == 0.0
  pred, conf, top1, top5 = Out((B,), torch.int32), Out((B,), torch.float32), Out((B,), torch.float32), Out((B,), torch.float32)
  call('asm_eval_rows', ptr(dev(padded(z, ld, np.float32(1e30)))), ld, ptr(dev(labels, torch.int32)), B, C, pred.p, conf.p,
       top1.p, top5.p)
  for b, (a, e) in enumerate(zip(pred.np(), pred_r)):
    assert a == e, 'C=%d row %d (%s): pred %d, reference %d' % (C, b, names[b], a, e)
  for what, got, ref in (('top1', top1.np(), top1_r), ('top5', top5.np(), top5_r)):
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, 'C=%d %s differs in rows %s' % (C, what, [(int(b), names[b]) for b in bad])
  close_rel('eval_rows conf C=%d' % C, conf.np(), conf_r)


@pytest.mark.parametrize('C', [3, 257])
def test_eval_rows_degenerate_rows(hip_lib, C):
  """the arg-max runs over the non-NaN logits and takes the lowest index of the largest (include/asm_hip.h): a row of -inf
  predicts class 0, -inf with a NaN at index 0 predicts class 1, and a NaN left of a finite row's maximum is passed over.
  conf of these rows is NaN by definition (exp(-inf + inf), a NaN term in the sum) and stays unasserted."""
  am = C // 2
  z = np.full((3, C), -np.inf, np.float32)
  z[1, 0] = np.nan
  z[2] = R.rng(7, C).standard_normal(C) * 2
  z[2, am], z[2, am - 1] = 9.0, np.nan
  labels = np.array([0, 1, am], np.int32)
  B, ld = 3, C + 5
  pred, conf, top1, top5 = Out((B,), torch.int32), Out((B,), torch.float32), Out((B,), torch.float32), Out((B,), torch.float32)
  call('asm_eval_rows', ptr(dev(padded(z, ld, np.float32(1e30)))), ld, ptr(dev(labels, torch.int32)), B, C, pred.p, conf.p,
       top1.p, top5.p)
  conf.check_flanks()
  top5.np()
  got = pred.np()
  exact('eval_rows degenerate pred C=%d' % C, got, [0, 1, am])
  exact('eval_rows degenerate top1 C=%d' % C, top1.np(), (got == labels).astype(np.float64))


# ---- GeM -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [3.0, 2.5])
@pytest.mark.parametrize('N,HW,C', [(1, 1, 8), (3, 49, 256), (2, 49, 264), (2, 12, 1000), (2, 9, 24)])
def test_gem_shapes_and_exponents(hip_lib, N, HW, C, p):
  """C below / at / above one 256-thread block and no multiple of it, HW = 1, p as an argument; zeros and negatives in x (the
  clip), an all-negative channel (sum clamped at eps: y = HW^(-1/p) eps^(1/p), zero gradient)"""
  x, dy = R.gem_inputs(N, HW, C)
  y_r, s_r, dx_r = R.gem(x, p, dy)
  fy = R.floor_of(lambda dt: R.gem(x, p, None, dt)[0])
  fdx = R.floor_of(lambda dt: R.gem(x, p, dy, dt)[2])
  xd = dev(x, BF)
  y, ssum, dx = Out((N, C), BF), Out((N, C), torch.float32), Out((N, HW, C), BF)
  call('asm_gem_fwd', ptr(xd), y.p, ssum.p, N, HW, C, p)
  call('asm_gem_bwd', ptr(xd), ptr(dev(dy, BF)), ssum.p, dx.p, N, HW, C, p)
  case = 'gem N=%d HW=%d C=%d p=%g' % (N, HW, C, p)
  close_rel(case + ' ssum', ssum.np(), s_r)
  close_bf16(case + ' y', y.np(), y_r, fy)
  d = dx.np()
  close_bf16(case + ' dx', d, dx_r, fdx)
  assert (d[x <= 0] == 0).all() and (d[:, :, C // 2] == 0).all(), case + ': gradient through the clip / the clamped sum'


# ---- DropBlock ---------------------------------------------------------------------------------------------------------------------
def _dropblock_shapes(bs):
  return list(dict.fromkeys([(7, 7), (9, 12), (bs, bs), (bs, bs + 3)])) if bs <= 7 else []


@pytest.mark.parametrize('bs', [1, 2, 4, 6, 7])
def test_dropblock_mask_is_the_definition_bit_for_bit(hip_lib, bs):
  """odd and EVEN block sizes (the (tl, br) padding is asymmetric only for even ones), bs = 1, a 1 x 1 seed grid (H = bs),
  gamma that keeps all / some / nothing, draws EQUAL to gamma (no seed: the comparison is strict).  keep is 0/1: equal bits.
  The device-scalar form gives the same bits, and follows the scalar when it is overwritten between two identical launches."""
  for H, W in _dropblock_shapes(bs):
    for C in (8, 72):
      for kind in ('none', 'mid', 'all'):
        gamma = R.dropblock_gamma(kind, H, W, bs)
        u = R.dropblock_uniform(H, W, C, bs, gamma)
        keep_r = R.dropblock_keep(u, gamma, H, W, bs)
        ud = dev(u)
        case = 'dropblock bs=%d %dx%dx%d gamma %s' % (bs, H, W, C, kind)
        keep, scale = Out((H, W, C), torch.float32), Out((1,), torch.float32)
        call('asm_dropblock_mask', ptr(ud), float(gamma), H, W, C, bs, keep.p, scale.p)
        exact(case, keep.np(), keep_r)
        sr = float(R.dropblock_scale(keep_r))
        assert abs(float(scale.t[0]) - sr) <= 1e-6 * sr, case + ' scale'
        scale.np()
        # the recorded-step form: gamma read from device memory
        gdev = dev(np.array([gamma], np.float32))
        keep2, scale2 = Out((H, W, C), torch.float32), Out((1,), torch.float32)
        args = (ptr(ud), ptr(gdev), H, W, C, bs, keep2.p, scale2.p)
        call('asm_dropblock_mask_dev', *args)
        exact(case + ' (device scalar)', keep2.np(), keep_r)
        assert float(scale2.t[0]) == float(scale.t[0])
        g2 = np.float32(0.5) * gamma if kind != 'none' else R.dropblock_gamma('mid', H, W, bs)
        gdev.fill_(float(g2))
        call('asm_dropblock_mask_dev', *args)
        keep_r2 = R.dropblock_keep(u, g2, H, W, bs)
        exact(case + ' (device scalar rewritten)', keep2.np(), keep_r2)
        sr2 = float(R.dropblock_scale(keep_r2))
        assert abs(float(scale2.t[0]) - sr2) <= 1e-6 * sr2, case + ' scale after the rewrite'


@pytest.mark.parametrize('bs,H,W,C,kind', [(2, 9, 12, 72, 'mid'), (7, 7, 7, 8, 'mid'), (4, 4, 7, 8, 'none'), (6, 7, 7, 72, 'all'),
                                           (1, 1, 4, 8, 'mid')])
def test_dropblock_apply_forms(hip_lib, bs, H, W, C, kind):
  """y = x keep scale; relu: max(y, 0); relu_mask_from: y where the given forward output is positive, else 0"""
  N = 3
  gamma = R.dropblock_gamma(kind, H, W, bs)
  u = R.dropblock_uniform(H, W, C, bs, gamma)
  keep_r = R.dropblock_keep(u, gamma, H, W, bs)
  scale_r = float(R.dropblock_scale(keep_r))
  keep, scale = Out((H, W, C), torch.float32), Out((1,), torch.float32)
  call('asm_dropblock_mask', ptr(dev(u)), float(gamma), H, W, C, bs, keep.p, scale.p)
  r = R.rng(8, bs, H, W, C)
  x, fwd = R.bf16_randn(r, (N, H, W, C)), R.bf16_randn(r, (N, H, W, C))
  xd, fd = dev(x, BF), dev(fwd, BF)
  for name, relu, gate in (('plain', 0, None), ('relu', 1, None), ('relu_mask_from', 0, fwd)):
    ref = R.dropblock_apply(x, keep_r, scale_r, bool(relu), gate)
    floor = R.floor_of(lambda dt: R.dropblock_apply(x, keep_r, scale_r, bool(relu), gate, dt))
    y = Out((N, H, W, C), BF)
    call('asm_dropblock_apply', ptr(xd), keep.p, scale.p, ptr(fd) if gate is not None else None, relu, y.p, N, H * W * C)
    got = y.np()
    close_bf16('dropblock_apply %s bs=%d %dx%dx%d %s' % (name, bs, H, W, C, kind), got, ref, floor)
    if kind == 'none' and name == 'plain':
      exact('keep everything: y == x', got, x.astype(np.float64))
    if keep_r.max() == 0:
      assert (got == 0).all()


# ---- second trips of the capped grid-stride loops ------------------------------------------------------------------------------------
def _grid_cap():
  """the block cap of the element-wise launchers, read from the launcher itself (ew_grid in csrc/common.h)"""
  here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  src = open(os.path.join(here, 'assembled_cnn_amd', 'csrc', 'common.h')).read()
  m = re.findall(r'inline unsigned ew_grid\(size_t n\) \{.*?b < (\d+) \?.*?: (\d+)\);', src, re.S)
  assert len(m) == 1 and m[0][0] == m[0][1], 'ew_grid not found in common.h'
  return int(m[0][0])


def test_dropblock_apply_second_grid_stride_trip(hip_lib):
  """(1200, 14, 14, 72): 2,116,800 vectors of 8 > cap x 256, and 1764 vectors per image do not divide the stride, so a
  thread lands on another mask position in its second trip.  Element-wise: the whole tensor == its two halves, bit for bit,
  and a sample of images == the definition."""
  ops = _abi()
  cap = _grid_cap()
  N, H, W, C = 1200, 14, 14, 72
  nvec_img = H * W * C // 8
  assert N * nvec_img > cap * 256 >= (N // 2) * nvec_img and (cap * 256) % nvec_img != 0
  g = torch.Generator(device=DEV).manual_seed(21)
  x = torch.randn((N, H, W, C), generator=g, device=DEV).to(BF)
  fwd = torch.randn((N, H, W, C), generator=g, device=DEV).to(BF)
  gamma = R.dropblock_gamma('mid', H, W, 7)
  u = R.dropblock_uniform(H, W, C, 7, gamma)
  keep, scale = ops.dropblock_mask(dev(u), float(gamma), H, W, C, 7)
  keep_r = R.dropblock_keep(u, gamma, H, W, 7)
  exact('keep', keep.cpu().numpy(), keep_r)
  for relu, gate in ((False, None), (True, None), (False, fwd)):
    whole = Out((N, H, W, C), BF)
    call('asm_dropblock_apply', ptr(x), ptr(keep), ptr(scale), ptr(gate) if gate is not None else None, int(relu), whole.p, N,
         H * W * C)
    whole.check_flanks()
    h = N // 2
    parts = [ops.dropblock_apply(x[a:a + h], keep, scale, relu=relu, relu_mask_from=None if gate is None else gate[a:a + h])
             for a in (0, h)]
    assert torch.equal(whole.t, torch.cat(parts))
    for n in (0, 599, 600, 1188, 1189, 1199):      # both trips, and the images around the first trip's end
      ref = R.dropblock_apply(x[n:n + 1].float().cpu().numpy(), keep_r, float(R.dropblock_scale(keep_r)), relu,
                              None if gate is None else gate[n:n + 1].float().cpu().numpy())
      close_bf16('dropblock_apply 2nd trip image %d' % n, whole.t[n:n + 1].double().cpu().numpy(), ref, 0.0)


def test_elementwise_second_grid_stride_trip(hip_lib):
  """cast / widen (one element per thread) at n = cap x 256 + 5, the 8-wide kernels at the next multiple of 8 above
  cap x 256 x 8 (they refuse a ragged n): the second trip and its tail.  Equal bits against the framework's own cast,
  comparison and add on the same device, and the flanks survive."""
  cap = _grid_cap()
  n1 = cap * 256 + 5
  g = torch.Generator(device=DEV).manual_seed(22)
  x32 = torch.randn(n1, generator=g, device=DEV) * 3
  o = Out((n1,), BF)
  call('asm_cast_f32_to_bf16', ptr(x32), o.p, n1)
  assert torch.equal(o.t, x32.to(BF))
  o.np()
  w = Out((n1,), torch.float32)
  call('asm_cast_bf16_to_f32', o.p, w.p, n1)
  assert torch.equal(w.t, x32.to(BF).float())
  w.np()
  n8 = cap * 256 * 8 + 8
  a = torch.randn(n8, generator=g, device=DEV).to(BF)
  b = torch.randn(n8, generator=g, device=DEV).to(BF)
  with pytest.raises(ValueError):       # the vector kernels take whole vectors only: no ragged n + 5 for them
    call('asm_relu_fwd', ptr(a), ptr(b), n8 - 3)
  mask = torch.randint(0, 256, (n8 // 8,), generator=g, device=DEV, dtype=torch.uint8)
  zero = torch.zeros((), dtype=BF, device=DEV)
  bits = ((mask.to(torch.int32)[:, None] >> torch.arange(8, device=DEV, dtype=torch.int32)[None]) & 1).bool().view(n8)
  for name, args, ref in (('asm_add_bf16', (ptr(a), ptr(b)), (a.float() + b.float()).to(BF)),
                          ('asm_relu_fwd', (ptr(a),), torch.where(a > 0, a, zero)),
                          ('asm_relu_bwd', (ptr(a), ptr(b)), torch.where(b > 0, a, zero)),
                          ('asm_mask_apply', (ptr(a), ptr(mask)), torch.where(bits, a, zero))):
    o = Out((n8,), BF)
    call(name, *args, o.p, n8)
    assert torch.equal(o.t, ref), name
    assert bool(torch.equal(o.t[-8:], ref[-8:])), name + ': the last vector'
    o.np()


# ---- UpSampling2D backward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,Hs,Ws,C', [(1, 1, 1, 8), (2, 3, 5, 72), (2, 7, 7, 64)])
def test_upsample2x_bwd_is_the_block_sum(hip_lib, N, Hs, Ws, C):
  """plain and masked against the float64 2 x 2 block sum of dy * bit (odd low-resolution sizes included)"""
  r = R.rng(9, N, Hs, Ws, C)
  dy = R.bf16_randn(r, (N, 2 * Hs, 2 * Ws, C))
  mask = r.integers(0, 256, (N * 4 * Hs * Ws, C // 8), dtype=np.uint8)
  dyd = dev(dy, BF)
  for name, m in (('plain', None), ('masked', mask)):
    ref = R.upsample2x_bwd(dy, m)
    floor = R.floor_of(lambda dt: R.upsample2x_bwd(dy, m, dt))
    dx = Out((N, Hs, Ws, C), BF)
    if m is None:
      call('asm_upsample2x_bwd', ptr(dyd), dx.p, N, Hs, Ws, C)
    else:
      call('asm_upsample2x_bwd_masked', ptr(dyd), ptr(dev(m, torch.uint8)), dx.p, N, Hs, Ws, C)
    close_bf16('upsample2x_bwd %s %dx%dx%dx%d' % (name, N, Hs, Ws, C), dx.np(), ref, floor)


# ---- batch-norm partial sums ------------------------------------------------------------------------------------------------------------------
def _partials_on_device(p):
  """the partial rows followed by one row of 1e30 inside the same allocation: a kernel that reads one row too many says so"""
  blocks, _, C = p.shape
  buf = torch.full((blocks + 1, 2, C), 1e30, dtype=torch.float32, device=DEV)
  buf[:blocks] = dev(p)
  _ALIVE.append(buf)
  return buf


@pytest.mark.parametrize('C', [8, 24, 1008])
def test_partials_compact_known_answer(hip_lib, C):
  """every group = float32(float64 sum of its rows), 1 ulp; group sizes from one row to 1000, ragged last groups"""
  for blocks in (1, 63, 64, 65, 511, 513, 1000):
    p = R.partials(blocks, C, 1)
    buf = _partials_on_device(p)
    for groups in (1, 2, 7, 64):
      if groups > blocks or -(-blocks // -(-blocks // groups)) != groups:       # the entry point's own tiling check
        continue
      out = Out((groups, 2, C), torch.float32)
      call('asm_bn_partials_compact', ptr(buf), blocks, C, out.p, groups)
      close_ulp('compact blocks=%d groups=%d C=%d' % (blocks, groups, C), out.np(), R.compact(p, groups))
  with pytest.raises(ValueError):         # 64 groups of ceil(1000 / 64) = 16 rows: 63 of them already cover 1000 rows
    rows1000, refused = _partials_on_device(R.partials(1000, C, 1)), Out((64, 2, C), torch.float32)
    call('asm_bn_partials_compact', ptr(rows1000), 1000, C, refused.p, 64)


@pytest.mark.parametrize('C', [8, 24, 1008])
def test_bn_finalize_kernels_on_synthetic_partials(hip_lib, C):
  """asm_bn_finalize / asm_bn_bwd_finalize / asm_bn_bwd_finalize_raw called directly (ops._compact does not stand in the way)
  on partials with a known float64 answer; blocks on both sides of the 64- and 128-row steps of sum_partials.  What the
  kernel rounds once from float64 (mean, invstd, dbeta, dgamma, A, B, C) is the float32 next to the float64 reference, 1 ulp.
  What it evaluates in float32 from those rounded values is allowed the roundings of that expression, each half an ulp of
  the terms' magnitudes: scale = gamma * invstd (invstd's ulp = 2, the product 1 -> 3), shift = beta - mean * scale (mean 1,
  scale 3, product 1, difference 1 -> 6), the moving statistics old * momentum + new * (1 - momentum) (new 1, two products,
  the sum -> 4; the Bessel factor M / (M - 1) is in ``new`` of the variance)."""
  r = R.rng(10, C)
  gamma = r.uniform(0.5, 1.5, C).astype(np.float32)
  beta = r.standard_normal(C).astype(np.float32)
  mm0 = r.standard_normal(C).astype(np.float32)
  mv0 = r.uniform(0.5, 1.5, C).astype(np.float32)
  mean_in = r.standard_normal(C).astype(np.float32)
  invstd_in = r.uniform(0.3, 3.0, C).astype(np.float32)
  gd, bd, md, isd = dev(gamma), dev(beta), dev(mean_in), dev(invstd_in)
  for blocks in (1, 2, 64, 65, 128, 129, 200, 1024):
    M = 8 * blocks + 3
    p = R.partials(blocks, C, 2, positive_second=True)
    ref = R.bn_finalize(p, M, gamma, beta, 1e-5, 0.9, mm0, mv0)
    assert (p[:, 1].astype(np.float64).sum(0) / M - ref['mean'] ** 2 > 1.0).all()      # a variance well away from the clamp
    o = {k: Out((C,), torch.float32) for k in ('mean', 'invstd', 'scale', 'shift')}
    mm, mv = Out((C,), torch.float32, init=dev(mm0)), Out((C,), torch.float32, init=dev(mv0))
    call('asm_bn_finalize', ptr(_partials_on_device(p)), blocks, M, C, ptr(gd), ptr(bd), 1e-5, 0.9, mm.p, mv.p, o['mean'].p,
         o['invstd'].p, o['scale'].p, o['shift'].p)
    case = 'bn_finalize blocks=%d C=%d ' % (blocks, C)
    close_ulp(case + 'mean', o['mean'].np(), ref['mean'])
    close_ulp(case + 'invstd', o['invstd'].np(), ref['invstd'])
    close_terms(case + 'scale', o['scale'].np(), (ref['scale'],), 3)
    close_terms(case + 'shift', o['shift'].np(), (beta.astype(np.float64), -ref['mean'] * ref['scale']), 6)
    close_terms(case + 'moving_mean', mm.np(), ref['mm_terms'], 4)
    close_terms(case + 'moving_var', mv.np(), ref['mv_terms'], 4)
    # without moving statistics: same outputs, nothing else touched
    o2 = {k: Out((C,), torch.float32) for k in ('mean', 'invstd', 'scale', 'shift')}
    call('asm_bn_finalize', ptr(_partials_on_device(p)), blocks, M, C, ptr(gd), ptr(bd), 1e-5, 0.9, None, None, o2['mean'].p,
         o2['invstd'].p, o2['scale'].p, o2['shift'].p)
    for k in o:
      exact(case + k + ' (no moving statistics)', o2[k].np(), o[k].np())
    pb = R.partials(blocks, C, 3)
    for fn, raw in (('asm_bn_bwd_finalize', False), ('asm_bn_bwd_finalize_raw', True)):
      refb = R.bn_bwd_finalize(pb, M, gamma, mean_in, invstd_in, raw=raw)
      ob = {k: Out((C,), torch.float32) for k in ('dgamma', 'dbeta', 'A', 'B', 'C')}
      call(fn, ptr(_partials_on_device(pb)), blocks, M, C, ptr(gd), ptr(md), ptr(isd), ob['dgamma'].p, ob['dbeta'].p,
           ob['A'].p, ob['B'].p, ob['C'].p)
      for k in ('dbeta', 'dgamma', 'A', 'B', 'C'):
        close_ulp('%s blocks=%d C=%d %s' % (fn[4:], blocks, C, k), ob[k].np(), refb[k])


# ---- data movement: equal bits ------------------------------------------------------------------------------------------------------------------
def test_filter_transpose_tiled_and_batched_equal_the_permutation(hip_lib):
  """the tiled form (the one nn.py calls) and the element form on one table that mixes a K < 64 layer, a 3 x 3 one, the
  classifier (K = 1001 in rows of 1008: columns 1001 .. 1007 zero filled by the tiled form) and an 8-channel 7 x 7 one"""
  layers = [(24, 1, 1, 40, 24), (64, 3, 3, 64, 64), (1001, 1, 1, 2048, 1008), (8, 7, 7, 8, 8)]
  r = R.rng(12)
  ws = [R.bf16_randn(r, (K, Rr, S, C)) for K, Rr, S, C, _ in layers]
  table, src_off, dst_off, elems, tiles = [], 0, 0, 0, 0
  for (K, Rr, S, C, ldk) in layers:
    table.append([src_off, dst_off, K, Rr * S, C, ldk, elems, tiles])
    src_off += K * Rr * S * C
    elems += K * Rr * S * C
    dst_off += C * Rr * S * ldk
    tiles += Rr * S * -(-K // 64) * -(-C // 64)
  src = dev(np.concatenate([w.reshape(-1) for w in ws]), BF)
  ref = np.concatenate([R.filter_transpose(w, l[4]).reshape(-1) for w, l in zip(ws, layers)]).astype(np.float64)
  tab = dev(np.array(table, np.int32), torch.int32)
  tiled = Out((dst_off,), BF)
  call('asm_filter_transpose_tiled', ptr(src), tiled.p, ptr(tab), len(layers), tiles)
  exact('filter_transpose_tiled', tiled.np(), ref)
  batched = Out((dst_off,), BF)
  batched.t.zero_()                 # the element form leaves the padding columns alone
  ops = _abi()
  ops.check(ops.L().asm_filter_transpose_batched(ptr(src), batched.p, ptr(tab), len(layers), elems, ops._stream()),
            'filter_transpose_batched')
  exact('filter_transpose_batched', batched.np(), ref)
  assert torch.equal(tiled.t, batched.t)


@pytest.mark.parametrize('K', [8, 32, 64])
@pytest.mark.parametrize('ksize', [3, 7])
def test_stem_pack_and_unpack_index_maps(hip_lib, ksize, K):
  """[K][k][k][3] float32 -> bf16 [K][k][L] at lane s * 4 + c with every other lane exactly zero, and the gradient's way back;
  any other ksize is refused"""
  r = R.rng(14, ksize, K)
  L = R.stem_lanes(ksize)
  w = r.standard_normal((K, ksize, ksize, 3)).astype(np.float32)
  wp = Out((K, ksize, L), BF)
  call('asm_stem_pack_filter', ptr(dev(w)), wp.p, K, ksize)
  exact('stem_pack ksize=%d K=%d' % (ksize, K), wp.np(), R.stem_pack(w).astype(np.float64))
  dwp = np.full((K, ksize, L), 1e30, np.float32)            # lanes the unpack must never read
  vals = r.standard_normal((K, ksize, ksize, 3)).astype(np.float32)
  for s in range(ksize):
    dwp[:, :, s * 4:s * 4 + 3] = vals[:, :, s]
  dw = Out((K, ksize, ksize, 3), torch.float32)
  call('asm_stem_unpack_grad', ptr(dev(dwp)), dw.p, K, ksize)
  exact('stem_unpack ksize=%d K=%d' % (ksize, K), dw.np(), R.stem_unpack(dwp, ksize).astype(np.float64))
  exact('stem_unpack values', dw.np(), vals.astype(np.float64))
  for bad in (1, 5):
    with pytest.raises(ValueError):
      call('asm_stem_pack_filter', ptr(dev(w)), wp.p, K, bad)
