"""Plain references of the pooling, SK and SE kernels (csrc/pool.hip, csrc/sk_se.hip, csrc/sk_fused.hip), written from the
definitions the kernel comments quote: tf.layers.max_pooling2d / average_pooling2d with TF's SAME rule, nets/blocks.py:45-107
(anti-aliased downsample: REFLECT pad, binomial filter), nets/blocks.py:110-154 (selective kernel), nets/blocks.py:156-184
(squeeze-excite) and the batch-norm backward.  numpy on the CPU, NHWC in and NHWC out ([N, HW, C] where the kernel sees rows),
float64 unless ``dtype`` says otherwise; nothing here calls the product or tests/cpu_double.py.
tests/test_pool_ref_cpu.py checks every function against oracle/assembled_oracle.py and its autograd;
tests/test_gpu_pool_edges.py checks the HIP kernels against them.

Every reference takes ``dtype`` so that ``rows_ref.floor_of`` can measure its float32 floor (see tests/rows_ref.py).
"""
from __future__ import annotations

import numpy as np

from tests.rows_ref import F32, F64, to_bf16

BINOMIAL = {2: [1, 1], 3: [1, 2, 1], 4: [1, 3, 3, 1], 5: [1, 4, 6, 4, 1], 6: [1, 5, 10, 10, 5, 1],
            7: [1, 6, 15, 20, 15, 6, 1]}


# ---- window geometry ----------------------------------------------------------------------------------------------------
def same_pad(size, k, s):
  """TF SAME: out = ceil(in / s); pad_total = max((out - 1) s + k - in, 0); before = total // 2  -> (out, before)"""
  out = -(-size // s)
  return out, max((out - 1) * s + k - size, 0) // 2


def avgpool_geometry(size, k, stride, count_valid):
  """the two ways the network pools on average -> (out, pad before).  count_valid: SAME, the divisor counts the taps inside
  the map.  Otherwise model_helper.fixed_padding (k - 1 zeros, (k - 1) // 2 of them before) and a VALID pool, divisor k k."""
  if count_valid:
    return same_pad(size, k, stride)
  return (size + (k - 1) - k) // stride + 1, (k - 1) // 2


def _taps(out, size, stride, pad, r):
  """tap r of every window along one axis -> (output positions whose tap lies inside the map, the input positions they read)"""
  o = np.arange(out)
  i = o * stride + r - pad
  ok = (i >= 0) & (i < size)
  return o[ok], i[ok]


# ---- max pool 3x3 / 2, SAME ---------------------------------------------------------------------------------------------
def maxpool3x3s2(x, dtype=F64):
  """-> (y [N, Ho, Wo, C], code [N, Ho, Wo, C]): code = r * 3 + s of the FIRST maximum in (r, s) scan order among the taps
  inside the map (what tf.nn.max_pool's gradient and torch's max_pool2d pick: a later tap wins only if strictly larger)"""
  x = np.asarray(x, dtype)
  N, H, W, C = x.shape
  (Ho, ph), (Wo, pw) = same_pad(H, 3, 2), same_pad(W, 3, 2)
  best = np.full((N, Ho, Wo, C), -np.inf, dtype)
  code = np.zeros((N, Ho, Wo, C), np.int64)
  for r in range(3):
    oh, ih = _taps(Ho, H, 2, ph, r)
    for s in range(3):
      ow, iw = _taps(Wo, W, 2, pw, s)
      if not oh.size or not ow.size:
        continue
      tap = x[:, ih][:, :, iw]
      cur = best[:, oh][:, :, ow]
      win = tap > cur
      best[np.ix_(np.arange(N), oh, ow)] = np.where(win, tap, cur)
      code[np.ix_(np.arange(N), oh, ow)] = np.where(win, r * 3 + s, code[:, oh][:, :, ow])
  return best, code


def maxpool3x3s2_bwd(dy, code, shape, dtype=F64):
  """the scatter of dy to the coded tap -> dx [N, H, W, C]"""
  dy = np.asarray(dy, dtype)
  N, H, W, C = shape
  (Ho, ph), (Wo, pw) = same_pad(H, 3, 2), same_pad(W, 3, 2)
  dx = np.zeros(shape, dtype)
  for r in range(3):
    oh, ih = _taps(Ho, H, 2, ph, r)
    for s in range(3):
      ow, iw = _taps(Wo, W, 2, pw, s)
      if not oh.size or not ow.size:
        continue
      g = np.where(code == r * 3 + s, dy, dtype(0))[:, oh][:, :, ow]
      dx[np.ix_(np.arange(N), ih, iw)] += g       # one tap: distinct windows read distinct pixels
  return dx


# ---- average pool -------------------------------------------------------------------------------------------------------
def _avg_divisor(H, W, k, stride, pad, Ho, Wo, count_valid, dtype):
  ch, cw = np.zeros(Ho, np.int64), np.zeros(Wo, np.int64)
  for r in range(k):
    ch[_taps(Ho, H, stride, pad, r)[0]] += 1
    cw[_taps(Wo, W, stride, pad, r)[0]] += 1
  div = ch[:, None] * cw[None, :] if count_valid else np.full((Ho, Wo), k * k, np.int64)
  return div.astype(dtype)[None, :, :, None]


def avgpool(x, k, stride, pad, Ho, Wo, count_valid, dtype=F64):
  """zero pad ``pad`` before (and whatever Ho, Wo need after); divisor k k, or the number of taps inside the map"""
  x = np.asarray(x, dtype)
  N, H, W, C = x.shape
  acc = np.zeros((N, Ho, Wo, C), dtype)
  for r in range(k):
    oh, ih = _taps(Ho, H, stride, pad, r)
    for s in range(k):
      ow, iw = _taps(Wo, W, stride, pad, s)
      if oh.size and ow.size:
        acc[np.ix_(np.arange(N), oh, ow)] += x[:, ih][:, :, iw]
  return acc / _avg_divisor(H, W, k, stride, pad, Ho, Wo, count_valid, dtype)


def avgpool_bwd(dy, shape, k, stride, pad, count_valid, addend=None, dtype=F64):
  """the adjoint of ``avgpool`` (+ addend) -> dx [N, H, W, C]"""
  dy = np.asarray(dy, dtype)
  N, H, W, C = shape
  Ho, Wo = dy.shape[1:3]
  g = dy / _avg_divisor(H, W, k, stride, pad, Ho, Wo, count_valid, dtype)
  dx = np.zeros(shape, dtype)
  for r in range(k):
    oh, ih = _taps(Ho, H, stride, pad, r)
    for s in range(k):
      ow, iw = _taps(Wo, W, stride, pad, s)
      if oh.size and ow.size:
        dx[np.ix_(np.arange(N), ih, iw)] += g[:, oh][:, :, ow]
  return dx if addend is None else dx + np.asarray(addend, dtype)


# ---- blur pool ------------------------------------------------------------------------------------------------------------
def blur_out(size, k, stride):
  return (size + 2 * ((k - 1) // 2) - k) // stride + 1


def _blur_row(k, dtype):
  a = np.asarray(BINOMIAL[k], dtype)
  return a / a.sum(dtype=dtype)


def blurpool(x, k, stride, dtype=F64):
  """nets/blocks.py:45-107: REFLECT pad (k - 1) // 2 on both sides, the k x k outer product of the normalised binomial row,
  stride, VALID"""
  x = np.asarray(x, dtype)
  N, H, W, C = x.shape
  p = (k - 1) // 2
  xp = np.pad(x, ((0, 0), (p, p), (p, p), (0, 0)), mode='reflect') if p else x
  Ho, Wo = blur_out(H, k, stride), blur_out(W, k, stride)
  a = _blur_row(k, dtype)
  y = np.zeros((N, Ho, Wo, C), dtype)
  for r in range(k):
    for s in range(k):
      y += (a[r] * a[s]) * xp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride]
  return y


def blurpool_bwd(dy, shape, k, stride, dtype=F64):
  """the adjoint of ``blurpool``: the gradient of the padded map, then every padded position folded onto the pixel the
  REFLECT pad copied it from"""
  dy = np.asarray(dy, dtype)
  N, H, W, C = shape
  p = (k - 1) // 2
  Ho, Wo = dy.shape[1:3]
  a = _blur_row(k, dtype)
  gp = np.zeros((N, H + 2 * p, W + 2 * p, C), dtype)
  for r in range(k):
    for s in range(k):
      gp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride] += (a[r] * a[s]) * dy
  src_h = np.pad(np.arange(H), p, mode='reflect') if p else np.arange(H)
  src_w = np.pad(np.arange(W), p, mode='reflect') if p else np.arange(W)
  dx = np.zeros(shape, dtype)
  np.add.at(dx, (slice(None), src_h[:, None], src_w[None, :]), gp)
  return dx


# ---- global average pool --------------------------------------------------------------------------------------------------
def gap(x, dtype=F64):
  """[N, HW, C] -> mean over HW [N, C]"""
  x = np.asarray(x, dtype)
  return x.sum(axis=1, dtype=dtype) / dtype(x.shape[1])


def gap_bwd(dy, shape, dtype=F64):
  """[N, C] -> dy / HW on every row [N, HW, C]"""
  N, HW, C = shape
  return np.broadcast_to((np.asarray(dy, dtype) / dtype(HW))[:, None, :], shape).copy()


def sk_gap(f, F, dtype=F64):
  """nets/blocks.py:131-134 on f [N, HW, 2F]: mean over HW of f0 + f1 -> [N, F]"""
  f = np.asarray(f, dtype)
  return (f[:, :, :F] + f[:, :, F:]).sum(axis=1, dtype=dtype) / dtype(f.shape[1])


def mean_of_exact_sum(total, count):
  """the kernels' last step, o = t * (1.0f / count), on a sum t that float32 holds exactly (grid inputs): two float32
  roundings, stated by the kernels (gap_fwd_kernel, sk_gap_bn_kernel), on top of an order-free sum"""
  t = np.asarray(total, F64).astype(F32)
  assert (t.astype(F64) == np.asarray(total, F64)).all(), 'the sum is not exact in float32'
  return t * (F32(1.0) / F32(count))


# ---- selective kernel: V = a0 f0 + a1 f1, a = softmax over the two branches -------------------------------------------------
def sk_gates(att, F, dtype=F64):
  """att [N, 2F] logits -> (a0, a1) [N, F], the softmax over the two branches (nets/blocks.py:150-151)"""
  att = np.asarray(att, dtype)
  l0, l1 = att[:, :F], att[:, F:]
  m = np.maximum(l0, l1)
  e0, e1 = np.exp(l0 - m), np.exp(l1 - m)
  return e0 / (e0 + e1), e1 / (e0 + e1)


def sk_select(f, att, dtype=F64):
  """f [N, HW, 2F], att [N, 2F] -> V [N, HW, F]"""
  f = np.asarray(f, dtype)
  F = f.shape[2] // 2
  a0, a1 = sk_gates(att, F, dtype)
  return a0[:, None] * f[:, :, :F] + a1[:, None] * f[:, :, F:]


def sk_select_bwd_att(f, dv, att, dtype=F64):
  """-> datt [N, 2F]: the softmax backward of da_b = sum_hw f_b dV, i.e. a0 a1 (da0 - da1) and its negative"""
  f, dv = np.asarray(f, dtype), np.asarray(dv, dtype)
  F = f.shape[2] // 2
  a0, a1 = sk_gates(att, F, dtype)
  da0 = (f[:, :, :F] * dv).sum(axis=1, dtype=dtype)
  da1 = (f[:, :, F:] * dv).sum(axis=1, dtype=dtype)
  d0 = a0 * a1 * (da0 - da1)
  return np.concatenate([d0, -d0], axis=1)


def sk_select_bwd_f(dv, att, ds, dtype=F64):
  """dV [N, HW, F], ds [N, F] (gradient of the pooled mean) -> df [N, HW, 2F] = a_b dV + ds / HW"""
  dv, ds = np.asarray(dv, dtype), np.asarray(ds, dtype)
  HW, F = dv.shape[1:]
  a0, a1 = sk_gates(att, F, dtype)
  u = (ds / dtype(HW))[:, None]
  return np.concatenate([a0[:, None] * dv + u, a1[:, None] * dv + u], axis=2)


# ---- squeeze-excite: y = x sigmoid(e) ----------------------------------------------------------------------------------------
def sigmoid(e, dtype=F64):
  e = np.asarray(e, dtype)
  z = np.exp(-np.abs(e))
  return np.where(e >= 0, 1 / (1 + z), z / (1 + z))


def se_scale(x, e, dtype=F64):
  """x [N, HW, C], e [N, C] -> y"""
  return np.asarray(x, dtype) * sigmoid(e, dtype)[:, None]


def se_scale_bwd_e(x, dy, e, dtype=F64):
  """-> de [N, C] = s (1 - s) sum_hw x dy"""
  s = sigmoid(e, dtype)
  return (np.asarray(x, dtype) * np.asarray(dy, dtype)).sum(axis=1, dtype=dtype) * s * (1 - s)


def se_scale_bwd_x(dy, e, dsq, dtype=F64):
  """dy [N, HW, C], dsq [N, C] (gradient of the squeezed mean) -> dx = dy s + dsq / HW"""
  dy = np.asarray(dy, dtype)
  return dy * sigmoid(e, dtype)[:, None] + (np.asarray(dsq, dtype) / dtype(dy.shape[1]))[:, None]


# ---- the SK unit with its batch norm and ReLU applied on the fly (csrc/sk_fused.hip) -----------------------------------------
def sk_fused_f(y, scale, shift, dtype=F64):
  """y [N, HW, 2F] -> (f = bf16(relu(y scale + shift)), mask = [y scale + shift > 0])"""
  t = np.asarray(y, dtype) * np.asarray(scale, dtype) + np.asarray(shift, dtype)
  return to_bf16(np.maximum(t, 0).astype(F32)).astype(dtype), t > 0


def sk_fused_fwd(y, scale, shift, att, dtype=F64):
  """-> (s [N, F] pooled mean of f0 + f1, V [N, HW, F], mask statistics [N, 2, 2F]: sum_hw [t > 0] and sum_hw [t > 0] y)"""
  y = np.asarray(y, dtype)
  F = y.shape[2] // 2
  f, m = sk_fused_f(y, scale, shift, dtype)
  stats = np.stack([m.astype(dtype).sum(axis=1, dtype=dtype), np.where(m, y, dtype(0)).sum(axis=1, dtype=dtype)], axis=1)
  return sk_gap(f, F, dtype), sk_select(f, att, dtype), stats


def sk_fused_bwd(y, scale, shift, gamma, mean, invstd, att, dv, ds, dtype=F64):
  """the backward half: datt from f and dV; df = a_b dV + ds / HW NOT rounded to bf16 (header of csrc/sk_fused.hip);
  dz = df [t > 0]; xhat = (y - mean) invstd; dbeta = sum dz; dgamma = sum dz xhat;
  dy = gamma invstd (dz - dbeta / M - xhat dgamma / M), M = N HW.
  -> dict(datt [N, 2F], gstats [N, 2, 2F] (sum_hw [t > 0] dV, sum_hw [t > 0] dV y), dz, xhat, dbeta, dgamma, dy)"""
  y, dv = np.asarray(y, dtype), np.asarray(dv, dtype)
  N, HW, C2 = y.shape
  F = C2 // 2
  f, m = sk_fused_f(y, scale, shift, dtype)
  dv2 = np.concatenate([dv, dv], axis=2)
  mg = np.where(m, dv2, dtype(0))
  gstats = np.stack([mg.sum(axis=1, dtype=dtype), (mg * y).sum(axis=1, dtype=dtype)], axis=1)
  dz = np.where(m, sk_select_bwd_f(dv, att, ds, dtype), dtype(0))
  xhat = (y - np.asarray(mean, dtype)) * np.asarray(invstd, dtype)
  dbeta = dz.sum(axis=(0, 1), dtype=dtype)
  dgamma = (dz * xhat).sum(axis=(0, 1), dtype=dtype)
  M = dtype(N * HW)
  dy = np.asarray(gamma, dtype) * np.asarray(invstd, dtype) * (dz - dbeta / M - xhat * (dgamma / M))
  return dict(datt=sk_select_bwd_att(f, dv, att, dtype), gstats=gstats, dz=dz, xhat=xhat, dbeta=dbeta, dgamma=dgamma, dy=dy)


# ---- cases and inputs shared by the CPU proof and the GPU module -----------------------------------------------------------------
MAXPOOL_SHAPES = [(2, 1, 1, 8), (1, 2, 3, 8), (2, 5, 4, 16), (1, 9, 8, 24), (2, 8, 9, 8), (2, 15, 17, 16)]
AVG_FORMS = [(3, 2, 1, 0), (2, 2, 0, 0), (2, 1, 0, 1)]       # (k, stride, pad, count_valid): the three forms of the network
AVG_SHAPES = [(2, 5, 8, 8), (1, 6, 3, 16), (2, 7, 4, 8), (1, 8, 5, 24)]
ALL_K = (2, 3, 4, 5, 6, 7)
BLUR_CASES = [((1, 4, 4, 8), (7,)),          # pad 3 = H - 1: both reflections reach rows 1 and 2
              ((1, 3, 3, 8), (5,)),          # three sources per axis for the middle pixel
              ((1, 2, 2, 8), (3,)), ((1, 2, 4, 8), (3,)),      # H = 2: the generic backward kernel at k = 3, stride 2
              ((2, 5, 4, 8), ALL_K), ((1, 6, 7, 16), ALL_K),
              ((1, 4, 4, 8), (3,)), ((2, 6, 4, 8), (3,)), ((1, 4, 8, 24), (3,))]    # stride 2: blur3s2_bwd_kernel


def fused_rows(Fh):
  """HW at 1, 3 and around 4 rpb (the floor of rows_per_chunk: one chunk, exactly one chunk, a second chunk of one row) and
  one row past the second chunk, for the backward passes (rpb = 256 // (2F / 8)) and the forward select (256 // (F / 8))"""
  rows = {1, 3}
  for rpb in (256 // (2 * Fh // 8), 256 // (Fh // 8)):
    rows |= {4 * rpb - 1, 4 * rpb, 4 * rpb + 1, 8 * rpb + 1}
  return sorted(rows)


FUSED_CASES = [(N, HW, Fh) for Fh in (8, 24, 40, 1024) for N in (1, 3) for HW in fused_rows(Fh)] + [(1025, 3, 8)]


def grid(r, shape, relu=False):
  """values j / 8 with |j| <= 32, exact in bf16; ``relu``: drawn from an upstream ReLU (clamped at 0, so zeros tie)"""
  x = r.integers(-32, 33, shape).astype(F32) / F32(8)
  return np.maximum(x, F32(0)) if relu else x


def fused_grid_inputs(r, N, HW, F):
  """inputs of the fused SK kernels on which every intermediate is exact: y on the 1/8 grid, scale a power of two, shift a
  multiple of 1/16 chosen as -scale y0 with y0 on the grid, and y == y0 planted on every fifth row, so that
  t = y scale + shift is exactly 0 on a fifth of the elements (more by chance); gate logits whose differences are 0 or
  +-100, i.e. gates of exactly 1/2, 0 and 1  -> (y [N, HW, 2F], scale, shift [2F], att [N, 2F])"""
  y = grid(r, (N, HW, 2 * F))
  scale = (F32(2.0) ** r.integers(-1, 2, 2 * F)).astype(F32)
  y0 = grid(r, (2 * F,))
  y[:, ::5, :] = y0
  shift = (-scale * y0).astype(F32)
  att = np.zeros((N, 2 * F), F32)
  att[:, :F] = r.integers(-4, 5, (N, F)).astype(F32)
  att[:, F:] = att[:, :F] + np.asarray([0.0, 100.0, -100.0, 0.0], F32)[r.integers(0, 4, (N, F))]
  return y, scale, shift, att


def fused_random_inputs(r, N, HW, F):
  """bf16 random y with a per-channel offset and spread, batch statistics of it, random affine parameters and gates
  -> dict(y, gamma, beta, mean, invstd, scale, shift (float32, derived in float64), att, dv, ds)"""
  C2 = 2 * F
  y = to_bf16(r.standard_normal((N, HW, C2)) * r.uniform(0.5, 2.0, C2) + r.uniform(-0.5, 0.5, C2))
  gamma = r.uniform(0.5, 1.5, C2).astype(F32)
  beta = r.uniform(-0.5, 0.5, C2).astype(F32)
  mean = y.astype(F64).mean(axis=(0, 1))
  var = ((y.astype(F64) - mean) ** 2).mean(axis=(0, 1))
  invstd = 1.0 / np.sqrt(var + 1e-5)
  mean, invstd = mean.astype(F32), invstd.astype(F32)
  scale = (gamma.astype(F64) * invstd).astype(F32)
  shift = (beta.astype(F64) - mean.astype(F64) * scale).astype(F32)
  att = (r.standard_normal((N, C2)) * 2).astype(F32)
  dv = to_bf16(r.standard_normal((N, HW, F)))
  ds = to_bf16(r.standard_normal((N, F)))
  return dict(y=y, gamma=gamma, beta=beta, mean=mean, invstd=invstd, scale=scale, shift=shift, att=att, dv=dv, ds=ds)


def sk_logits(r, N, Fh):
  """gate logits whose differences l1 - l0 are 0, +-30 and +-100 on the first channels and random elsewhere"""
  att = (r.standard_normal((N, 2 * Fh)) * 2).astype(F32)
  planted = np.asarray([0.0, 30.0, -30.0, 100.0, -100.0], F32)
  n = min(Fh, 5)
  att[:, Fh:Fh + n] = att[:, :n] + planted[:n]
  if Fh >= 8:
    att[:, Fh + 3:Fh + 8] = att[:, 3:8] + planted
  return att


def se_logits(r, N, C):
  e = (r.standard_normal((N, C)) * 2).astype(F32)
  e[:, 0::7] = 100.0
  e[:, 3::7] = -100.0
  return e
