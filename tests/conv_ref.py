"""Exact references and case tables of the convolution kernels (csrc/conv_igemm.hip, conv_gemm1.hip, conv_igemm8.hip,
conv_dgrad_s2.hip, conv_wgrad.hip, dense_small.hip): forward, input gradient and weight gradient straight from the descriptor
(include/asm_hip.h: out(n, ho, wo, k) = sum_{r,s,c} x(n, ho stride + r - pad, wo stride + s - pad, c) w(k, r, s, c) over an input
addressed by three element pitches), one plain loop over the taps, plus the epilogues the kernels fuse.  numpy on the CPU; nothing
here calls the product or the oracle.  tests/test_conv_ref_cpu.py proves the functions against torch.nn.functional.conv2d, its
autograd and the oracle, and the conditions below for every case; tests/test_gpu_conv_exact.py checks the HIP kernels.

Why the comparison needs no tolerance.  The kernels multiply bf16 operands and accumulate in fp32.  With the small integer
operands generated here every product and every partial sum is an integer below 2^24, so the fp32 accumulator holds the exact
integer whatever the tile, chunk, tap, split or slab order, and a bf16 output is that integer rounded once to nearest-even
(f2bf, csrc/common.h): every integer up to 256 and every even one up to 512 survives.  No operand is zero, so one dropped, doubled
or misplaced product moves an integer sum by at least 1.  float64 holds all of it exactly, which is what the references use.

Conditions the tables meet (asserted on the CPU for every case, never measured on the GPU):
  1. 2 L < 2^24 for the forward (L = R S C) and the input gradient (L = R S K); 6 M < 2^24 for the weight gradient (M pixels);
  2. at most 1 % of a case's exact sums exceed 256 in magnitude (there a +-1 error could round away);
  3. where fused statistics or batch-norm backward sums are checked (L <= 1152 only) no exact sum exceeds 256: the sums of the
     fp32 accumulators and of the bf16 outputs are then the same numbers and every 128-row partial is an exact integer
     (sum y^2 <= 128 2^16 < 2^24).
"""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np

from tests import pool_ref as P
from tests import rows_ref as R
from tests.gpu_guard import exact

F64 = np.float64
STATS_BM = 128        # rows per statistics partial (asm_conv2d_stats_blocks)
STATS_L = 1152        # longest reduction whose fused sums are checked (condition 3)

# what an element nobody wrote reads as: the guard pattern 0xA5 of tests/gpu_guard.py in both output types
FILL_BF16 = float(np.array([0xA5A50000], np.uint32).view(np.float32)[0])
FILL_F32 = float(np.array([0xA5A5A5A5], np.uint32).view(np.float32)[0])


# ---- descriptor ---------------------------------------------------------------------------------------------------------
class Desc(object):
  """the fields of asm_conv_desc; ops.make_conv_desc's rules (pad (R - 1) // 2 before, SAME / fixed-padding output size)"""

  def __init__(self, N, H, W, C, K, R, S, stride, pad=None, Ho=None, Wo=None, ldy=0, img_pitch=0, row_pitch=0, pix_pitch=0):
    self.N, self.H, self.W, self.C, self.K, self.R, self.S, self.stride = N, H, W, C, K, R, S, stride
    self.pad = (R - 1) // 2 if pad is None else pad
    self.Ho = out_size(H, stride) if Ho is None else Ho
    self.Wo = out_size(W, stride) if Wo is None else Wo
    self.x_img_pitch, self.x_row_pitch, self.x_pix_pitch, self.ldy = img_pitch, row_pitch, pix_pitch, ldy


def out_size(size, stride):
  """conv2d_fixed_padding: SAME for stride 1, fixed_padding(k) + VALID otherwise -> (in - 1) // stride + 1 for either"""
  return (size - 1) // stride + 1


def _pitches(d):
  return (d.x_img_pitch or d.H * d.W * d.C, d.x_row_pitch or d.W * d.C, d.x_pix_pitch or d.C)


def _tap(d, r, s):
  """tap (r, s) of every output pixel -> (rows m of the [N Ho Wo] output whose tap lies inside the map, the element offset of
  the input pixel each of them reads)"""
  n, ho, wo = np.meshgrid(np.arange(d.N), np.arange(d.Ho), np.arange(d.Wo), indexing='ij')
  ih, iw = ho * d.stride + r - d.pad, wo * d.stride + s - d.pad
  ok = ((ih >= 0) & (ih < d.H) & (iw >= 0) & (iw < d.W)).reshape(-1)
  img, row, pix = _pitches(d)
  off = (n * img + ih * row + iw * pix).reshape(-1)
  return np.nonzero(ok)[0], off[ok]


def _gather(xf, off, C):
  return xf[off[:, None] + np.arange(C)[None, :]]


def fprop(x, w, d):
  """x: the input as the kernel's pointer sees it (any shape, read flat through the pitches), w [K, R, S, C] -> the exact
  sums [N Ho Wo, K] in float64"""
  xf, w = np.asarray(x, F64).reshape(-1), np.asarray(w, F64)
  acc = np.zeros((d.N * d.Ho * d.Wo, d.K), F64)
  for r in range(d.R):
    for s in range(d.S):
      m, off = _tap(d, r, s)
      acc[m] += _gather(xf, off, d.C) @ w[:, r, s, :].T
  return acc


def dgrad(dy, w, d):
  """dy [N Ho Wo, K] (columns past K of a padded row ignored), w [K, R, S, C] -> dx [N H W, C]: every product of ``fprop``
  credited to the input element it read (packed input only, as asm_conv2d_dgrad requires)"""
  assert not (d.x_img_pitch or d.x_row_pitch or d.x_pix_pitch)
  dy, w = np.asarray(dy, F64).reshape(d.N * d.Ho * d.Wo, -1)[:, :d.K], np.asarray(w, F64)
  dx = np.zeros((d.N * d.H * d.W, d.C), F64)
  for r in range(d.R):
    for s in range(d.S):
      m, off = _tap(d, r, s)
      dx[off // d.C] += dy[m] @ w[:, r, s, :]       # one tap maps output pixels to input pixels one to one
  return dx


def wgrad(x, dy, d):
  """-> dw [K, R, S, C]: dw(k, r, s, c) = sum over the output pixels of dy(m, k) x(the pixel tap (r, s) of m reads, c)"""
  xf = np.asarray(x, F64).reshape(-1)
  dy = np.asarray(dy, F64).reshape(d.N * d.Ho * d.Wo, -1)[:, :d.K]
  dw = np.zeros((d.K, d.R, d.S, d.C), F64)
  for r in range(d.R):
    for s in range(d.S):
      m, off = _tap(d, r, s)
      dw[:, r, s, :] = dy[m].T @ _gather(xf, off, d.C)
  return dw


# ---- epilogues ----------------------------------------------------------------------------------------------------------
def round_bf16(a):
  """round to nearest-even bfloat16 through ONE float32 -> bf16 cast (the values here are exact in float32), as float64"""
  a32 = np.asarray(a, F64).astype(np.float32)
  assert np.array_equal(a32.astype(F64), np.asarray(a, F64)), 'not a float32 value: the cast would round twice'
  return R.to_bf16(a32).astype(F64)


def mask_bits(mask, C):
  """packed mask [rows, C / 8] bytes -> 0/1 [rows, C]: bit c % 8 of byte c / 8"""
  return R.unpack_mask(np.asarray(mask).reshape(-1, C // 8), C).astype(F64)


def dgrad_out(acc, addend=None, mask=None, pool=None):
  """what an input-gradient kernel stores: the accumulator rounded to bf16 (it crosses LDS as bf16, igemm_epilogue), then in
  fp32 + the pooled gradient's share + the addend where its mask bit is set, rounded once more.  Without any of the three it is
  the accumulator rounded once."""
  v = round_bf16(acc)
  if addend is None and pool is None:
    return v
  if pool is not None:
    v = v + np.asarray(pool, F64).reshape(v.shape)
  if addend is not None:
    a = np.asarray(addend, F64).reshape(v.shape)
    v = v + (a if mask is None else a * mask_bits(mask, v.shape[1]))
  return round_bf16(v)


def pool_bwd(pool_dy, shape, k, stride, count_valid):
  """the average-pool backward asm_conv2d_dgrad_pooled gathers: pool_dy [N, Hp, Wp, C] -> [N H W, C] (pad 0)"""
  N, H, W, C = shape
  return P.avgpool_bwd(pool_dy, shape, k, stride, 0, count_valid).reshape(N * H * W, C)


def pool_shape(shape, k, stride, count_valid):
  N, H, W, C = shape
  return (N, P.avgpool_geometry(H, k, stride, count_valid)[0], P.avgpool_geometry(W, k, stride, count_valid)[0], C)


def fprop_bn(acc, scale, shift, residual=None, relu=False):
  """asm_conv2d_fprop_bn: the convolution rounded to bf16, then [relu](y scale[k] + shift[k] [+ residual]) in fp32, rounded"""
  v = round_bf16(acc) * np.asarray(scale, F64)[None, :] + np.asarray(shift, F64)[None, :]
  if residual is not None:
    v = v + np.asarray(residual, F64).reshape(v.shape)
  return round_bf16(np.maximum(v, 0.0) if relu else v)


def stats(y):
  """per-channel (sum y, sum y^2) of the stored rows -> [2, K]"""
  y = np.asarray(y, F64)
  return np.stack([y.sum(axis=0), (y * y).sum(axis=0)])


def bn_sums(dx, bn_y, relu_mask=None):
  """asm_conv2d_dgrad_bnred: (sum dz, sum dz y) over the rows, dz = the stored dx [where the ReLU mask bit is set] -> [2, C]"""
  dz = np.asarray(dx, F64)
  if relu_mask is not None:
    dz = dz * mask_bits(relu_mask, dz.shape[1])
  return np.stack([dz.sum(axis=0), (dz * np.asarray(bn_y, F64).reshape(dz.shape)).sum(axis=0)])


# ---- the comparison both modules use ----------------------------------------------------------------------------------------
def exact_rows(case, out, ref, pad_value):
  """out [M, ld] against ref [M, K]: the first K columns are the reference, every pad column holds ``pad_value`` (the fill
  pattern where the contract leaves it alone, zero where the contract writes zeros)"""
  out, ref = np.asarray(out), np.asarray(ref)
  K = ref.shape[1]
  exact(case, out[:, :K], ref)
  assert (out[:, K:] == pad_value).all(), '%s: %d pad elements are not %r' % (case, int((out[:, K:] != pad_value).sum()), pad_value)


def exact_partials(case, partials, ref):
  """partials [blocks, 2, K] of a fused reduction: every one an exact integer (an unwritten one is the fill pattern), and their
  float64 sum over the blocks the reference [2, K]"""
  p = np.asarray(partials, F64)
  assert np.array_equal(p, np.rint(p)), '%s: %d partials are not integers' % (case, int((p != np.rint(p)).sum()))
  exact(case, p.sum(axis=0), ref)


# ---- seeded operands ------------------------------------------------------------------------------------------------------
def _signed(r, shape, mags):
  return (r.choice(np.asarray(mags, F64), size=shape) * r.choice(np.asarray([-1.0, 1.0]), size=shape)).astype(np.float32)


def operand(r, shape, L):
  """activations / gradients of a reduction of length L: +-{1, 2} up to 2304, +-1 up to 4608, beyond that not to be used"""
  assert L <= 4608, 'the recipe is not to be used above L = 4608'
  return _signed(r, shape, (1, 2) if L <= 2304 else (1,))


def filters(r, shape):
  return _signed(r, shape, (1,))


def addend_of(r, shape):
  return _signed(r, shape, (1, 2, 3, 4))


def mask_of(r, rows, C):
  return r.integers(0, 256, size=(rows, C // 8), dtype=np.uint8)


def bn_coeffs(r, K):
  """folded batch norm: a power of two per channel in 2^-2 .. 2^1, a shift in quarters with |shift| <= 8"""
  return (2.0 ** r.integers(-2, 2, size=K)).astype(np.float32), (r.integers(-32, 33, size=K) / 4.0).astype(np.float32)


def residual_of(r, shape):
  return r.integers(-8, 9, size=shape).astype(np.float32)


def pooled_of(r, shape):
  """multiples of 4: with pool k = 2 the weights are quarters (halves / ones under count-valid)"""
  return _signed(r, shape, (4, 8))


# ---- case tables ------------------------------------------------------------------------------------------------------------
# family codes of asm_debug_last_conv_kernel (csrc/igemm_common.h ConvFamily)
GENERAL, GEMM1, IGEMM2, IGEMM3, HALO, DGRAD_S2, DENSE, IGEMM8 = 0, 1, 2, 3, 4, 5, 6, 8
GEMM1_CODES = (1, 5, 8, 10, 11, 12, 13, 14, 16)      # as tests/test_gpu_conv.py

# shape = (N, H, W, C, K, k, stride); fam_f / fam_d: the family the forward / the input gradient must report under ``knobs``;
# flags: 'pool' the pooled-gradient gather, 'bnred' the batch-norm backward sums, 'bn' asm_conv2d_fprop_bn, 'nomask' the entry
# point takes no masked addend (1x1 / stride 2)
Case = namedtuple('Case', 'name shape knobs fam_f fam_d flags')


def _c(name, shape, knobs, fam_f, fam_d, flags=''):
  return Case(name, shape, dict(knobs), fam_f, fam_d, frozenset(flags.split()))


_I2 = {'ASM_IGEMM3': '0', 'ASM_IGEMM8': '0', 'ASM_GEMM1': '0'}

CONV_CASES = [
    # the general kernel: channel tail 72 % 32 = 8 and a K tail; strided with a masked N; ragged M = 147, K tail 8 in the fifth
    # column tile
    _c('general', (2, 9, 9, 72, 40, 3, 1), {'ASM_IGEMM_MODE': '1'}, GENERAL, GENERAL, 'bn'),
    _c('general', (2, 12, 12, 32, 32, 3, 2), {'ASM_IGEMM_MODE': '1'}, GENERAL, GENERAL, 'bn'),
    _c('general', (3, 7, 7, 256, 520, 1, 1), {'ASM_IGEMM_MODE': '1'}, GENERAL, GENERAL, 'bn bnred'),
    # igemm2: BK 32; ragged M on four column tiles; an odd map under stride 2 (its input gradient: four parity classes on
    # igemm2); 1x1; the 256 x 256 tile with M < one tile
    _c('igemm2', (2, 12, 12, 32, 64, 3, 1), _I2, IGEMM2, IGEMM2, 'bn'),
    _c('igemm2', (3, 7, 7, 256, 512, 3, 1), _I2, IGEMM2, IGEMM2, 'bn'),
    _c('igemm2', (4, 15, 15, 64, 64, 3, 2), _I2, IGEMM2, IGEMM2, 'bn'),
    _c('igemm2', (2, 16, 16, 256, 64, 1, 1), _I2, IGEMM2, IGEMM2, 'bn pool bnred'),
    _c('igemm2-tile256', (3, 7, 7, 256, 512, 3, 1), dict(_I2, ASM_IGEMM_TILE='3'), IGEMM2, IGEMM2, 'bn'),
    _c('igemm2-tile256', (4, 15, 15, 64, 64, 3, 2), dict(_I2, ASM_IGEMM_TILE='3'), IGEMM2, IGEMM2, 'bn'),
    # stride-2 input gradient as parity classes: four classes of unequal size scattered into odd H and W; 1x1 with one class,
    # the other three quarters of dx exact zeros or exactly the addend
    _c('parity', (4, 15, 15, 64, 64, 3, 2), {'ASM_DGRAD_PARITY': '1'}, IGEMM2, IGEMM2),
    _c('parity', (2, 9, 11, 64, 96, 1, 2), {'ASM_DGRAD_PARITY': '1'}, IGEMM2, IGEMM2, 'nomask'),
    # ... and as the generic gather over dy (three quarters of its pixel / tap pairs are parity misses)
    _c('gather', (4, 15, 15, 64, 64, 3, 2), {'ASM_DGRAD_PARITY': '0'}, IGEMM2, IGEMM2),
    # the one-launch stride-2 input gradient
    _c('dgrad_s2', (1, 16, 16, 64, 64, 3, 2), {'ASM_DGRAD_PARITY': '2'}, IGEMM2, DGRAD_S2),
    _c('dgrad_s2', (3, 16, 32, 64, 64, 3, 2), {'ASM_DGRAD_PARITY': '2'}, IGEMM2, DGRAD_S2),
] + [
    # ring-GEMM, every configuration of its table: a single partial chunk (24 channels), ragged rows, N tail; L = 1024
    _c('gemm1-%d' % code, shape, {'ASM_GEMM1': str(code)}, GEMM1, GEMM1, 'pool bnred')
    for code in GEMM1_CODES for shape in ((1, 9, 11, 24, 192, 1, 1), (3, 7, 7, 1024, 320, 1, 1))
] + [
    # ... and forward only where the gathered channels of the input gradient (136, 264) are no multiple of a ring step, which
    # leaves that direction to the general kernel: a 40-channel tail inside the one 64-channel chunk (the 64-channel
    # configurations), ragged rows, an N tail of 8; L = 1024 with an N tail of 8
    _c('gemm1-%d' % code, (1, 9, 11, 40, 136, 1, 1), {'ASM_GEMM1': str(code)}, GEMM1, GENERAL) for code in (1, 8, 11)
] + [
    _c('gemm1-%d' % code, (3, 7, 7, 1024, 264, 1, 1), {'ASM_GEMM1': str(code)}, GEMM1, GENERAL) for code in GEMM1_CODES
] + [
    # igemm3: images inside a tile and a K tail; the widest map; a single chunk in the 256-row buffer; the input gradient of
    # the K-tail shapes gathers 136 / 72 channels, which only the general kernel steps through
    _c('igemm3', (5, 7, 7, 192, 136, 3, 1), {'ASM_IGEMM3': '2'}, IGEMM3, GENERAL, 'bn'),
    _c('igemm3', (1, 9, 30, 128, 128, 3, 1), {'ASM_IGEMM3': '2'}, IGEMM3, IGEMM3, 'bn bnred'),
    _c('igemm3', (3, 7, 7, 192, 128, 3, 1), {'ASM_IGEMM3': '2'}, IGEMM3, IGEMM3, 'bn bnred'),
    _c('igemm3', (1, 11, 62, 64, 72, 3, 1), {'ASM_IGEMM3': '3'}, IGEMM3, GENERAL, 'bn'),
    _c('igemm3', (2, 9, 31, 64, 136, 3, 1), {'ASM_IGEMM3': '3'}, IGEMM3, GENERAL, 'bn'),
    # igemm8: M = 147 < one tile with an N tail 192 of 256; two row tiles, the second ragged, an 8-column tail in the second
    # column tile (its input gradient gathers 264 channels: the general kernel); 128 gathered channels for the fused sums
    _c('igemm8', (3, 7, 7, 128, 192, 3, 1), {'ASM_IGEMM8': '2'}, IGEMM8, IGEMM8, 'bn'),
    _c('igemm8', (2, 14, 14, 64, 264, 3, 1), {'ASM_IGEMM8': '2'}, IGEMM8, GENERAL, 'bn'),
    _c('igemm8', (3, 7, 7, 256, 128, 3, 1), {'ASM_IGEMM8': '2'}, IGEMM8, IGEMM8, 'bn bnred'),
    # conv_halo: one patch per image; 8 x 16 patches; 3 x 3 patches
    _c('halo', (3, 8, 16, 32, 64, 3, 1), {}, HALO, HALO),
    _c('halo', (2, 16, 32, 64, 32, 3, 1), {}, HALO, HALO),
    _c('halo', (1, 24, 48, 32, 32, 3, 1), {}, HALO, HALO),
]

# dense [N,1,1,C] layers: (N, C, K, ldy), then the family of the forward and of the input gradient with asm_tuning.dense_small
# 1 and 0.  dense_small_kernel takes a direction whose reduction is a multiple of 16 (asm_hip.h; dense_covers): both of the
# second shape, neither of the first, whose weight gradient alone is a dense form, and the forward of the third: its input
# gradient (K = 100) runs on a descriptor padded to K = 104, as the network's classifier does, and 104 is no multiple of 16.
DenseCase = namedtuple('DenseCase', 'N C K ldy fam_f fam_d fam_f0 fam_d0')
DENSE_CASES = [DenseCase(37, 40, 24, 0, GENERAL, IGEMM2, GENERAL, IGEMM2),
               DenseCase(37, 48, 80, 0, DENSE, DENSE, GENERAL, GENERAL),
               DenseCase(64, 256, 100, 104, DENSE, GENERAL, IGEMM2, GENERAL)]

# stem (pitched input, R = k, S = 1): (N, H, W, k, K)
STEM_CASES = [(2, 32, 32, 7, 64), (1, 24, 40, 7, 64), (2, 32, 32, 3, 32), (1, 24, 40, 3, 32)]

# weight gradient: the form (asm_conv2d_wgrad_plan's second entry: 128 wgrad_kernel, 256 wgrad8_kernel, -1 halo) and the split
# count the plan must report; register-staged against ring is what ASM_WGRAD_RING = 0 / 1 forces on a 1x1 stride-1 layer
WCase = namedtuple('WCase', 'name shape knobs bcw splits')


def _w(name, shape, knobs, bcw, splits):
  return WCase(name, shape, dict(knobs), bcw, splits)


_REG = {'ASM_WGRAD_RING': '0'}
WGRAD_CASES = [
    # register-staged: column tail 648 = 5 128 + 8 and K 40 of 64; three slabs with a split ending inside an image; stride 2
    _w('reg', (2, 9, 9, 72, 40, 3, 1), _REG, 128, 1),
    _w('reg-splits3', (2, 9, 9, 72, 40, 3, 1), dict(_REG, ASM_WGRAD_SPLITS='3'), 128, 3),
    _w('reg', (4, 15, 15, 64, 64, 3, 2), _REG, 128, 1),
    _w('reg', (2, 9, 11, 64, 72, 1, 2), _REG, 128, 1),
    # ... and the linear-address 1x1 stride-1 form of the same kernel (the ring's shapes)
    _w('reg', (2, 9, 11, 40, 24, 1, 1), _REG, 128, 1),
    _w('reg', (3, 7, 7, 520, 264, 1, 1), _REG, 128, 1),
    # LDS-DMA ring (1x1 stride 1)
    _w('ring', (2, 9, 11, 40, 24, 1, 1), {'ASM_WGRAD_RING': '1'}, 128, 1),
    _w('ring', (3, 7, 7, 520, 264, 1, 1), {'ASM_WGRAD_RING': '1'}, 128, 1),
    _w('ring-splits3', (3, 7, 7, 520, 264, 1, 1), {'ASM_WGRAD_RING': '1', 'ASM_WGRAD_SPLITS': '3'}, 128, 3),
    # 256 x 256: columns 648 padded to 768; 1x1; and a K tail (264 of 512)
    _w('big', (3, 7, 7, 128, 256, 3, 1), {'ASM_WGRAD_BIG': '1'}, 256, 1),
    _w('big', (2, 14, 14, 72, 512, 3, 1), {'ASM_WGRAD_BIG': '1'}, 256, 1),
    _w('big', (2, 14, 14, 256, 256, 1, 1), {'ASM_WGRAD_BIG': '1'}, 256, 1),
    _w('big-ktail', (3, 7, 7, 128, 264, 3, 1), {'ASM_WGRAD_BIG': '1'}, 256, 1),
    _w('big-splits3', (2, 14, 14, 256, 256, 1, 1), {'ASM_WGRAD_BIG': '1', 'ASM_WGRAD_SPLITS': '3'}, 256, 3),
    # resident halo: the eight-wave form; 32 -> 32; two K slices; 56-wide bands
    _w('halo', (3, 8, 16, 64, 64, 3, 1), {'ASM_WGRAD_HALO': '2'}, -1, 3),
    _w('halo', (2, 8, 16, 32, 32, 3, 1), {'ASM_WGRAD_HALO': '2'}, -1, 2),
    _w('halo', (1, 4, 28, 64, 128, 3, 1), {'ASM_WGRAD_HALO': '2'}, -1, 1),
    _w('halo', (1, 2, 56, 32, 64, 3, 1), {'ASM_WGRAD_HALO': '2'}, -1, 1),
    # deep 3x3 under the cost model and with three slabs
    _w('deep', (3, 7, 7, 64, 128, 3, 1), {}, 128, 1),
    _w('deep-splits3', (3, 7, 7, 64, 128, 3, 1), {'ASM_WGRAD_SPLITS': '3'}, 128, 3),
    _w('deep', (6, 7, 14, 128, 128, 3, 1), {}, 128, 1),
    _w('deep-splits3', (6, 7, 14, 128, 128, 3, 1), {'ASM_WGRAD_SPLITS': '3'}, 128, 3),
]


def case_id(c):
  return '%s-%s' % (c.name, 'x'.join(map(str, c.shape)))


def desc_of(shape, **kw):
  N, H, W, C, K, k, stride = shape
  return Desc(N, H, W, C, K, k, k, stride, **kw)


def seed_of(*key):
  return zlib.crc32(repr(key).encode()) & 0x7fffffff


def _frozen(d):
  for v in d.values():
    if isinstance(v, np.ndarray):
      v.setflags(write=False)
  return d


@functools.lru_cache(maxsize=None)
def conv_reference(shape):
  """operands and exact sums of a forward / input-gradient case, computed once per shape and read-only"""
  N, H, W, C, K, k, stride = shape
  d = desc_of(shape)
  r = R.rng(seed_of('conv', shape))
  M, Mi, Lf, Ld = N * d.Ho * d.Wo, N * H * W, k * k * C, k * k * K
  out = dict(d=d, M=M, Mi=Mi, Lf=Lf, Ld=Ld)
  out['w'] = filters(r, (K, k, k, C))
  out['x'] = operand(r, (N, H, W, C), Lf)
  out['dy'] = operand(r, (M, K), Ld)
  out['addend'] = addend_of(r, (Mi, C))
  out['mask'] = mask_of(r, Mi, C)
  out['acc_f'] = fprop(out['x'], out['w'], d)
  out['acc_d'] = dgrad(out['dy'], out['w'], d)
  out['scale'], out['shift'] = bn_coeffs(r, K)
  out['residual'] = residual_of(r, (M, K))
  out['bn_y'] = _signed(r, (Mi, C), (1, 2, 3))
  out['relu_mask'] = mask_of(r, Mi, C)
  return _frozen(out)


@functools.lru_cache(maxsize=None)
def wgrad_reference(shape, ldy=0):
  N, H, W, C, K, k, stride = shape
  d = desc_of(shape, ldy=ldy)
  r = R.rng(seed_of('wgrad', shape))
  M = N * d.Ho * d.Wo
  out = dict(d=d, M=M)
  out['x'] = _signed(r, (N, H, W, C), (1, 2, 3))
  dy = np.zeros((M, max(ldy, K)), np.float32)
  dy[:, :K] = _signed(r, (M, K), (1, 2))
  out['dy'] = dy
  out['dw'] = wgrad(out['x'], dy, d)
  return _frozen(out)


@functools.lru_cache(maxsize=None)
def dense_reference(case):
  return conv_reference((case.N, 1, 1, case.C, case.K, 1, 1))


def stem_desc(N, H, W, k, K):
  """nn.ConvKernel.desc of a stem layer: R = k, S = 1, "C" = round_up(4 k, 8) lanes over the zero-haloed [N][H+6][W+6][4] buffer"""
  Hp, Wp = H + 6, W + 6
  return Desc(N, Hp, Wp, R.stem_lanes(k), K, k, 1, 2, pad=0, Ho=out_size(H, 2), Wo=out_size(W, 2),
              img_pitch=Hp * Wp * 4, row_pitch=Wp * 4, pix_pitch=4)


def stem_view_offset(W, k):
  """the halo is 3 pixels wide, a k x k window needs (k - 1) // 2: the kernel's pointer starts that many rows / pixels in"""
  off = 3 - (k - 1) // 2
  return (off * (W + 6) + off) * 4


@functools.lru_cache(maxsize=None)
def stem_reference(case):
  """-> the padded buffer xp [N, H+6, W+6, 4], the master filter w [K, k, k, 3], its packed rows, dy, and the exact forward
  sums / packed and unpacked weight gradient through the pitched descriptor"""
  N, H, W, k, K = case
  d = stem_desc(N, H, W, k, K)
  r = R.rng(seed_of('stem', case))
  out = dict(d=d, M=N * d.Ho * d.Wo)
  out['w'] = filters(r, (K, k, k, 3))
  out['wp'] = R.stem_pack(out['w'])
  out['xp'] = R.stem_pad(_signed(r, (N, H, W, 3), (1, 2, 3)))
  out['dy'] = _signed(r, (out['M'], K), (1, 2))
  # what the pointer sees: the buffer from the view's first element on; a read past the buffer's end is a NaN
  view = np.concatenate([out['xp'].reshape(-1)[stem_view_offset(W, k):], np.full(stem_view_offset(W, k) + 64, np.nan, np.float32)])
  out['acc_f'] = fprop(view, out['wp'].reshape(K, k, 1, -1), d)
  out['dwp'] = wgrad(view, out['dy'], d).reshape(K, k, -1)
  out['dw'] = R.stem_unpack(out['dwp'], k).astype(F64)
  return _frozen(out)
