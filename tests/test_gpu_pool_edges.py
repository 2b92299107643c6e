"""Edge shapes, ties and guard bands of the pooling, SK and SE kernels (csrc/pool.hip, csrc/sk_se.hip, csrc/sk_fused.hip)
against the plain float64 references of tests/pool_ref.py, which tests/test_pool_ref_cpu.py proves against the oracle on the
CPU.  Every case calls the C ABI directly.

Rules of every case:
* every output is an ``Out``: 4 KiB of the byte 0xA5 on either side, which must survive the call, and an output that starts as
  0xA5, so an element the kernel skips shows.  Every bf16 and mask input is an ``In``: 4 KiB of NaN on either side (+1e30 for
  the max pool, whose ``f > best`` drops a NaN; the impossible code 0xFF for the argmax bytes), and no output may hold a NaN or a huge value.
* two kinds of input.  GRID: values j / 8, |j| <= 32 (clamped at 0 for the max pool, so zeros tie), on which every float32
  sum the kernels form is exact: the output must be the bf16 nearest the float64 reference, bit for bit (``same``).  RANDOM:
  rows_ref.bf16_randn under |out - ref| <= 2^-8 |ref| + 4 floor (+ n 2^-24 sum |terms| for a float32 sum of n terms,
  + 1e-4 of what a gate that went through __expf multiplies); floor = rows_ref.floor_of(reference), measured on the reference
  alone.  profiles/pool_edges_tolerances.md derives each bound and records the worst measured fraction of it.
* bounds are element-wise, never a norm; ``-s`` prints the worst error of every case next to its bound.

Max-pool inputs are finite: what the kernel does with a NaN or with a window of -inf only is not asserted.
"""
import numpy as np
import pytest
import torch

from tests import gpu_guard as G
from tests import pool_ref as P
from tests import rows_ref as R
from tests.gpu_guard import BF, In, Out, _release_inputs, call, dev, exact, ptr  # noqa: F401

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
U8 = torch.uint8
TF32 = torch.float32


def bf(ref):
  """the bf16 nearest a float64 reference value, as float64.  Magnitudes below the float32 normal range count as 0: they
  arise only from a gate of exp(-100) = 3.7e-44, which float32 arithmetic loses against 1 (the gate is exactly 0)"""
  return R.to_bf16(flush(ref).astype(F32)).astype(F64)


def same(case, out, ref):
  """equal bits: the output is the bf16 nearest the reference (+0 and -0 count as equal)"""
  exact(case, np.asarray(out, F64), bf(ref))
  print('\npool-edges %-46s equal bits (%d elements)' % (case, np.size(out)), end='')


def close(case, out, ref, bound):
  out, ref = np.asarray(out, F64), np.asarray(ref, F64)
  err, bound = np.abs(out - ref), np.asarray(bound, F64) + np.zeros_like(ref)
  worst = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
  print('\npool-edges %-46s worst |err| %.3e = %.3f of its bound' % (case, float(err.max()) if err.size else 0.0, worst), end='')
  assert (err <= bound).all(), '%s: |err| %.3e at %s' % (case, err.max(), np.unravel_index(np.argmax(err - bound), err.shape))


def bf16_bound(ref, floor, n=0, sum_abs=0.0, gated=0.0):
  """2^-8 |ref| + 4 floor + n 2^-24 sum |terms| + 1e-4 |what an __expf gate multiplies|"""
  return R.BF16_ULP * np.abs(ref) + 4.0 * floor + n * R.U24 * np.asarray(sum_abs, F64) + 1e-4 * np.asarray(gated, F64)


def untouched(out):
  return bool((out.buf.view(U8) == G.PATTERN).all())


def refused(name, *args):
  with pytest.raises(ValueError):      # ASM_EINVAL
    call(name, *args)


def flush(ref):
  """a float32 sum whose only non-zero terms carry a gate of exp(-100) = 3.7e-44 is exactly 0 on the device"""
  r = np.asarray(ref, F64)
  return np.where(np.abs(r) < 2.0 ** -126, 0.0, r)


# ---- max pool 3x3 / 2 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['grid', 'const', 'random'])
@pytest.mark.parametrize('shape', P.MAXPOOL_SHAPES)
def test_maxpool_ties_and_shapes(hip_lib, shape, kind):
  """H != W, odd and even extents (a row or column of padding before, or none), one pixel, a second and ragged block
  (15 x 17: 288 output vectors); post-ReLU zeros that tie and a constant map where every window is a full tie: y, the argmax
  bytes and dx bit for bit -- the first maximum in (r, s) scan order among the VALID taps gets the gradient"""
  N, H, W, C = shape
  r = R.rng(11, *shape)
  x = {'grid': lambda: P.grid(r, shape, relu=True), 'const': lambda: np.full(shape, 1.5, F32),
       'random': lambda: R.bf16_randn(r, shape)}[kind]()
  y_ref, code = P.maxpool3x3s2(x)
  dy = P.grid(R.rng(12, *shape), y_ref.shape)
  xd = In(x, BF, 1e30)
  y, amax, y2 = Out(y_ref.shape, BF), Out(y_ref.shape, U8), Out(y_ref.shape, BF)
  call('asm_maxpool3x3s2_fwd', xd.p, y.p, amax.p, N, H, W, C)
  call('asm_maxpool3x3s2_fwd', xd.p, y2.p, None, N, H, W, C)
  case = 'maxpool %s %s' % (kind, 'x'.join(map(str, shape)))
  same(case + ' y', y.np(), y_ref)
  same(case + ' y (no argmax)', y2.np(), y_ref)
  exact(case + ' argmax', amax.np(), code)
  dx = Out(shape, BF)
  call('asm_maxpool3x3s2_bwd', In(dy).p, In(code.astype(np.uint8), U8, 0xFF).p, dx.p, N, H, W, C)
  same(case + ' dx', dx.np(), P.maxpool3x3s2_bwd(dy, code, shape))


# ---- average pool -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', P.AVG_FORMS)
@pytest.mark.parametrize('shape', P.AVG_SHAPES)
def test_avgpool_non_square(hip_lib, shape, form):
  """the three forms of the network on maps with H != W: forward, backward, backward + a separate addend, backward + the
  addend aliased to dx.  Divisors 1, 2 and 4 (k = 2, either count mode) are exact on grid inputs: equal bits; the divisor 9
  and random inputs are held to the bound"""
  k, stride, pad, cv = form
  N, H, W, C = shape
  Ho, Wo = P.avgpool_geometry(H, k, stride, cv)[0], P.avgpool_geometry(W, k, stride, cv)[0]
  oshape = (N, Ho, Wo, C)
  for kind in ('grid', 'random'):
    r = R.rng(21, *shape, k, stride, kind == 'grid')
    if kind == 'grid':
      x, dy, add = P.grid(r, shape), P.grid(r, oshape), P.grid(r, shape)
    else:
      x, dy, add = R.bf16_randn(r, shape), R.bf16_randn(r, oshape), R.bf16_randn(r, shape)
    case = 'avgpool k%d s%d cv%d %s %s' % (k, stride, cv, kind, 'x'.join(map(str, shape)))
    floor = R.floor_of(lambda dt: (P.avgpool(x, k, stride, pad, Ho, Wo, cv, dt),
                                   P.avgpool_bwd(dy, shape, k, stride, pad, cv, add, dt)))

    def check(what, out, ref, sum_abs):
      if kind == 'grid' and k == 2:
        same(case + what, out, ref)
      else:
        close(case + what, out, ref, bf16_bound(ref, floor, k * k + 1, sum_abs))

    y = Out(oshape, BF)
    call('asm_avgpool_fwd', In(x).p, y.p, N, H, W, C, k, stride, pad, Ho, Wo, cv)
    check(' y', y.np(), P.avgpool(x, k, stride, pad, Ho, Wo, cv), P.avgpool(np.abs(x), k, stride, pad, Ho, Wo, cv))
    dyd = In(dy)
    abs_dx = P.avgpool_bwd(np.abs(dy), shape, k, stride, pad, cv)
    dx = Out(shape, BF)
    call('asm_avgpool_bwd', dyd.p, dx.p, N, H, W, C, k, stride, pad, Ho, Wo, cv, None)
    check(' dx', dx.np(), P.avgpool_bwd(dy, shape, k, stride, pad, cv), abs_dx)
    ref_add = P.avgpool_bwd(dy, shape, k, stride, pad, cv, addend=add)
    dx = Out(shape, BF)
    call('asm_avgpool_bwd', dyd.p, dx.p, N, H, W, C, k, stride, pad, Ho, Wo, cv, In(add).p)
    check(' dx + addend', dx.np(), ref_add, abs_dx + np.abs(add))
    dx = Out(shape, BF, init=dev(add, BF))
    call('asm_avgpool_bwd', dyd.p, dx.p, N, H, W, C, k, stride, pad, Ho, Wo, cv, dx.p)
    check(' dx += (aliased)', dx.np(), ref_add, abs_dx + np.abs(add))


def test_avgpool_bwd_refuses_stride_3(hip_lib):
  """the gather form tests window membership with a shift and a mask: stride 3 is refused with a status, nothing is written"""
  N, H, W, C, k, stride, pad = 2, 7, 5, 8, 3, 3, 1
  Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
  dx = Out((N, H, W, C), BF)
  refused('asm_avgpool_bwd', In(P.grid(R.rng(22), (N, Ho, Wo, C))).p, dx.p, N, H, W, C, k, stride, pad, Ho, Wo, 0, None)
  torch.cuda.synchronize()
  assert untouched(dx)


# ---- blur pool --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('shape,ks', P.BLUR_CASES)
def test_blurpool_filters_strides_and_reflections(hip_lib, shape, ks, stride):
  """k in 2..7 at strides 1 and 2, maps no larger than the padding reaches, H != W; grid inputs: equal bits for the generic
  kernels and for the k = 3 / stride 2 fast backward path (its "same bits" claim); random inputs: the bound"""
  N, H, W, C = shape
  for k in ks:
    oshape = (N, P.blur_out(H, k, stride), P.blur_out(W, k, stride), C)
    for kind in ('grid', 'random'):
      r = R.rng(31, *shape, k, stride, kind == 'grid')
      x, dy = (P.grid(r, shape), P.grid(r, oshape)) if kind == 'grid' else (R.bf16_randn(r, shape), R.bf16_randn(r, oshape))
      case = 'blur k%d s%d %s %s' % (k, stride, kind, 'x'.join(map(str, shape)))
      y, dx = Out(oshape, BF), Out(shape, BF)
      call('asm_blurpool_fwd', In(x).p, y.p, N, H, W, C, k, stride)
      call('asm_blurpool_bwd', In(dy).p, dx.p, N, H, W, C, k, stride)
      y_ref, dx_ref = P.blurpool(x, k, stride), P.blurpool_bwd(dy, shape, k, stride)
      if kind == 'grid':
        same(case + ' y', y.np(), y_ref)
        same(case + ' dx', dx.np(), dx_ref)
      else:
        floor = R.floor_of(lambda dt: (P.blurpool(x, k, stride, dt), P.blurpool_bwd(dy, shape, k, stride, dt)))
        close(case + ' y', y.np(), y_ref, bf16_bound(y_ref, floor, k * k, P.blurpool(np.abs(x), k, stride)))
        # a pixel draws on at most 3 padded positions per axis, k taps each
        close(case + ' dx', dx.np(), dx_ref, bf16_bound(dx_ref, floor, 9 * k * k, P.blurpool_bwd(np.abs(dy), shape, k, stride)))


def test_blurpool_fwd_refuses_pad_not_below_size(hip_lib):
  """REFLECT folds once: pad >= H has no source pixel and is refused with a status"""
  y = Out((1, 3, 5, 8), BF)
  refused('asm_blurpool_fwd', In(P.grid(R.rng(32), (1, 3, 5, 8))).p, y.p, 1, 3, 5, 8, 7, 1)
  torch.cuda.synchronize()
  assert untouched(y)


# ---- row-lane reductions ------------------------------------------------------------------------------------------------------
# C = 256: vcb = 32.  256 threads: nrl = 8, the unrolled loop takes U nrl = 32 rows (GAP, U = 4) or 16 (sk_select_bwd_att,
# U = 2) per trip; 1024 threads from HW = 512 on: nrl = 32, 128 or 64 rows per trip.  Below, at and above every boundary.
ROWS_256 = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 49, 511, 512, 513, 575, 576, 577, 639, 640, 641]
# C = 8, 24: fewer columns than 32; C = 72: vcb = 9 leaves 4 idle threads; C = 264: a second column group of one vector
ROW_CASES = [(256, hw) for hw in ROWS_256] + [(c, hw) for c in (8, 24, 72, 264) for hw in (1, 5, 29, 513)]
N_ROWS = 2


@pytest.mark.parametrize('C,HW', ROW_CASES)
def test_gap_row_lanes(hip_lib, C, HW):
  """gap_fwd, sk_gap (both through gap_fwd_kernel) and gap_bwd"""
  N = N_ROWS
  for kind in ('grid', 'random'):
    r = R.rng(41, C, HW, kind == 'grid')
    mk = (lambda s: P.grid(r, s)) if kind == 'grid' else (lambda s: R.bf16_randn(r, s))
    x, f, dy = mk((N, HW, C)), mk((N, HW, 2 * C)), mk((N, C))
    case = 'C=%d HW=%d %s' % (C, HW, kind)
    y, s, dx = Out((N, C), BF), Out((N, C), BF), Out((N, HW, C), BF)
    call('asm_gap_fwd', In(x).p, y.p, N, HW, C)
    call('asm_sk_gap', In(f).p, s.p, N, HW, C)
    call('asm_gap_bwd', In(dy).p, dx.p, N, HW, C)
    if kind == 'grid':      # the sum is exact; the kernels state the scaling: t * (1.0f / HW)
      same('gap_fwd ' + case, y.np(), P.mean_of_exact_sum(x.astype(F64).sum(1), HW))
      same('sk_gap ' + case, s.np(), P.mean_of_exact_sum(f.astype(F64).sum(1)[:, :C] + f.astype(F64).sum(1)[:, C:], HW))
      same('gap_bwd ' + case, dx.np(), np.broadcast_to(P.mean_of_exact_sum(dy, HW)[:, None], (N, HW, C)))
    else:
      fl = R.floor_of(lambda dt: P.gap(x, dt))
      close('gap_fwd ' + case, y.np(), P.gap(x), bf16_bound(P.gap(x), fl, HW, P.gap(np.abs(x))))
      fl = R.floor_of(lambda dt: P.sk_gap(f, C, dt))
      close('sk_gap ' + case, s.np(), P.sk_gap(f, C), bf16_bound(P.sk_gap(f, C), fl, 2 * HW, P.sk_gap(np.abs(f), C)))
      fl = R.floor_of(lambda dt: P.gap_bwd(dy, (N, HW, C), dt))
      close('gap_bwd ' + case, dx.np(), P.gap_bwd(dy, (N, HW, C)), bf16_bound(P.gap_bwd(dy, (N, HW, C)), fl))


def exact_gate_logits(r, N, Fh):
  """logit differences 0 and +-100: gates of exactly 1/2, 0 and 1"""
  att = np.zeros((N, 2 * Fh), F32)
  att[:, :Fh] = r.integers(-4, 5, (N, Fh)).astype(F32)
  att[:, Fh:] = att[:, :Fh] + np.asarray([0.0, 100.0, -100.0, 0.0], F32)[r.integers(0, 4, (N, Fh))]
  return att


@pytest.mark.parametrize('C,HW', ROW_CASES)
def test_sk_att_and_se_e_row_lanes(hip_lib, C, HW):
  """sk_select_bwd_att (unrolled by 2, 1024 threads from HW = 512) and se_scale_bwd_e (one row per trip, 256 threads)"""
  N, Fh = N_ROWS, C
  for kind in ('grid', 'random'):
    r = R.rng(42, C, HW, kind == 'grid')
    mk = (lambda s: P.grid(r, s)) if kind == 'grid' else (lambda s: R.bf16_randn(r, s))
    f, dv, x, dy = mk((N, HW, 2 * Fh)), mk((N, HW, Fh)), mk((N, HW, C)), mk((N, HW, C))
    if kind == 'grid':
      att = exact_gate_logits(r, N, Fh)
      e = np.asarray([0.0, 100.0, -100.0], F32)[r.integers(0, 3, (N, C))]
    else:
      att, e = P.sk_logits(r, N, Fh), P.se_logits(r, N, C)
    case = 'C=%d HW=%d %s' % (C, HW, kind)
    datt, de = Out((N, 2 * Fh), BF), Out((N, C), BF)
    call('asm_sk_select_bwd_att', In(f).p, In(dv).p, ptr(dev(att)), datt.p, N, HW, Fh)
    call('asm_se_scale_bwd_e', In(x).p, In(dy).p, ptr(dev(e)), de.p, N, HW, C)
    datt_ref, de_ref = P.sk_select_bwd_att(f, dv, att), P.se_scale_bwd_e(x, dy, e)
    if kind == 'grid':
      same('sk_select_bwd_att ' + case, datt.np(), datt_ref)
      same('se_scale_bwd_e ' + case, de.np(), de_ref)
    else:
      # the gate factor a0 (1 - a0) is at most 1/4 and multiplies the sum.  d[a (1 - a)] = (1 - 2a) da is at most 1e-4 in
      # ABSOLUTE terms for a relative 1e-4 in a, so the gated magnitude is the sum of |terms| itself; the 2^-24 of the
      # complement formed in float32 is among the HW + 4 roundings
      mag = (np.abs(f[:, :, :Fh].astype(F64) - f[:, :, Fh:]) * np.abs(dv)).sum(1)
      mag = np.concatenate([mag, mag], axis=1)
      fl = R.floor_of(lambda dt: P.sk_select_bwd_att(f, dv, att, dt))
      close('sk_select_bwd_att ' + case, datt.np(), datt_ref, bf16_bound(datt_ref, fl, HW + 4, mag / 4, mag))
      mag = (np.abs(x.astype(F64)) * np.abs(dy)).sum(1)
      fl = R.floor_of(lambda dt: P.se_scale_bwd_e(x, dy, e, dt))
      close('se_scale_bwd_e ' + case, de.np(), de_ref, bf16_bound(de_ref, fl, HW + 4, mag / 4, mag))
      hard = np.abs(att[:, :Fh] - att[:, Fh:]) > 90
      assert (datt.np()[:, :Fh][hard] == 0).all() and (de.np()[np.abs(e) == 100] == 0).all()


# ---- element-wise SK select and SE scale --------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,HW,C', [(2, 1, 8), (3, 5, 24), (3, 49, 40), (2, 33, 264)])
def test_sk_select_and_se_scale_gates(hip_lib, N, HW, C):
  """sk_select_fwd, sk_select_bwd_f, se_scale_fwd, se_scale_bwd_x: the (image, row, column) decode at N = 2 and 3, a ragged
  last block, gate logits that differ by 0, +-30 and +-100 (SE: e = +-100): at +-100 the gate is exactly 0 or 1"""
  Fh = C
  for kind in ('grid', 'random'):
    r = R.rng(43, N, HW, C, kind == 'grid')
    mk = (lambda s: P.grid(r, s)) if kind == 'grid' else (lambda s: R.bf16_randn(r, s))
    f, dv, ds, x, dy, dsq = mk((N, HW, 2 * Fh)), mk((N, HW, Fh)), mk((N, Fh)), mk((N, HW, C)), mk((N, HW, C)), mk((N, C))
    if kind == 'grid':
      att = exact_gate_logits(r, N, Fh)
      e = np.asarray([0.0, 100.0, -100.0], F32)[r.integers(0, 3, (N, C))]
      ds, dsq = np.zeros_like(ds), np.zeros_like(dsq)        # ds / HW is not exact
    else:
      att, e = P.sk_logits(r, N, Fh), P.se_logits(r, N, C)
    case = 'N=%d HW=%d C=%d %s' % (N, HW, C, kind)
    attd, ed = dev(att), dev(e)
    v, df, y, dx = Out((N, HW, Fh), BF), Out((N, HW, 2 * Fh), BF), Out((N, HW, C), BF), Out((N, HW, C), BF)
    call('asm_sk_select_fwd', In(f).p, ptr(attd), v.p, N, HW, Fh)
    call('asm_sk_select_bwd_f', In(dv).p, ptr(attd), In(ds).p, df.p, N, HW, Fh)
    call('asm_se_scale_fwd', In(x).p, ptr(ed), y.p, N, HW, C)
    call('asm_se_scale_bwd_x', In(dy).p, ptr(ed), In(dsq).p, dx.p, N, HW, C)
    refs = (P.sk_select(f, att), P.sk_select_bwd_f(dv, att, ds), P.se_scale(x, e), P.se_scale_bwd_x(dy, e, dsq))
    outs = (v.np(), df.np(), y.np(), dx.np())
    names = ('sk_select_fwd ', 'sk_select_bwd_f ', 'se_scale_fwd ', 'se_scale_bwd_x ')
    if kind == 'grid':
      for nm, o, rf in zip(names, outs, refs):
        same(nm + case, o, rf)
      continue
    f64, dv64 = f.astype(F64), np.abs(dv.astype(F64))
    gated = (np.abs(f64[:, :, :Fh]) + np.abs(f64[:, :, Fh:]), np.concatenate([dv64, dv64], axis=2), np.abs(x.astype(F64)),
             np.abs(dy.astype(F64)))
    fns = (lambda dt: P.sk_select(f, att, dt), lambda dt: P.sk_select_bwd_f(dv, att, ds, dt), lambda dt: P.se_scale(x, e, dt),
           lambda dt: P.se_scale_bwd_x(dy, e, dsq, dt))
    for nm, o, rf, g, fn in zip(names, outs, refs, gated, fns):
      close(nm + case, o, rf, bf16_bound(rf, R.floor_of(fn), 4, np.abs(rf) + g, g))
    # +-100: the output IS one of the inputs (or 0), bit for bit
    hard = np.abs(att[:, :Fh] - att[:, Fh:]) > 90
    pick1 = (att[:, Fh:] > att[:, :Fh])[:, None, :] & np.ones((N, HW, Fh), bool)
    hm = hard[:, None, :] & np.ones((N, HW, Fh), bool)
    exact('sk_select_fwd hard gates ' + case, outs[0][hm], np.where(pick1, f64[:, :, Fh:], f64[:, :, :Fh])[hm])
    em = (np.abs(e) == 100)[:, None, :] & np.ones((N, HW, C), bool)
    exact('se_scale_fwd hard gates ' + case, outs[2][em], np.where(e[:, None, :] > 0, x.astype(F64), 0.0)[em])


# ---- the fused SK unit ----------------------------------------------------------------------------------------------------------
def _fused_grid(N, HW, Fh):
  """forward, statistics and apply on inputs where everything is exact and a fifth of t = y scale + shift is exactly 0"""
  C2 = 2 * Fh
  r = R.rng(51, N, HW, Fh)
  y, scale, shift, att = P.fused_grid_inputs(r, N, HW, Fh)
  dv = P.grid(r, (N, HW, Fh))
  ds0 = np.zeros((N, Fh), F32)           # ds / HW is not exact
  mean = P.grid(r, (C2,))
  invstd = (F32(2.0) ** r.integers(-1, 2, C2)).astype(F32)
  cA, cB, cC = (F32(2.0) ** r.integers(-1, 2, C2)).astype(F32), (F32(2.0) ** r.integers(-2, 1, C2)).astype(F32), P.grid(r, (C2,))
  case = 'fused grid N=%d HW=%d F=%d ' % (N, HW, Fh)
  f, m = P.sk_fused_f(y, scale, shift)
  t = y.astype(F64) * scale + shift
  assert (t == 0).mean() >= 0.2 and not m[t == 0].any()
  _, v_ref, mst_ref = P.sk_fused_fwd(y, scale, shift, att)
  s_bits = P.mean_of_exact_sum((f[:, :, :Fh] + f[:, :, Fh:]).sum(1), HW)
  yd, scd, shd, attd, md, isd = In(y), dev(scale), dev(shift), dev(att), dev(mean), dev(invstd)
  args = (yd.p, ptr(scd), ptr(shd))
  # pooled sum, with and without statistics, and the un-fused kernel on the materialised f
  s, s2, s3, mst = Out((N, Fh), BF), Out((N, Fh), BF), Out((N, Fh), BF), Out((N, 2, C2), TF32)
  call('asm_sk_gap_bn', *args, s.p, N, HW, Fh)
  call('asm_sk_gap_bn_stats', *args, ptr(md), ptr(isd), s2.p, mst.p, N, HW, Fh)
  call('asm_sk_gap', In(f).p, s3.p, N, HW, Fh)
  same(case + 's', s.np(), s_bits)
  same(case + 's (stats)', s2.np(), s_bits)
  exact(case + 's == sk_gap(f)', s.np(), s3.np())
  exact(case + 'mask counts, sum [t>0] y', mst.np(), mst_ref)
  # select
  v, v2 = Out((N, HW, Fh), BF), Out((N, HW, Fh), BF)
  call('asm_sk_select_bn_fwd', *args, ptr(attd), v.p, N, HW, Fh)
  call('asm_sk_select_fwd', In(f).p, ptr(attd), v2.p, N, HW, Fh)
  same(case + 'V', v.np(), v_ref)
  exact(case + 'V == sk_select(f)', v.np(), v2.np())
  # gate gradient and gradient statistics
  b = P.sk_fused_bwd(y, scale, shift, np.ones(C2), mean, invstd, att, dv, ds0)
  dvd, dsd = In(dv), In(ds0)
  datt, datt2, gst = Out((N, C2), BF), Out((N, C2), BF), Out((N, 2, C2), TF32)
  call('asm_sk_select_bn_bwd_att', *args, dvd.p, ptr(attd), datt.p, N, HW, Fh)
  call('asm_sk_select_bn_bwd_att_stats', *args, ptr(md), ptr(isd), dvd.p, ptr(attd), datt2.p, gst.p, N, HW, Fh)
  same(case + 'datt', datt.np(), b['datt'])
  same(case + 'datt (stats)', datt2.np(), b['datt'])
  exact(case + 'sum [t>0] dV, sum [t>0] dV y', gst.np(), b['gstats'])
  # reduce: per-chunk partial sums of dz and dz xhat, exact here; apply with given coefficients
  blocks = _abi_blocks(N, HW, Fh)
  part, dy = Out((blocks, 2, C2), TF32), Out((N, HW, C2), BF)
  call('asm_sk_bn_bwd_reduce', dvd.p, ptr(attd), dsd.p, yd.p, ptr(scd), ptr(shd), ptr(md), ptr(isd), N, HW, Fh, part.p)
  exact(case + 'reduce', part.np().sum(0), flush(np.stack([b['dbeta'], (b['dz'] * b['xhat']).sum((0, 1))])))
  call('asm_sk_bn_bwd_apply', dvd.p, ptr(attd), dsd.p, yd.p, ptr(scd), ptr(shd), ptr(dev(cA)), ptr(dev(cB)), ptr(dev(cC)),
       dy.p, N, HW, Fh)
  same(case + 'dy = A dz + B y + C', dy.np(), cA.astype(F64) * b['dz'] + cB.astype(F64) * y + cC)


def _abi_blocks(N, HW, Fh):
  from assembled_cnn_amd import ops
  blocks = ops.L().asm_sk_bn_bwd_blocks(N, HW, Fh)
  rpb = 256 // (2 * Fh // 8)
  rows = -(-HW // max(1024 // N, 1))
  rows = max(-(-rows // rpb) * rpb, 4 * rpb)
  assert blocks == N * -(-HW // rows), 'sk_bn_bwd_blocks'
  return blocks


def _fused_random(N, HW, Fh):
  """dy, dgamma and dbeta through both chains: statistics -> finalize -> apply, and reduce (-> bn_bwd_finalize) -> apply"""
  C2, M = 2 * Fh, N * HW
  d = P.fused_random_inputs(R.rng(52, N, HW, Fh), N, HW, Fh)
  case = 'fused random N=%d HW=%d F=%d ' % (N, HW, Fh)
  fn = lambda dt: P.sk_fused_bwd(d['y'], d['scale'], d['shift'], d['gamma'], d['mean'], d['invstd'], d['att'], d['dv'],  # noqa: E731
                                 d['ds'], dt)
  b = fn(F64)
  floor = R.floor_of(lambda dt: fn(dt)['dy'])
  # what the bounds are made of (all from the inputs and the reference)
  y64, mu, isd, g64 = d['y'].astype(F64), d['mean'].astype(F64), d['invstd'].astype(F64), d['gamma'].astype(F64)
  # what the gates multiply: [t > 0] |dV| (a1 = 1 - a0 is formed in float32: its error is absolute, not relative to a1)
  gated = np.where(P.sk_fused_f(d['y'], d['scale'], d['shift'])[1], np.abs(np.concatenate([d['dv'], d['dv']], 2)), 0.0)
  abs_dz = np.abs(b['dz'])
  # dbeta: a float32 sum of M terms dz (summed per image in float32, across images in float64); + 8: the roundings of
  # 1 / HW, ds / HW, the gate, a_b dV, the two products and the sum of the finalize, mean * w and the cast of the result
  e_db = (M + 8) * R.U24 * abs_dz.sum((0, 1)) + 1e-4 * gated.sum((0, 1))
  # dgamma: the kernels sum dz y and subtract mean sum dz (the factorised form of the header), times invstd
  terms_dg = isd * ((abs_dz * np.abs(y64)).sum((0, 1)) + np.abs(mu) * abs_dz.sum((0, 1)))
  e_dg = (M + 8) * R.U24 * terms_dg + 1e-4 * isd * ((gated * np.abs(y64)).sum((0, 1)) + np.abs(mu) * gated.sum((0, 1)))
  # dy = A dz + B y + C in float32 from coefficients that carry e_db and e_dg, rounded to bf16
  A = g64 * isd
  Bc = A * isd * np.abs(b['dgamma']) / M
  mags = A * abs_dz + Bc * (np.abs(y64) + np.abs(mu)) + A * np.abs(b['dbeta']) / M
  extra = A * (1e-4 * gated + (e_db + np.abs(b['xhat']) * e_dg) / M) + 6 * R.U24 * mags
  dy_bound = R.BF16_ULP * np.abs(b['dy']) + 4.0 * floor + extra

  yd, dvd, dsd = In(d['y']), In(d['dv']), In(d['ds'])
  scd, shd, attd, md, isdd, gd = (dev(d[k]) for k in ('scale', 'shift', 'att', 'mean', 'invstd', 'gamma'))
  s, datt = Out((N, Fh), BF), Out((N, C2), BF)
  mst, gst = Out((N, 2, C2), TF32), Out((N, 2, C2), TF32)
  call('asm_sk_gap_bn_stats', yd.p, ptr(scd), ptr(shd), ptr(md), ptr(isdd), s.p, mst.p, N, HW, Fh)
  call('asm_sk_select_bn_bwd_att_stats', yd.p, ptr(scd), ptr(shd), ptr(md), ptr(isdd), dvd.p, ptr(attd), datt.p, gst.p, N, HW,
       Fh)
  s.np(), datt.np()
  exact(case + 'mask counts', mst.np()[:, 0], P.sk_fused_fwd(d['y'], d['scale'], d['shift'], d['att'])[2][:, 0])

  def apply(co):
    dy = Out((N, HW, C2), BF)
    call('asm_sk_bn_bwd_apply', dvd.p, ptr(attd), dsd.p, yd.p, ptr(scd), ptr(shd), co[0].p, co[1].p, co[2].p, dy.p, N, HW, Fh)
    return dy.np()

  dg, db, co = Out((C2,), TF32), Out((C2,), TF32), [Out((C2,), TF32) for _ in range(3)]
  call('asm_sk_bn_bwd_finalize', gst.p, mst.p, ptr(attd), dsd.p, N, HW, Fh, ptr(gd), ptr(md), ptr(isdd), dg.p, db.p, co[0].p,
       co[1].p, co[2].p)
  close(case + 'dbeta (statistics)', db.np(), b['dbeta'], e_db)
  close(case + 'dgamma (statistics)', dg.np(), b['dgamma'], e_dg)
  close(case + 'dy (statistics)', apply(co), b['dy'], dy_bound)

  blocks = _abi_blocks(N, HW, Fh)
  part = Out((blocks, 2, C2), TF32)
  call('asm_sk_bn_bwd_reduce', dvd.p, ptr(attd), dsd.p, yd.p, ptr(scd), ptr(shd), ptr(md), ptr(isdd), N, HW, Fh, part.p)
  ps = part.np().sum(0)
  e_dg_direct = (M + 8) * R.U24 * (abs_dz * np.abs(b['xhat'])).sum((0, 1)) + 1e-4 * (gated * np.abs(b['xhat'])).sum((0, 1))
  close(case + 'sum dz (reduce)', ps[0], b['dbeta'], e_db)
  close(case + 'sum dz xhat (reduce)', ps[1], b['dgamma'], e_dg_direct + 4 * R.U24 * terms_dg)
  if blocks <= 1024:       # more partial rows than that are compacted first (bn.hip's own tests)
    dg, db, co = Out((C2,), TF32), Out((C2,), TF32), [Out((C2,), TF32) for _ in range(3)]
    call('asm_bn_bwd_finalize', part.p, blocks, M, C2, ptr(gd), ptr(md), ptr(isdd), dg.p, db.p, co[0].p, co[1].p, co[2].p)
    close(case + 'dbeta (reduce)', db.np(), b['dbeta'], e_db)
    close(case + 'dgamma (reduce)', dg.np(), b['dgamma'], e_dg)
    close(case + 'dy (reduce)', apply(co), b['dy'], dy_bound)


@pytest.mark.parametrize('N,HW,Fh', P.FUSED_CASES)
def test_fused_sk_geometry_and_zero_mask(hip_lib, N, HW, Fh):
  """make_geom and the launcher of sk_select_bn_fwd: rpb = 256 / vector columns (85 and 42 row lanes with idle threads at
  F = 24, one row lane at F = 1024), rows_per_chunk >= 4 rpb, the clamped second in-flight row, a second chunk of one row, a
  chunk count of zero clamped to 1 (N = 1025); image_pass_vcb of 3 and 5 (LDS path of lane_sum8), 1 and 8 (shuffle path); the
  1024-thread variants from HW = 512.  t == 0 exactly on a fifth of the elements: masked out in the forward, the statistics
  and the apply pass alike"""
  _fused_grid(N, HW, Fh)
  _fused_random(N, HW, Fh)


def test_fused_sk_refuses_more_than_256_vector_columns(hip_lib):
  """F = 1032: 2F / 8 = 258 vector columns do not fit the 256-thread block of the chunked passes"""
  N, HW, Fh = 1, 3, 1032
  r = R.rng(53)
  y, scale, shift, att = P.fused_grid_inputs(r, N, HW, Fh)
  yd, scd, shd, attd = In(y), dev(scale), dev(shift), dev(att)
  dvd, dsd = In(P.grid(r, (N, HW, Fh))), In(P.grid(r, (N, Fh)))
  s, v, datt, dy = Out((N, Fh), BF), Out((N, HW, Fh), BF), Out((N, 2 * Fh), BF), Out((N, HW, 2 * Fh), BF)
  part = Out((4, 2, 2 * Fh), TF32)
  refused('asm_sk_gap_bn', yd.p, ptr(scd), ptr(shd), s.p, N, HW, Fh)
  refused('asm_sk_select_bn_fwd', yd.p, ptr(scd), ptr(shd), ptr(attd), v.p, N, HW, Fh)
  refused('asm_sk_select_bn_bwd_att', yd.p, ptr(scd), ptr(shd), dvd.p, ptr(attd), datt.p, N, HW, Fh)
  refused('asm_sk_bn_bwd_reduce', dvd.p, ptr(attd), dsd.p, yd.p, ptr(scd), ptr(shd), ptr(scd), ptr(scd), N, HW, Fh, part.p)
  refused('asm_sk_bn_bwd_apply', dvd.p, ptr(attd), dsd.p, yd.p, ptr(scd), ptr(shd), ptr(scd), ptr(scd), ptr(scd), dy.p, N, HW,
          Fh)
  from assembled_cnn_amd import ops
  assert ops.L().asm_sk_bn_bwd_blocks(N, HW, Fh) < 0
  torch.cuda.synchronize()
  assert all(untouched(o) for o in (s, v, datt, dy, part))
