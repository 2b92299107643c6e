"""Edge shapes and guard bands of the kernels that open and close a training step (csrc/misc.hip): asm_mixup_meansub with its
two uint8 paths and its float32 path, asm_mixup_labels, asm_stem_pad_input, and asm_sgd_momentum, against the plain float64
references of tests/rows_ref.py (mixup_meansub, mixup_terms, stem_pad, sgd_terms), which tests/test_rows_ref_cpu.py proves
against the oracle on the CPU.  The rules are those of tests/test_gpu_rows_edges.py: element-wise bounds only, every output
between two flanks of 0xA5 and pre-filled with 0xA5, every input between two flanks."""
import numpy as np
import pytest
import torch

from tests import gpu_guard
from tests import rows_ref as R
from tests.gpu_guard import (BF, DEV, FLANK, PATTERN, In, Out, _abi, _release_inputs, call, close_bf16,  # noqa: F401
                             close_terms, exact, ptr)
from tests.test_gpu_rows_edges import _grid_cap

pytestmark = pytest.mark.gpu

F32 = torch.float32
U8 = torch.uint8


# ---- mixup + mean subtraction + stem halo ------------------------------------------------------------------------------------
def _u8_image(img, misalign):
  """the uint8 pixels inside a larger allocation of 0xFF bytes, at a 4-byte aligned address or one byte past one"""
  flat = torch.from_numpy(np.ascontiguousarray(img.astype(np.uint8))).reshape(-1)
  buf = torch.full((flat.numel() + 2 * FLANK + 4,), 0xFF, dtype=U8, device=DEV)
  t = buf[FLANK + misalign:FLANK + misalign + flat.numel()]
  t.copy_(flat)
  gpu_guard._ALIVE.append(buf)
  assert t.data_ptr() % 4 == misalign
  return t


def _lams(half, kind):
  if kind == 'mixed':       # 0, 1 and 0.5 among them wherever the batch has room
    return np.array([0.0, 1.0, 0.5][:half] if half > 1 else [0.7], np.float32), np.array([1.0, 0.3, 0.0][:half], np.float32)
  v = 1.0 if kind == 'one' else 0.0
  return np.full(half, v, np.float32), np.full(half, v, np.float32)


@pytest.mark.parametrize('mixup_type,Bin', [(0, 2), (0, 3), (0, 6), (1, 2), (1, 6), (2, 2), (2, 6)])
@pytest.mark.parametrize('H,W', [(1, 4), (3, 5), (5, 8), (2, 260)])
def test_mixup_meansub_three_ways(hip_lib, H, W, Bin, mixup_type):
  """the same pixels as an aligned uint8 tensor (the rows kernel when W % 4 == 0), as a uint8 view one byte into an allocation
  (the per-pixel kernel) and as float32: equal bits, each within one bf16 ulp + 4 floors of the float64 reference, halo and
  fourth channel all-zero bits.  W = 260: 65 quads and 266 padded pixels, a second trip of both loops of the rows kernel.
  lambda = 1 gives the unmixed first operand and lambda = 0 the second, exactly."""
  r = R.rng(401, H, W, Bin, mixup_type)
  img = r.integers(0, 256, (Bin, H, W, 3)).astype(np.float32)
  img.reshape(-1)[::17] = 255.0
  img.reshape(-1)[5::19] = 0.0
  Bout = Bin // 2 if mixup_type == 1 else Bin
  srcs = (('u8 aligned', _u8_image(img, 0), 1), ('u8 + 1 byte', _u8_image(img, 1), 1), ('float32', In(img, F32).t, 0))
  inside = np.zeros((Bout, H + 6, W + 6, 4), bool)
  inside[:, 3:3 + H, 3:3 + W, :3] = True
  for kind in (('mixed', 'one', 'zero') if mixup_type else ('mixed',)):
    lam1, lam2 = _lams(Bin // 2, kind)
    l1 = In(lam1, F32) if mixup_type else None
    l2 = In(lam2, F32) if mixup_type == 2 else None
    ref = R.mixup_meansub(img, mixup_type, lam1, lam2)
    floor = R.floor_of(lambda dt: R.mixup_meansub(img, mixup_type, lam1, lam2, dt))
    bits = []
    for name, src, is_u8 in srcs:
      out = Out((Bout, H + 6, W + 6, 4), BF)
      call('asm_mixup_meansub', ptr(src), is_u8, Bin, H, W, mixup_type, l1.p if l1 else None, l2.p if l2 else None, out.p)
      case = 'mixup_meansub %s type %d Bin=%d %dx%d lam %s' % (name, mixup_type, Bin, H, W, kind)
      got = out.np()
      close_bf16(case, got, ref, floor)
      raw = out.t.view(torch.int16).cpu().numpy()
      assert (raw[~inside] == 0).all(), case + ': halo and fourth channel must be all-zero bits'
      if kind != 'mixed' or mixup_type == 0:
        fa, fb, _ = R.mixup_operands(img, mixup_type, lam1, lam2)
        exact(case + ': the unmixed operand', got, R.to_bf16(R.mixup_meansub(fb if kind == 'zero' else fa, 0)).astype(np.float64))
      bits.append(raw)
    assert np.array_equal(bits[0], bits[1]) and np.array_equal(bits[0], bits[2]), 'the three input forms differ'


@pytest.mark.parametrize('C', [1, 11, 1001])
def test_mixup_labels(hip_lib, C):
  """lam a + (1 - lam) b from float32 values: (1 - lam), two products and the sum, of which a product may be fused into the
  sum -- at most 3 half-ulps of |lam a| + |(1 - lam) b| either way (the rounding of 1 - lam scales the second term alone)"""
  for mixup_type, Bin in ((0, 3), (0, 6), (1, 2), (1, 6), (2, 2), (2, 6)):
    r = R.rng(402, C, mixup_type, Bin)
    y = r.random((Bin, C)).astype(np.float32)
    y[np.arange(Bin), r.integers(0, C, Bin)] = 1.0
    lam1, lam2 = _lams(Bin // 2, 'mixed')
    Bout = Bin // 2 if mixup_type == 1 else Bin
    out = Out((Bout, C), F32)
    call('asm_mixup_labels', In(y, F32).p, Bin, C, mixup_type, In(lam1, F32).p if mixup_type else None,
         In(lam2, F32).p if mixup_type == 2 else None, out.p)
    case = 'mixup_labels type %d Bin=%d C=%d' % (mixup_type, Bin, C)
    terms = R.mixup_terms(y, mixup_type, lam1, lam2)
    if mixup_type == 0:
      exact(case, out.np(), terms[0])
    else:
      close_terms(case, out.np(), terms, 3)


@pytest.mark.parametrize('N,H,W', [(2, 1, 4), (3, 3, 5), (1, 2, 260)])
def test_stem_pad_input(hip_lib, N, H, W):
  """float32 and bf16 images -> bf16 with the stem's zero halo and zero fourth channel: equal bits"""
  x = (R.rng(403, N, H, W).standard_normal((N, H, W, 3)) * 50).astype(np.float32)
  for name, src, is_f32 in (('float32', In(x, F32), 1), ('bf16', In(R.to_bf16(x), BF), 0)):
    out = Out((N, H + 6, W + 6, 4), BF)
    call('asm_stem_pad_input', src.p, is_f32, out.p, N, H, W)
    ref = R.stem_pad(R.to_bf16(x))
    exact('stem_pad_input %s %dx%dx%d' % (name, N, H, W), out.np(), ref.astype(np.float64))
    assert (out.t.view(torch.int16).cpu().numpy()[ref == 0] == 0).all()


# ---- SGD with momentum -------------------------------------------------------------------------------------------------------------
def _second_trip_n():
  """four elements per thread: one vector more than a full grid of the capped launcher, plus a scalar tail of 3"""
  return 4 * (_grid_cap() * 256 + 1) + 3


SGD_N = [1, 3, 4, 5, 1023, 1024, 1027, 4 * (2 ** 20 + 1) + 3, 'second trip']


@pytest.mark.parametrize('n', SGD_N)
def test_sgd_momentum_lengths_and_forms(hip_lib, n):
  """the vector loop, its scalar tail and (the last length: more vectors than the capped grid has threads) a second
  grid-stride trip; with and without the bf16 shadow, weight decay 1e-4 and 0, gradient scale 1 and 1 / 128.

  Roundings of sgd_kernel's expression, each at most half a float32 ulp of the sum of the magnitudes of the terms, whether or
  not the compiler fuses a product into its add (a fused product is one rounding fewer):
    a' = mom * a + (g * gs + wd * w): g gs, wd w, their sum, mom a, the sum                       -> 5 on (mom a, g gs, wd w)
    w' = w - lr * a': the 5 of a' scaled by lr, lr a', the difference                             -> 7 on (w, -lr mom a, -lr g gs, -lr wd w)
  w_bf16 is the bf16 rounding of the kernel's own w', bit for bit.  Elements past n keep their bits (the flanks)."""
  if n == 'second trip':
    n = _second_trip_n()
    assert -(-(n // 4) // 256) > _grid_cap()
  r = R.rng(404, n)
  w0, a0 = r.standard_normal(n).astype(np.float32), (r.standard_normal(n) * 0.1).astype(np.float32)
  g0 = r.standard_normal(n).astype(np.float32)
  w0[::3] *= np.float32(1e-3)               # small weights: the weight-decay term must still be wd * w
  for gs in (1.0, 1.0 / 128):
    g = In(g0 / np.float32(gs), F32)
    gnp = (g0 / np.float32(gs)).astype(np.float32)
    for wd in (1e-4, 0.0):
      ta, tw = R.sgd_terms(w0, a0, gnp, 0.1, 0.9, wd, gs)
      for shadow in (True, False):
        w, a = Out((n,), F32, init=In(w0, F32).t), Out((n,), F32, init=In(a0, F32).t)
        wb = Out((n,), BF)
        call('asm_sgd_momentum', w.p, a.p, g.p, wb.p if shadow else None, n, 0.1, 0.9, wd, gs)
        case = 'sgd n=%d wd=%g gs=%g shadow %d ' % (n, wd, gs, shadow)
        close_terms(case + 'accum', a.np(), ta, 5)
        wk = w.np()
        close_terms(case + 'w', wk, tw, 7)
        if shadow:
          exact(case + 'w_bf16', wb.np(), R.to_bf16(wk.astype(np.float32)).astype(np.float64))
        else:
          wb.check_flanks()
          assert bool((wb.t.view(U8) == PATTERN).all()), case + ': no shadow was asked for'


@pytest.mark.parametrize('n', [1, 5, 1027])
def test_sgd_momentum_dyadic_is_exact(hip_lib, n):
  """weight decay 0, gradient scale 1, momentum 0.5, lr 0.25 on multiples of 1/8: every product and sum is exact"""
  r = R.rng(405, n)
  w0, a0, g0 = [(r.integers(-32, 33, n) / 8.0).astype(np.float32) for _ in range(3)]
  ta, tw = R.sgd_terms(w0, a0, g0, 0.25, 0.5, 0.0, 1.0)
  w, a, wb = Out((n,), F32, init=In(w0, F32).t), Out((n,), F32, init=In(a0, F32).t), Out((n,), BF)
  call('asm_sgd_momentum', w.p, a.p, In(g0, F32).p, wb.p, n, 0.25, 0.5, 0.0, 1.0)
  exact('sgd dyadic accum', a.np(), sum(ta))
  exact('sgd dyadic w', w.np(), sum(tw))
  exact('sgd dyadic w_bf16', wb.np(), R.to_bf16(sum(tw).astype(np.float32)).astype(np.float64))


def test_sgd_momentum_refusals_and_empty(hip_lib):
  """n = 0 returns OK and writes nothing; a pointer one element into an allocation (4 bytes off for w, accum, grad; 2 bytes
  off for w_bf16) is refused with ASM_EINVAL before any launch"""
  L = _abi().L()
  n = 8
  w, a, wb = Out((n + 1,), F32), Out((n + 1,), F32), Out((n + 1,), BF)
  g = In(np.ones(n + 1, np.float32), F32)
  n0 = L.asm_launch_count()
  call('asm_sgd_momentum', w.p, a.p, g.p, wb.p, 0, 0.1, 0.9, 1e-4, 1.0)
  off = {k: ptr(t[1:]) for k, t in (('w', w.t), ('a', a.t), ('g', g.t), ('wb', wb.t))}
  assert off['w'] % 16 == 4 and off['wb'] % 8 == 2
  for args in ((off['w'], a.p, g.p, wb.p), (w.p, off['a'], g.p, wb.p), (w.p, a.p, off['g'], wb.p), (w.p, a.p, g.p, off['wb']),
               (off['w'], a.p, g.p, None)):
    with pytest.raises(ValueError):
      call('asm_sgd_momentum', *args, n, 0.1, 0.9, 1e-4, 1.0)
  with pytest.raises(ValueError):
    call('asm_sgd_momentum', None, a.p, g.p, wb.p, n, 0.1, 0.9, 1e-4, 1.0)
  assert L.asm_launch_count() == n0, 'a refused or empty call launched a kernel'
  for o in (w, a, wb):
    o.check_flanks()
    assert bool((o.t.view(U8) == PATTERN).all())
