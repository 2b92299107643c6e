"""Guard-band plumbing and element-wise bounds shared by the GPU edge-shape modules (tests/test_gpu_rows_edges.py,
tests/test_gpu_pool_edges.py, tests/test_gpu_bn_edges.py, tests/test_gpu_step_edges.py, tests/test_gpu_conv_exact.py,
tests/test_gpu_retrieval_edges.py).  A plain module, not a conftest: the test modules import what they use, the autouse fixture
``_release_inputs`` included.

* ``Out``: an output between two 4 KiB flanks of the byte 0xA5 which must survive the call; the output itself starts as 0xA5,
  so an element the kernel skips shows.  ``Out.np()`` rejects NaN and huge values; ``Out.np_inf()`` admits the infinities
  of a top-K output (-inf in an unused slot) and rejects an element that still holds the fill.
* ``In``: an input between two 4 KiB flanks of NaN (or a huge value where the kernel would drop a NaN silently): a read one
  row or one vector outside the tensor shows up in an output, where ``Out.np()`` rejects it.
* ``close_*`` / ``exact``: element-wise assertions; each prints the worst error of its case next to its bound under ``-s``.
"""
import numpy as np
import pytest
import torch

from tests import rows_ref as R

BF = torch.bfloat16
DEV = 'cuda'
FLANK = 4096
PATTERN = 0xA5


def _abi():
  from assembled_cnn_amd import ops
  return ops


def call(name, *args):
  ops = _abi()
  ops.check(getattr(ops.L(), name)(*args, ops._stream()), name)


def ptr(t):
  return _abi()._ptr(t)


class Out(object):
  """``shape`` elements of ``dtype`` between two 4 KiB flanks of one allocation, all bytes 0xA5 before the call"""

  def __init__(self, shape, dtype, init=None):
    n = int(np.prod(shape))
    self.pad = FLANK // torch.empty((), dtype=dtype).element_size()
    self.buf = torch.empty(n + 2 * self.pad, dtype=dtype, device=DEV)
    self.buf.view(torch.uint8).fill_(PATTERN)
    self.t = self.buf[self.pad:self.pad + n].view(*shape)
    if init is not None:
      self.t.copy_(init)

  @property
  def p(self):
    return ptr(self.t)

  def check_flanks(self):
    raw = self.buf.view(torch.uint8)
    assert bool((raw[:FLANK] == PATTERN).all()) and bool((raw[-FLANK:] == PATTERN).all()), 'a flank was written'

  def np(self):
    """flanks intact -> the output as float64 (int64 for integer outputs); NaN and huge values are failures"""
    self.check_flanks()
    a = self.t.detach().cpu()
    if a.dtype in (torch.int32, torch.uint8):
      return a.numpy().astype(np.int64)
    a = a.double().numpy()
    assert np.isfinite(a).all() and (np.abs(a) < 1e29).all() if a.size else True, 'NaN or huge value in an output'
    return a

  def assert_written(self):
    """no 4-byte element still holds the fill: 0xA5A5A5A5 is the float -2.9e-16 / the int32 -1515870811"""
    assert self.t.element_size() == 4
    words = self.t.contiguous().view(torch.uint8).view(-1, self.t.element_size())
    assert not bool((words == PATTERN).all(1).any()), 'an output element was never written'

  def np_inf(self):
    """``np`` for an output that legitimately holds infinities (the -inf of an unused top-K slot): flanks intact, every
    element written, no NaN and no huge finite value -> float64 (int64 for integer outputs)"""
    self.check_flanks()
    self.assert_written()
    a = self.t.detach().cpu()
    if a.dtype in (torch.int32, torch.uint8):
      return a.numpy().astype(np.int64)
    a = a.double().numpy()
    assert not np.isnan(a).any() and (np.abs(a[np.isfinite(a)]) < 1e29).all(), 'NaN or huge value in an output'
    return a


class Work(Out):
  """a workspace of exactly ``nbytes`` bytes between the flanks; ``p`` is a null pointer for an empty one.  The kernel may
  leave anything inside; ``check_flanks`` tells whether it stayed inside."""

  def __init__(self, nbytes):
    Out.__init__(self, (int(nbytes),), torch.uint8)
    self.nbytes = int(nbytes)

  @property
  def p(self):
    return ptr(self.t) if self.nbytes else 0


def dev(a, dtype=torch.float32):
  """numpy -> device tensor (bf16: the values are bf16 already or get rounded here)"""
  t = torch.from_numpy(np.ascontiguousarray(a))
  if dtype == BF:
    t = t.float()
  t = t.to(dtype).to(DEV)
  _ALIVE.append(t)        # an input handed over as a bare pointer must outlive the call
  return t


_ALIVE = []


@pytest.fixture(autouse=True)
def _release_inputs():
  yield
  del _ALIVE[:]


class In(object):
  """``array`` as ``dtype`` between two 4 KiB flanks of one allocation that hold ``flank_value``: bf16 NaN in general, +1e30
  for an input of the max pool (``f > best`` drops a NaN silently), an impossible code (0xFF) for a byte mask.  The kernel
  gets the pointer ``p`` of the inner tensor ``t``; the allocation lives until the end of the test."""

  def __init__(self, array, dtype=BF, flank_value=float('nan')):
    a = torch.from_numpy(np.ascontiguousarray(array))
    if dtype == BF:
      a = a.float()
    n = a.numel()
    self.pad = FLANK // torch.empty((), dtype=dtype).element_size()
    self.buf = torch.full((n + 2 * self.pad,), flank_value, dtype=dtype, device=DEV)
    self.t = self.buf[self.pad:self.pad + n].view(*a.shape) if n else self.buf[self.pad:self.pad]
    self.t.copy_(a.to(dtype))
    _ALIVE.append(self.buf)

  @property
  def p(self):
    return ptr(self.t)


# ---- bounds -------------------------------------------------------------------------------------------------------------
def _report(case, err, bound):
  worst = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
  print('\nrows-edges %-46s worst |err| %.3e = %.3f of its bound' % (case, float(err.max()) if err.size else 0.0, worst), end='')


def close_bf16(case, out, ref, floor):
  out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
  err, bound = np.abs(out - ref), R.BF16_ULP * np.abs(ref) + 4.0 * floor
  _report(case, err, bound)
  print('  (reference floor %.3e)' % floor, end='')
  assert (err <= bound).all(), '%s: |err| %.3e at %s' % (case, err.max(), np.unravel_index(np.argmax(err - bound), err.shape))


def close_sum(case, out, ref, n, sum_abs):
  out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
  err, bound = np.abs(out - ref), n * R.U24 * np.asarray(sum_abs, np.float64) + np.zeros_like(ref)
  _report(case, err, bound)
  assert (err <= bound).all(), '%s: |err| %.3e, bound %.3e' % (case, err.max(), bound.max())


def close_rel(case, out, ref):
  out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
  err, bound = np.abs(out - ref), 1e-4 * np.abs(ref) + 1e-8
  _report(case, err, bound)
  assert (err <= bound).all(), '%s: |err| %.3e' % (case, err.max())


def close_ulp(case, out, ref, ulps=1):
  """the float32 nearest the float64 reference, give or take ``ulps``"""
  r32 = np.asarray(ref, np.float64).astype(np.float32)
  err, bound = np.abs(np.asarray(out, np.float64) - r32.astype(np.float64)), ulps * R.ulp32(r32)
  _report(case, err, bound)
  assert (err <= bound).all(), '%s: %.2f ulp' % (case, float(np.max(err / bound)))


def close_terms(case, out, terms, roundings):
  """a float32 expression the kernel evaluates from already rounded float32 values: ``roundings`` half-ulps of the sum of the
  magnitudes of its terms"""
  ref = sum(terms)
  err, bound = np.abs(np.asarray(out, np.float64) - ref), roundings * R.U24 * sum(np.abs(t) for t in terms)
  _report(case, err, bound)
  assert (err <= bound).all(), '%s: |err| %.3e, bound %.3e' % (case, err.max(), bound.max())


def exact(case, out, ref):
  out, ref = np.asarray(out), np.asarray(ref)
  assert out.shape == ref.shape and np.array_equal(out, ref), \
      '%s: %d of %d elements differ' % (case, int((out != ref).sum()) if out.shape == ref.shape else -1, ref.size)
