"""asm_eval_groups (csrc/eval.hip) against tests/robustness_ref.eval_groups: equal counters and equal predictions.

Rules of every case:
* the logits lie between two 4 KiB flanks of 1e30 or NaN and their pad columns C .. ld-1 hold the same poison: a read past a
  row would raise a prediction or a strictly-larger count (1e30) -- NaN is the poison the arg-max must pass over anyway;
* counters and predictions are slices of larger tensors with 4 KiB of the byte 0xA5 on either side, which must survive;
* every case runs twice into fresh counters and the two results must be the same bits (integer atomics);
* logits are small integers with NaN and infinities sprinkled in, so ties at the maximum and at the top-5 boundary are the
  common case, and labels and groups reach one past either end of their range."""
import ctypes

import numpy as np
import pytest
import torch

from tests import robustness_ref as RR
from tests.gpu_guard import DEV, In, Out, _ALIVE, _release_inputs, call, dev, exact, ptr  # noqa: F401

pytestmark = pytest.mark.gpu

NAN, INF = float('nan'), float('inf')


def _case(B, C, G, seed, specials=True):
  r = np.random.default_rng(seed)
  R = 3 if C <= 64 else C // 6           # a few equal values per level whatever the width
  z = r.integers(-R, R + 1, (B, C)).astype(np.float32)
  if specials:                            # about 0.3 NaN, 0.3 +inf and 0.3 -inf per row
    m = r.random((B, C)) * C
    z[m < 0.3] = NAN
    z[(m >= 0.3) & (m < 0.6)] = INF
    z[(m >= 0.6) & (m < 0.9)] = -INF
  labels = r.integers(-1, C + 1, B).astype(np.int32)
  groups = r.integers(-1, G + 1, B).astype(np.int32)
  return z, labels, groups


def _padded(z, ld, poison):
  out = np.full((z.shape[0], ld), poison, np.float32)
  out[:, :z.shape[1]] = z
  return out


def _run(z, ld, labels, groups, G, poison, start=None, want_pred=True, misalign=False):
  """two runs into fresh counters -> (counts int64 [G + 1, 3], pred int64 [B] or None), the two runs compared"""
  B, C = z.shape
  zp = _padded(z, ld, poison)
  if misalign:          # a row base that is not 16-byte aligned: one float into an allocation
    buf = torch.full((zp.size + 2,), float(poison), dtype=torch.float32, device=DEV)
    buf[1:1 + zp.size].copy_(torch.from_numpy(zp.reshape(-1)))
    _ALIVE.append(buf)
    zptr = ptr(buf[1:1 + zp.size])
    assert zptr % 16 == 4
  else:
    zin = In(zp, torch.float32, flank_value=float(poison))
    zptr = zin.p
    assert zptr % 16 == 0
  lab, grp = In(labels, torch.int32, flank_value=0), In(groups, torch.int32, flank_value=0)
  runs = []
  for _ in range(2):
    counts = Out((G + 1, 3), torch.int32, init=torch.zeros((G + 1, 3), dtype=torch.int32) if start is None
                 else torch.from_numpy(np.asarray(start, np.int32)))
    pred = Out((B,), torch.int32) if want_pred else None
    call('asm_eval_groups', zptr, ld, lab.p, grp.p, B, C, G, counts.p, pred.p if want_pred else 0)
    if want_pred:
      pred.check_flanks()
      pred.assert_written()
    runs.append((counts.np(), pred.np() if want_pred else None))
  exact('second run, counts', runs[1][0], runs[0][0])
  if want_pred:
    exact('second run, pred', runs[1][1], runs[0][1])
  return runs[0]


@pytest.mark.parametrize('round_ld', [False, True], ids=['ld_eq_C', 'ld_rounded_to_8'])
@pytest.mark.parametrize('C', [1, 4, 5, 6, 63, 64, 65, 255, 256, 257, 1001])
def test_counters_and_predictions_equal_the_reference(hip_lib, C, round_ld):
  ld = (C + 7) // 8 * 8 if round_ld else C
  n = 0
  for B in (1, 3, 4, 5, 9):
    for G in (1, 95):
      poison = np.float32(1e30) if n % 2 == 0 else np.float32(NAN)
      z, labels, groups = _case(B, C, G, 1000 * C + 10 * B + G)
      want_c, want_p = RR.eval_groups(z, labels, groups, G)
      got_c, got_p = _run(z, ld, labels, groups, G, poison)
      exact('C=%d ld=%d B=%d G=%d pred' % (C, ld, B, G), got_p, want_p)
      exact('C=%d ld=%d B=%d G=%d counts' % (C, ld, B, G), got_c, want_c)
      n += 1


@pytest.mark.parametrize('C,ld', [(1000, 1000), (1001, 1008), (6, 8)])
def test_a_base_off_16_bytes_takes_the_scalar_loads(hip_lib, C, ld):
  z, labels, groups = _case(9, C, 95, 77 + C)
  want_c, want_p = RR.eval_groups(z, labels, groups, 95)
  got_c, got_p = _run(z, ld, labels, groups, 95, np.float32(1e30), misalign=True)
  exact('pred', got_p, want_p)
  exact('counts', got_c, want_c)


# (row of 7 logits, label, pred, top-1 hit, top-5 hit): the rules of include/asm_hip.h, one per line
KNOWN = [
    ([1, 7, 7, 3, 7, 0, 0], 1, 1, 1, 1),                  # ties at the maximum: the lowest index
    ([1, 7, 7, 3, 7, 0, 0], 2, 1, 0, 1),
    ([9, 9, 9, 9, 9, 1, 0], 5, 0, 0, 0),                  # five strictly larger: out of the top 5
    ([9, 9, 9, 9, 1, 1, 0], 5, 0, 0, 1),                  # four
    ([9, 9, 9, 9, 9, 9, 0], 5, 0, 0, 1),                  # five equal ones are not larger
    ([1, NAN, 5, 2, 0, 0, 0], 2, 2, 1, 1),                # a NaN at the maximum's place
    ([NAN, 1, 5, 5, 0, 0, 0], 3, 2, 0, 1),
    ([NAN, -INF, -INF, NAN, NAN, NAN, NAN], 1, 1, 1, 0),
    ([NAN] * 7, 0, -1, 0, 0),                             # a row of NaNs
    ([NAN] * 7, -1, -1, 0, 0),
    ([0, -INF, 1, 0, 0, 0, 0], 1, 2, 0, 0),               # the label's logit -inf
    ([0, INF, 1, 0, 0, 0, 0], 1, 1, 1, 0),                # and +inf: the arg-max, never in_top_k
    ([3, 2, 1, 0, 0, 0, 0], -1, 0, 0, 0),                 # labels outside [0, C)
    ([3, 2, 1, 0, 0, 0, 0], 7, 0, 0, 0),
]


@pytest.mark.parametrize('ld', [7, 8])
def test_known_answer_rows(hip_lib, ld):
  z = np.asarray([k[0] for k in KNOWN], np.float32)
  labels = np.asarray([k[1] for k in KNOWN], np.int32)
  B = len(KNOWN)
  groups = np.arange(B, dtype=np.int32)                  # one group per row: the counters show every row's hits
  want = np.zeros((B + 1, 3), np.int64)
  want[:B] = [[1, k[3], k[4]] for k in KNOWN]
  ref_c, ref_p = RR.eval_groups(z, labels, groups, B)
  assert np.array_equal(ref_c, want) and ref_p.tolist() == [k[2] for k in KNOWN]
  got_c, got_p = _run(z, ld, labels, groups, B, np.float32(1e30))
  exact('known pred', got_p, ref_p)
  exact('known counts', got_c, want)
  # a group of -1 and of G: one image each in row G, no hit although both rows would hit
  z2 = np.asarray([[5, 1, 0], [5, 1, 0], [5, 1, 0]], np.float32)
  got_c, got_p = _run(z2, 3, np.zeros(3, np.int32), np.asarray([-1, 2, 1], np.int32), 2, np.float32(NAN))
  exact('stray groups', got_c, [[0, 0, 0], [1, 1, 1], [2, 0, 0]])
  exact('stray groups pred', got_p, [0, 0, 0])


@pytest.mark.parametrize('pad,misalign', [(3, False), (3, True), (2, False)], ids=['vector', 'scalar_base_off_16', 'scalar_ld'])
@pytest.mark.parametrize('C', [5, 257])
def test_the_two_tails_agree(hip_lib, C, pad, misalign):
  """asm_eval_rows and asm_eval_groups (one arg-max rule, csrc/eval.hip) on the same logits: B = 7 rows, so the second
  workgroup of four holds three; seeded normal logits, one row with its maximum twice, one label outside [0, C).  ld = C + 3
  (8, 260) on a 16-byte aligned base takes the 16-byte loads; the same ld on a base off 16 bytes and ld = C + 2 take the
  scalar ones.  Equal predictions, and with every row in group 0 the counters are {7, sum top1, sum top5} of asm_eval_rows."""
  B, ld = 7, C + pad
  r = np.random.default_rng(500 + C)
  z = r.standard_normal((B, C)).astype(np.float32)
  z[3, 1] = z[3, C - 2] = 9.0                                   # the tie row: the lower index must win in both
  labels = np.argmax(z, axis=1).astype(np.int32)
  labels[1::2] = r.integers(0, C, labels[1::2].size)
  labels[3], labels[5] = 1, C                                   # a hit on the tie row; a label outside [0, C)
  groups = np.zeros(B, np.int32)
  zp = _padded(z, ld, np.float32(1e30)).reshape(-1)
  buf = torch.full((zp.size + 8,), 1e30, dtype=torch.float32, device=DEV)
  off = 5 if misalign else 4
  zt = buf[off:off + zp.size]
  zt.copy_(torch.from_numpy(zp))
  assert ptr(zt) % 16 == (4 if misalign else 0)
  lab, grp = In(labels, torch.int32, flank_value=0), In(groups, torch.int32, flank_value=0)
  pred_r, conf, top1, top5 = Out((B,), torch.int32), Out((B,), torch.float32), Out((B,), torch.float32), Out((B,), torch.float32)
  call('asm_eval_rows', ptr(zt), ld, lab.p, B, C, pred_r.p, conf.p, top1.p, top5.p)
  counts, pred_g = Out((2, 3), torch.int32, init=torch.zeros((2, 3), dtype=torch.int32)), Out((B,), torch.int32)
  call('asm_eval_groups', ptr(zt), ld, lab.p, grp.p, B, C, 1, counts.p, pred_g.p)
  conf.np()
  p, t1, t5 = pred_r.np(), top1.np(), top5.np()
  assert p[3] == 1 and t1[3] == 1 and t1[5] == 0 and t5[5] == 0 and 0 < t1.sum() < B
  exact('pred of the two tails', pred_g.np(), p)
  exact('counters', counts.np(), [[B, int(t1.sum()), int(t5.sum())], [0, 0, 0]])


def test_null_pred_and_counters_that_start_non_zero(hip_lib):
  z, labels, groups = _case(9, 65, 5, 5)
  start = np.arange(18, dtype=np.int64).reshape(6, 3) * 1000 + 7
  want_c, _ = RR.eval_groups(z, labels, groups, 5, counts=start)
  got_c, got_p = _run(z, 72, labels, groups, 5, np.float32(1e30), start=start, want_pred=False)
  assert got_p is None
  exact('accumulated counts', got_c, want_c)
  assert (want_c >= start).all() and want_c[:, 0].sum() == start[:, 0].sum() + 9


@pytest.fixture(scope='module')
def big():
  """B = 1031 rows of 1001 classes, computed once: logits, labels, and the reference's per-row outcome"""
  B, C = 1031, 1001
  z, labels, _ = _case(B, C, 95, 31)
  r = np.random.default_rng(32)
  top = np.nanargmax(np.where(np.isnan(z), -np.inf, z), axis=1)
  labels = np.where(r.random(B) < 0.5, top, labels).astype(np.int32)        # half the rows are top-1 hits
  per_row, pred = RR.eval_groups(z, labels, np.arange(B), B)                # group b = row b
  return z, labels, per_row[:B], pred


def test_1031_rows_with_random_groups(hip_lib, big):
  z, labels, per_row, pred = big
  groups = np.random.default_rng(33).integers(-1, 96, z.shape[0]).astype(np.int32)
  want = np.zeros((96, 3), np.int64)
  for b, g in enumerate(groups):
    if 0 <= g < 95:
      want[g] += per_row[b]
    else:
      want[95, 0] += 1
  assert want[:95, 1].sum() > 400 and want[95, 0] > 0
  got_c, got_p = _run(z, 1008, labels, groups, 95, np.float32(1e30))
  exact('pred', got_p, pred)
  exact('counts', got_c, want)


def test_1031_rows_in_one_group_all_atomics_on_three_addresses(hip_lib, big):
  z, labels, per_row, pred = big
  groups = np.full(z.shape[0], 42, np.int32)
  want = np.zeros((96, 3), np.int64)
  want[42] = per_row.sum(axis=0)
  assert want[42, 0] == 1031 and want[42, 1] > 400 and want[42, 2] > 300
  got_c, got_p = _run(z, 1008, labels, groups, 95, np.float32(NAN))
  exact('pred', got_p, pred)
  exact('counts', got_c, want)


def test_bad_arguments_are_refused_before_any_launch(hip_lib):
  from assembled_cnn_amd import lib, ops
  L = hip_lib
  z, labels, groups = _case(4, 5, 3, 9)
  zin, lab, grp = In(_padded(z, 8, 0), torch.float32), In(labels, torch.int32, 0), In(groups, torch.int32, 0)
  counts = Out((4, 3), torch.int32)
  good = dict(logits=zin.p, ld=8, labels=lab.p, groups=grp.p, B=4, C=5, G=3, counts=counts.p, pred=0)
  order = ('logits', 'ld', 'labels', 'groups', 'B', 'C', 'G', 'counts', 'pred')
  launches = L.asm_launch_count()
  for bad in (dict(logits=0), dict(labels=0), dict(groups=0), dict(counts=0), dict(B=0), dict(C=0), dict(G=0), dict(B=-3),
              dict(ld=4)):
    kw = dict(good, **bad)
    rc = L.asm_eval_groups(*[ctypes.c_void_p(kw[k]) if k in ('logits', 'labels', 'groups', 'counts', 'pred') else kw[k]
                             for k in order], ctypes.c_void_p(ops._stream()))
    assert rc == lib.ASM_EINVAL, bad
  assert L.asm_launch_count() == launches
  torch.cuda.synchronize()
  counts.check_flanks()
  assert bool((counts.t.view(torch.uint8) == 0xA5).all()), 'a refused call wrote counters'
  # the ops wrapper refuses tables of the wrong type or size itself
  c = torch.zeros((4, 3), dtype=torch.int32, device=DEV)
  with pytest.raises(ValueError):
    ops.eval_groups(zin.t, 8, lab.t, grp.t, 4, 5, 4, c)
  with pytest.raises(ValueError):
    ops.eval_groups(zin.t, 8, lab.t.long(), grp.t, 4, 5, 3, c)
  pred = ops.eval_groups(zin.t, 8, lab.t, grp.t, 4, 5, 3, c, want_pred=True)
  want_c, want_p = RR.eval_groups(z, labels, groups, 3)
  exact('ops.eval_groups counts', c.cpu().numpy(), want_c)
  exact('ops.eval_groups pred', pred.cpu().numpy(), want_p)
  assert ops.eval_groups(zin.t, 8, lab.t, grp.t, 4, 5, 3, c) is None
