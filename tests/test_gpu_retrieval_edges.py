"""Edge shapes, pitches, splits, compaction and guard bands of the retrieval kernels (csrc/retrieval.hip) against the float64
references of tests/retrieval_cases.py, which tests/test_retrieval_edges_cpu.py proves on the CPU: the tables hold what they
claim, every case takes the kernel path it names (asm_debug_retrieval_plan), and the checkers used here fail on every kind of
damaged result.  Every case calls the C ABI directly.

Rules of every case:
* inputs are ``In`` (4 KiB of NaN on either side; an int32 input gets a value that would change the result if it were read),
  and where ld > D the channels D .. ld-1 of every row hold NaN; outputs are ``Out`` (4 KiB of 0xA5 on either side, which must
  survive; the output starts as 0xA5 and no element may still hold it); the workspace is a ``Work`` of exactly
  asm_*_workspace_bytes between the same flanks.  asm_launch_count must move by the launches the plan implies.
* a NaN similarity is never selected, so NaN flanks cannot show an index row read past N: every top-K case of the sweeps runs a
  second time with the index between rows of 1.0 and its norms between -1e30, which would win (run_topk).
* inputs are exact (integers for the euclidean similarity, rows of m entries of +-1 for the cosine), so indices and euclidean
  values are compared with ``array_equal`` and cosine values with the bound of the existing exact tests, 2 * 64 * 2^-24;
  ``-s`` prints the worst cosine error of every case next to it.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import gpu_guard as G
from tests import retrieval_cases as RC
from tests.gpu_guard import BF, In, Out, Work, _release_inputs, call, close_sum, exact  # noqa: F401

pytestmark = pytest.mark.gpu
TF32, TI32 = torch.float32, torch.int32
F32, F64 = np.float32, np.float64


def _ops():
  from assembled_cnn_amd import ops
  return ops


def _plan(c, sel):
  out = (ctypes.c_int32 * 4)()
  assert _ops().L().asm_debug_retrieval_plan(c.Q, c.N, c.K, int(sel == 'wide'), ctypes.byref(out)) == 0
  return tuple(out)


def _ids(cases):
  return [c.id for c in cases]


def run_topk(c, sel, counted=False, phantom=False):
  """one call between guard bands -> (values float64 [Q, K], indices int64 [Q, K], the three counters or None).  The flanks
  of the inputs are NaN: a read outside an operand spoils a similarity, and the row it belongs to goes missing.  A NaN can
  not show an index row read past N, though -- a NaN similarity is never selected -- so ``phantom`` surrounds the index
  with rows of 1.0 and its norms with -1e30: such a row would lead every euclidean list (-(|q|^2 - 1e30 - 2 q.x)) and,
  scaled by rsqrt(1e-12), the cosine list of every query whose entries sum to more than zero"""
  ops = _ops()
  L = ops.L()
  q, x = c.inputs()
  qd, xd = In(RC.padded(q, c.ldq)), In(RC.padded(x, c.ldi), BF, 1.0 if phantom else float('nan'))
  sqq, sqx = In(RC.sqnorm(q), TF32), In(RC.sqnorm(x), TF32, -1e30 if phantom else float('nan'))
  wide = sel == 'wide'
  nbytes = (L.asm_retrieval_topk_wide_workspace_bytes if wide else L.asm_retrieval_topk_workspace_bytes)(c.Q, c.N, c.K)
  ws, val, idx = Work(nbytes), Out((c.Q, c.K), TF32), Out((c.Q, c.K), TI32)
  args = (qd.p, c.ldq, xd.p, c.ldi, sqq.p, sqx.p, c.Q, c.N, c.D, RC.SIM_CODE[c.sim], c.K, c.base, val.p, idx.p, ws.p, nbytes)
  counters = torch.zeros(3, dtype=torch.int64, device=G.DEV) if counted else None
  n0 = L.asm_launch_count()
  if counted:
    ops.check(L.asm_debug_retrieval_topk_wide_counted(*(args + (ops._stream(), G.ptr(counters)))), 'retrieval_topk_wide_counted')
  else:
    call('asm_retrieval_topk_wide' if wide else 'asm_retrieval_topk', *args)
  torch.cuda.synchronize()
  assert L.asm_launch_count() - n0 == (1 if not wide and _plan(c, sel)[0] == 1 else 2), 'launches of %s %s' % (c.id, sel)
  ws.check_flanks()
  return val.np_inf(), idx.np_inf(), counters.cpu().tolist() if counted else None


def check_case(c):
  """every selection of the case against the reference, between NaN flanks and again between flanks that would win (see
  run_topk); the two selections against each other where both are legal"""
  want_val, want_idx = RC.reference(c)
  got = {}
  for sel in c.sels:
    val, idx, _ = run_topk(c, sel)
    RC.check_topk(c, val, idx, want_val, want_idx, sel)
    got[sel] = (val, idx)
    val, idx, _ = run_topk(c, sel, phantom=True)
    RC.check_topk(c, val, idx, want_val, want_idx, sel + ' (winning flanks)')
  if len(got) == 2:
    RC.selections_agree(c, got['list'][0], got['list'][1], got['wide'][0], got['wide'][1])
  return got


@pytest.mark.parametrize('c', RC.DTAIL, ids=_ids(RC.DTAIL))
def test_reduction_tail_and_pitch(hip_lib, c):
  """D from 1 to 129 around the 8-channel piece, the 16-channel MFMA step and the 64-channel k-step, each at ld = round_up(D, 8)
  and at ldq = that + 8, ldi = that + 16 with NaN in the padding; Q = 33 leaves a wave with one query, N = 129 a tile with one
  row; both selections"""
  check_case(c)


@pytest.mark.parametrize('c', RC.TILES, ids=_ids(RC.TILES))
def test_tile_and_split_edges_of_the_list_path(hip_lib, c):
  """one split written straight to the result, one tile per split, two tiles per split, a shorter last split that holds one
  row; index_base up to index_base + N = 2^31 - 1"""
  check_case(c)


@pytest.mark.parametrize('c', RC.KEDGES, ids=_ids(RC.KEDGES))
def test_k_edges(hip_lib, c):
  """K = 1, the list cap and the K at which the capacity of a candidate buffer changes form, with N = K - 1, K, K + 1: unused
  slots hold exactly -inf / -1, and a tie crosses the K / K + 1 boundary"""
  check_case(c)


@pytest.mark.parametrize('c', RC.NONFINITE, ids=_ids(RC.NONFINITE))
def test_non_finite_similarities(hip_lib, c):
  """the header's contract: a NaN similarity makes the row absent for that query (an unused slot appears), a -inf similarity
  ranks last, before the unused slots; both selections"""
  got = check_case(c)
  idx = got['wide'][1]
  assert (idx < 0).sum() == (2 if c.sim == 'euclidean' else 3)


@pytest.mark.parametrize('c', RC.COMPACTION, ids=_ids(RC.COMPACTION))
def test_compaction_of_the_wide_path(hip_lib, c):
  """Runs longer than the trigger of a candidate buffer, in adversarial orders: ascending (every row survives the threshold),
  descending, peaked, and an all-equal index (the radix select runs down into the index digits).  Exact indices and values;
  the counters prove the compactions happened: during the walk at least once per (query, run) at both K, at the end of a run
  at least once per (ascending query, run) at K = 1000 -- lower bounds from the plan, so a retuned capacity keeps them.  The
  uncounted entry point gives the same bits."""
  want_val, want_idx = RC.reference(c)
  S, tps, nt, B = _plan(c, 'wide')
  assert tps * RC.TILE > B - RC.TILE
  val, idx, counters = run_topk(c, 'wide', counted=True)
  RC.check_topk(c, val, idx, want_val, want_idx, 'counted')
  appended, walk, end = counters
  print('\nretrieval-edges %-64s S %d, %d tiles per run, B %d: appended %d, compactions walk %d end %d'
        % (c.id, S, tps, B, appended, walk, end), end='')
  assert walk >= c.Q * S, 'compactions during the walk: %d, at least %d expected' % (walk, c.Q * S)
  if c.K == 1000:
    need = RC.ascending_queries(c) * S
    assert end >= need, 'compactions at the end of a run: %d, at least %d expected' % (end, need)
  assert appended >= c.Q * S * min(c.K, tps * RC.TILE)
  val2, idx2, _ = run_topk(c, 'wide')
  assert np.array_equal(idx2, idx) and np.array_equal(val2.astype(F32).view(np.uint32), val.astype(F32).view(np.uint32))


# ---- the two merges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', RC.MERGE_LIST + RC.MERGE_WIDE, ids=_ids(RC.MERGE_LIST + RC.MERGE_WIDE))
def test_merges(hip_lib, m):
  """block tail (257 rows), K = 1, P = 1, wholly unused lists and rows, ties across lists, -0 against +0, +-inf; the wide merge
  with lists in any order, -1 anywhere, and K around the powers of two its sort pads to"""
  L = _ops().L()
  val, idx = RC.merge_inputs(m)
  want_val, want_idx = RC.merge_reference(m, val, idx)
  iv, ii = In(val, TF32, float('inf')), In(idx, TI32, 0x7ffffff0)       # a flank entry would lead the result
  ov, oi = Out((m.rows, m.K), TF32), Out((m.rows, m.K), TI32)
  n0 = L.asm_launch_count()
  call('asm_topk_merge_wide' if m.wide else 'asm_topk_merge', iv.p, ii.p, m.rows, m.P, m.K, ov.p, oi.p)
  torch.cuda.synchronize()
  assert L.asm_launch_count() - n0 == 1
  RC.check_merge(m, ov.np_inf(), oi.np_inf(), want_val, want_idx)


# ---- the hit counter --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', RC.RECALL, ids=_ids(RC.RECALL))
def test_recall_accumulate(hip_lib, c):
  """block tails (Q around 64 and 256), K = 1, a k above K, entries -1 and >= N (all within the flanks of the labels, which
  hold a label that would match), the query's own number zero, one and two times in its row, query_base > 0, and hits that start non-zero: ``hits +=``, exact"""
  L = _ops().L()
  top, qlab, ilab = RC.recall_inputs(c)
  want = RC.recall_reference(c, top, qlab, ilab)
  hits = Out((c.nk,), TI32, init=torch.tensor(c.preload, dtype=TI32))
  # flanks that change the hits if they are read (RC.recall_flanks; tests/test_retrieval_edges_cpu.py shows that they do): an
  # entry outside [0, N) that is looked up finds a label queries carry, row Q would score at every k; a k that counts everyone
  flanks = RC.recall_flanks(top, qlab, ilab)
  args = (In(top, TI32, flanks['top']).p, c.Q, c.K, In(qlab, TI32, flanks['qlab']).p, In(ilab, TI32, flanks['ilab']).p, c.N,
          c.base, In(np.asarray(c.k_list, np.int32), TI32, RC.INT32_MAX).p, c.nk, hits.p)
  n0 = L.asm_launch_count()
  call('asm_recall_accumulate', *args)
  torch.cuda.synchronize()
  assert L.asm_launch_count() - n0 == 1
  exact('recall ' + c.id, hits.np_inf(), np.asarray(want))


# ---- the norm kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pad', RC.SQNORM_PAD)
@pytest.mark.parametrize('D', RC.SQNORM_D)
def test_embed_sqnorm(hip_lib, D, pad):
  """N around the four rows of a block, D around the 8-channel piece and the 512 channels of one trip of a wave, ld with NaN
  padding: integer inputs exactly, one random input per D within D half-ulps of the sum"""
  L = _ops().L()
  ld = RC.round_up(D, 8) + pad
  for N in RC.SQNORM_N:
    rng = np.random.RandomState(100 * D + N)
    for kind in ('integer',) + (('random',) if N == 5 else ()):
      x = rng.randint(-2, 3, size=(N, D)).astype(F32) if kind == 'integer' else RC.to_bf16(rng.randn(N, D).astype(F32))
      sq = Out((N,), TF32)
      n0 = L.asm_launch_count()
      call('asm_embed_sqnorm', In(RC.padded(x, ld)).p, N, D, ld, sq.p)
      torch.cuda.synchronize()
      assert L.asm_launch_count() - n0 == 1
      sq.assert_written()
      ref = (x.astype(F64) ** 2).sum(1)
      case = 'sqnorm %s N=%d D=%d ld=%d' % (kind, N, D, ld)
      if kind == 'integer':
        exact(case, sq.np(), ref)
      else:
        close_sum(case, sq.np(), ref, D, ref)
