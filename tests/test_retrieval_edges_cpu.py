"""The retrieval edge cases without a GPU: the tables of tests/retrieval_cases.py hold what they claim (exact operands, exact
float32 sums, the ties), every case takes the kernel path it is meant for -- asked of the real library through
asm_debug_retrieval_plan, which launches nothing -- and the shared checkers pass on the reference's own result and fail on
every kind of damaged result in the group meant to catch it."""
import ctypes

import numpy as np
import pytest

from tests import retrieval_cases as RC
from tests import retrieval_ref as ref
from tests.test_retrieval_cpu import _lib

F32, F64 = np.float32, np.float64
CPU_TOPK = RC.ALL_TOPK


def _plan(L, Q, N, K, wide):
  out = (ctypes.c_int32 * 4)()
  assert L.asm_debug_retrieval_plan(Q, N, K, int(wide), ctypes.byref(out)) == 0
  return tuple(out)


def test_plan_query_is_host_only_and_checks_its_arguments():
  lib, L = _lib()
  n0 = L.asm_launch_count()
  out = (ctypes.c_int32 * 4)()
  for Q, N, K in ((0, 5, 6), (5, 0, 6), (5, 5, 0), (-1, 5, 6)):
    assert L.asm_debug_retrieval_plan(Q, N, K, 0, ctypes.byref(out)) == lib.ASM_EINVAL
  assert L.asm_debug_retrieval_plan(5, 5, 6, 0, None) == lib.ASM_EINVAL
  assert L.asm_debug_retrieval_plan(5, 5, 65, 0, ctypes.byref(out)) == lib.ASM_ENOTSUP
  assert L.asm_debug_retrieval_plan(5, 5, 1025, 1, ctypes.byref(out)) == lib.ASM_ENOTSUP
  assert _plan(L, 5, 5, 6, False) == (1, 1, 1, 0)
  S, tps, nt, B = _plan(L, 5, 5, 1024, True)
  assert (S, tps, nt) == (1, 1, 1) and B >= 1024 + RC.TILE and B % 64 == 0
  # the workspace the launchers ask for holds the plan's buffers: [Q][S][K] / [Q][S][B] values and as many indices
  for Q, N, K in ((1, 1, 1), (129, 8193, 6), (257, 300, 64), (8192, 60502, 6)):
    S, tps, nt, B = _plan(L, Q, N, K, False)
    assert L.asm_retrieval_topk_workspace_bytes(Q, N, K) >= Q * S * K * 8
  for Q, N, K in ((1, 1, 1), (129, 98304, 1000), (33, 16384, 6), (8192, 60502, 1001)):
    S, tps, nt, B = _plan(L, Q, N, K, True)
    assert L.asm_retrieval_topk_wide_workspace_bytes(Q, N, K) >= Q * S * B * 8
  assert L.asm_launch_count() == n0


def test_a_refusal_names_the_entry_point_that_was_called():
  """the two entry points share their checks: whichever refuses, the message starts with the name of the one called"""
  lib, L = _lib()
  n0 = L.asm_launch_count()
  p = ctypes.c_void_p(0x1000)                      # never dereferenced: every call below returns before any launch
  for name, cap in (('asm_retrieval_topk', 64), ('asm_retrieval_topk_wide', 1024)):
    fn, ws = getattr(L, name), getattr(L, name + '_workspace_bytes')(100, 1000, 6)
    assert ws > 0

    def refused(q=p, K=6, wb=ws):
      rc = fn(q, 64, p, 64, p, p, 100, 1000, 64, 0, K, 0, p, p, p, wb, None)
      return rc, L.asm_last_error()
    for kw, want in ((dict(q=None), lib.ASM_EINVAL), (dict(wb=ws - 1), lib.ASM_EINVAL), (dict(K=cap + 1), lib.ASM_ENOTSUP)):
      rc, msg = refused(**kw)
      assert rc == want and msg.startswith(name[len('asm_'):].encode() + b':'), (name, kw, rc, msg)
  assert L.asm_launch_count() == n0


def test_every_case_takes_the_path_it_claims():
  _, L = _lib()
  seen = set()
  for c in RC.ALL_TOPK:
    for sel in c.sels:
      plan = _plan(L, c.Q, c.N, c.K, sel == 'wide')
      assert plan[2] == -(-c.N // RC.TILE)
      if sel in c.path:
        assert RC.PATHS[c.path[sel]](*plan), (c.id, sel, c.path[sel], plan)
        seen.add((sel, c.path[sel]))
    if c.kind == 'thermo':
      assert c.path['period'] == _plan(L, c.Q, c.N, c.K, True)[1] * RC.TILE, 'the period is one run'
  assert seen >= {('list', 'single'), ('list', 'one_tile_splits'), ('list', 'two_tile_splits'), ('list', 'ragged'),
                  ('wide', 'one_tile_splits'), ('wide', 'compaction')}
  # the ragged case: the last split is ONE tile and that tile holds ONE row; the 66-tile case ends in a one-row tile too
  ragged = [c for c in RC.TILES if c.path['list'] == 'ragged'][0]
  S, tps, nt, _ = _plan(L, ragged.Q, ragged.N, ragged.K, False)
  assert nt - (S - 1) * tps == 1 and ragged.N - (nt - 1) * RC.TILE == 1
  assert all(c.N % RC.TILE == 1 for c in RC.TILES if c.path['list'] in ('ragged', 'two_tile_splits'))
  # every compaction case: whole runs, each longer than the trigger B - 128
  for c in RC.COMPACTION:
    S, tps, nt, B = _plan(L, c.Q, c.N, c.K, True)
    assert S * tps == nt and tps * RC.TILE > B - RC.TILE


def test_the_tables_hold_the_cases_the_suite_is_meant_to_have():
  assert sorted({c.D for c in RC.DTAIL}) == sorted(RC.DTAIL_D) and {c.pad for c in RC.DTAIL} == {(0, 0), (8, 16)}
  assert all(c.Q == 33 and c.N == 129 and c.K == 6 and c.sels == RC.BOTH for c in RC.DTAIL)
  assert all(c.ldq % 8 == 0 and c.ldi % 8 == 0 and c.ldq >= c.D and c.ldi >= c.D for c in RC.ALL_TOPK)
  shapes = {(c.Q, c.N) for c in RC.TILES}
  assert shapes >= {(1, 1), (1, 128), (1, 129), (128, 128), (129, 257), (257, 300), (129, 8321)}
  bases = [c.base for c in RC.TILES]
  assert sum(b == 0 for b in bases) * 2 == len(bases) and any(c.base + c.N == RC.INT32_MAX for c in RC.TILES)
  assert all(c.base + c.N <= RC.INT32_MAX for c in RC.ALL_TOPK)
  for K in (1, 2, 63, 64):
    assert {c.N for c in RC.KEDGE_LIST if c.K == K} == {n for n in (K - 1, K, K + 1) if n > 0}
  wide = {(c.K, c.N) for c in RC.KEDGES if 'wide' in c.sels}
  assert wide >= {(K, K + 1) for K in (1, 64, 65, 256, 257, 448, 449, 1023, 1024)}
  assert len({K for K, N in wide if K >= 65 and N == K - 1}) == 3
  for sim in RC.SIMS:
    assert {(c.K, c.N, c.Q) for c in RC.COMPACTION if c.sim == sim} == {(K, N, Q) for K, N in ((6, 16384), (1000, 98304))
                                                                          for Q in (1, 33, 129)}
  assert {c.sim for c in RC.NONFINITE} == set(RC.SIMS) and all(c.sels == RC.BOTH for c in RC.NONFINITE)
  assert len({c.id for c in RC.ALL_TOPK}) == len(RC.ALL_TOPK)
  assert {(m.rows, m.P, m.K) for m in RC.MERGE_LIST} == {(r, P, K) for r in (1, 257) for P in (1, 3, 64) for K in (1, 6, 64)}
  assert {m.K for m in RC.MERGE_WIDE} == {1, 2, 3, 255, 256, 257, 1024} and {m.P for m in RC.MERGE_WIDE} == {1, 3, 64}
  assert {(c.Q, c.K, c.nk) for c in RC.RECALL} == {(Q, K, nk) for Q in (1, 63, 64, 65, 257) for K in (1, 6) for nk in (1, 3)}
  assert any(c.base > 0 for c in RC.RECALL) and any(max(c.k_list) > c.K for c in RC.RECALL)


@pytest.mark.parametrize('c', CPU_TOPK, ids=[c.id for c in CPU_TOPK])
def test_inputs_are_exact_and_tie_as_claimed(c):
  q, x = c.inputs()
  assert q.shape == (c.Q, c.D) and x.shape == (c.N, c.D) and q.dtype == F32 and x.dtype == F32
  assert np.array_equal(RC.to_bf16(q), q) and np.array_equal(RC.to_bf16(x), x), 'an operand is not a bf16 value'
  fin = np.isfinite(x).all(1)
  assert c.kind == 'nonfinite' or fin.all()
  a, b = np.abs(q.astype(F64)), np.abs(x[fin].astype(F64))
  assert (a == np.round(a)).all() and (b == np.round(b)).all()                        # integers: every sum below is one
  aa, bb, ab = (a * a).sum(1), (b * b).sum(1), a @ b.T
  assert ab.max() < 2 ** 24 and aa.max() + bb.max() + 2 * ab.max() < 2 ** 24, 'a float32 sum of the epilogue could round'
  if c.sim == 'cosine' and c.kind != 'nonfinite':
    m = max(v for v in (1, 4, 16) if v <= c.D)
    assert (aa == m).all() and (bb == m).all() and set(np.unique(a)) <= {0.0, 1.0}, 'cosine rows: m entries of +-1'
  if c.kind == 'nonfinite':
    sim, inv = RC.similarities(c)
    nan, ninf = np.isnan(sim[inv]), np.isneginf(sim[inv])
    assert nan[:, 2].sum() == (2 if c.sim == 'euclidean' else 3) and nan.sum() == nan[:, 2].sum()
    assert ninf.sum() == (1 if c.sim == 'euclidean' else 0) and not np.isposinf(sim).any()
    return
  sim, inv = RC.similarities(c)
  own, _ = RC.similarities(c, own_formula=True)                 # the formula the damaged forms go through is the oracle's
  assert np.array_equal(own, sim) if c.sim == 'euclidean' else np.abs(own - sim).max() < 1e-15
  srt = -np.sort(-sim, axis=1)
  if 'inside' in c.ties:
    assert (srt[:, 1:c.K] == srt[:, :c.K - 1]).any(), 'no tied neighbours inside the top K'
  if 'boundary' in c.ties:
    assert c.N > c.K and (srt[:, c.K - 1] == srt[:, c.K]).any(), 'no tie across the K / K + 1 boundary'
  if c.kind == 'thermo':
    period = c.path['period']
    first = sim[:, :period]
    assert (np.diff(first[inv[0]]) > 0).all(), 'the ascending query: strictly rising within a run'
    if c.seed and c.Q >= 3:
      assert (np.diff(first[inv[1]]) < 0).all() and np.argmax(first[inv[2]]) == RC.thermo_middle(period)
    assert np.array_equal(sim[:, :period], sim[:, period:2 * period])


@pytest.mark.parametrize('c', CPU_TOPK, ids=[c.id for c in CPU_TOPK])
def test_checker_passes_on_the_reference(c):
  val, idx = RC.reference(c)
  RC.check_topk(c, val.astype(F32), idx, val, idx)
  if c.kind == 'equal':
    assert np.array_equal(idx, np.tile(c.base + np.arange(c.K), (c.Q, 1)))
  if c.kind not in ('nonfinite',) and c.N <= 400:      # the lexsort reference is the oracle's stable argsort
    q, x = c.inputs()
    wv, wi = ref.top_k(ref.similarity(q, x, c.sim), c.K)
    assert np.array_equal(idx[:, :wi.shape[1]], wi + c.base) and (idx[:, wi.shape[1]:] == -1).all()
  if c.kind == 'nonfinite':
    assert (idx == 2 + c.base).sum() == (1 if c.sim == 'euclidean' else 0)
    assert (idx < 0).sum() == (2 if c.sim == 'euclidean' else 3)
    if c.sim == 'euclidean':
      assert idx[1, -1] == 2 + c.base and np.isneginf(val[1, -1])


@pytest.mark.parametrize('damage', RC.DAMAGE)
def test_checker_notices_each_kind_of_damage(damage):
  """a kernel wrong in this way fails at least one case of every group meant to catch it"""
  for group in RC.DAMAGE_GROUPS[damage]:
    caught = []
    for c in RC.TOPK_GROUPS[group]:
      val, idx = RC.reference(c)
      bad_val, bad_idx = RC.reference(c, damage)
      try:
        RC.check_topk(c, bad_val.astype(F32), bad_idx, val, idx)
      except AssertionError:
        caught.append(c.id)
    print('\n%s in %s: caught by %d of %d cases' % (damage, group, len(caught), len(RC.TOPK_GROUPS[group])), end='')
    assert caught, '%s goes unnoticed in %s' % (damage, group)
    if damage == 'padding':
      assert len(caught) == sum(1 for c in RC.DTAIL if c.ldq > c.D)
    if damage == 'short':
      assert len(caught) == sum(1 for c in RC.DTAIL if c.D % 8)


def test_selections_agree_checker():
  c = RC.KEDGE_LIST[5]
  v32, idx = np.array([[3.0, 1.5, -np.inf]], F32), np.array([[4, 2, -1]])
  RC.selections_agree(c, v32, idx, v32, idx)
  with pytest.raises(AssertionError):
    RC.selections_agree(c, v32, idx, np.nextafter(v32, F32(1e9)), idx)
  with pytest.raises(AssertionError):
    RC.selections_agree(c, v32, idx, v32, idx[:, ::-1])
  z = np.zeros((1, 2), F32)
  RC.selections_agree(c, -z, np.zeros((1, 2)), z, np.zeros((1, 2)))
  with pytest.raises(AssertionError):
    RC.selections_agree(c, z, np.zeros((1, 2)), -z, np.zeros((1, 2)))


# ---- merges, recall, norms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', RC.MERGE_LIST + RC.MERGE_WIDE, ids=[m.id for m in RC.MERGE_LIST + RC.MERGE_WIDE])
def test_merge_inputs_and_reference(m):
  val, idx = RC.merge_inputs(m)
  assert val.shape == idx.shape == (m.rows, m.P, m.K)
  valid = idx >= 0
  assert (val[~valid] == RC.UNUSED_VALUE).all()
  for r in range(m.rows):
    ids = idx[r][valid[r]]
    assert ids.size == np.unique(ids).size, 'index rows are distinct within a row'
    flavour = RC.MERGE_FLAVOURS[r % 5]
    if flavour == 'none':
      assert ids.size == 0
    if flavour == 'few':
      assert ids.size < m.K
    if not m.wide:
      for l in range(m.P):
        n = int(valid[r, l].sum())
        assert valid[r, l, :n].all(), '-1 only at the end of a sorted list'
        v, i = val[r, l, :n].astype(F64), idx[r, l, :n]
        assert np.array_equal(np.lexsort((i, -v)), np.arange(n)), 'a list is not sorted'
  if valid.sum() >= 100:
    v0 = val[valid]
    assert np.signbit(v0[v0 == 0]).any() and not np.signbit(v0[v0 == 0]).all(), '-0 against +0'
  if m.wide:
    assert np.isposinf(val[valid]).any() and np.isneginf(val[valid]).any() if m.K >= 255 else True
    assert m.K < 255 or not valid[:, :, 0].all(), '-1 anywhere, not only at the end'
  if m.P > 1 and m.K > 1:
    assert (valid.sum(2)[0] == 0).any(), 'a wholly unused list next to used ones'
  wv, wi = RC.merge_reference(m, val, idx)
  RC.check_merge(m, np.where(wv == 0, 0.0, wv), wi, wv, wi)
  ties = (wv[:, 1:] == wv[:, :-1]) & (wi[:, 1:] >= 0)
  assert (wi[:, 1:][ties] > wi[:, :-1][ties]).all()
  if m.K > 1 and m.P > 1:
    assert ties.any()
    with pytest.raises(AssertionError):                 # the tie rule reversed
      sw = wi.copy()
      r, j = np.argwhere(ties)[0]
      sw[r, j], sw[r, j + 1] = wi[r, j + 1], wi[r, j]
      RC.check_merge(m, wv, sw, wv, wi)
  if (wi < 0).any():
    with pytest.raises(AssertionError):                 # an unused slot holds 0 / 0
      RC.check_merge(m, np.where(wi < 0, 0.0, wv), np.where(wi < 0, 0, wi), wv, wi)


@pytest.mark.parametrize('c', RC.RECALL, ids=[c.id for c in RC.RECALL])
def test_recall_inputs_and_reference(c):
  top, qlab, ilab = RC.recall_inputs(c)
  assert top.shape == (c.Q, c.K) and top.dtype == np.int32
  selfs = (top == (c.base + np.arange(c.Q))[:, None]).sum(1)
  want = np.where(np.arange(c.Q) % 3 == 0, 0, np.where((np.arange(c.Q) % 3 == 2) & (c.K >= 3), 2, 1))
  assert np.array_equal(selfs, want)
  if c.Q * c.K >= 300:
    assert (top == -1).any() and (top >= c.N).any()
  hits = RC.recall_reference(c, top, qlab, ilab)
  assert all(h >= p for h, p in zip(hits, c.preload)) and all(p > 0 for p in c.preload)
  # the same count by hand, written from the header's words
  for j, k in enumerate(c.k_list):
    n = 0
    for r in range(c.Q):
      kept = [int(e) for e in top[r] if e != c.base + r][:k]
      n += any(0 <= e < c.N and ilab[e] == qlab[r] for e in kept)
    assert hits[j] == c.preload[j] + n


@pytest.mark.parametrize('damage', ['flank', 'extrarow'])
def test_recall_reads_outside_the_arrays_are_noticed(damage):
  """a kernel that looks up an entry outside [0, N) reads the flank of the index labels, one that scores row Q reads the
  flanks of top_idx and of the query labels: with the flanks of recall_flanks either changes the hits, at every Q"""
  for Q in (1, 63, 64, 65, 257):
    caught = []
    for c in RC.RECALL:
      if c.Q == Q:
        top, qlab, ilab = RC.recall_inputs(c)
        flanks = RC.recall_flanks(top, qlab, ilab)
        assert flanks['ilab'] in qlab and flanks['qlab'] == ilab[flanks['top']] and flanks['top'] != c.base + c.Q
        if RC.recall_reference(c, top, qlab, ilab, damage=damage) != RC.recall_reference(c, top, qlab, ilab):
          caught.append(c.id)
    print('\n%s at Q = %d: caught by %d of 4 cases' % (damage, Q, len(caught)), end='')
    assert caught, '%s goes unnoticed at Q = %d' % (damage, Q)
    if damage == 'extrarow':
      assert len(caught) == 4


def test_recall_self_damage_is_noticed():
  caught = [c.id for c in RC.RECALL
            if RC.recall_reference(c, *RC.recall_inputs(c), damage='self') != RC.recall_reference(c, *RC.recall_inputs(c))]
  print('\nself entry counted as a position: caught by %d of %d cases' % (len(caught), len(RC.RECALL)), end='')
  assert caught and all('K6' in i for i in caught)
  for Q in (63, 64, 65, 257):
    assert any(i.startswith('Q%d-' % Q) for i in caught)
