"""Recall@K for K up to 1023 without a GPU: the argument checks and the workspace query of the wide entry points on the real
library (every refusal comes before the first device call), and RecallEvaluator's choice between the list and the wide
selection over a numpy double."""
import ctypes

import numpy as np
import pytest
import torch

from tests import retrieval_ref as ref
from tests.cpu_double import T
from tests.test_retrieval_cpu import RetrievalDouble, _lib, _set


def test_wide_argument_checks_need_no_gpu():
  lib, L = _lib()
  p = ctypes.c_void_p(0x1000)                      # never dereferenced: the calls below return before any launch
  ws = L.asm_retrieval_topk_wide_workspace_bytes(100, 1000, 101)

  def topk(q=p, ldq=64, x=p, ldi=64, sqq=p, sqx=p, Q=100, N=1000, D=64, sim=0, K=101, base=0, tv=p, ti=p, w=p, wb=ws):
    return L.asm_retrieval_topk_wide(q, ldq, x, ldi, sqq, sqx, Q, N, D, sim, K, base, tv, ti, w, wb, None)
  for kw in (dict(q=None), dict(x=None), dict(sqq=None), dict(sqx=None), dict(tv=None), dict(ti=None), dict(w=None),
             dict(Q=0), dict(N=0), dict(D=0), dict(K=0), dict(Q=-3), dict(ldq=60), dict(ldi=60), dict(ldq=56), dict(ldi=56),
             dict(D=60, ldq=64, ldi=63), dict(base=-1), dict(base=2**31 - 500), dict(wb=ws - 1), dict(wb=0)):
    assert topk(**kw) == lib.ASM_EINVAL, kw
  assert b'workspace' in L.asm_last_error()
  assert topk(sim=2) == lib.ASM_ENOTSUP and topk(sim=-1) == lib.ASM_ENOTSUP
  # K = 1024 passes every check up to the workspace check; K = 1025 is refused by the cap, whatever the workspace
  assert topk(K=1024, wb=L.asm_retrieval_topk_wide_workspace_bytes(100, 1000, 1024) - 1) == lib.ASM_EINVAL
  assert b'workspace' in L.asm_last_error()
  assert topk(K=1025, wb=1 << 40) == lib.ASM_ENOTSUP and b'cap of 1024' in L.asm_last_error()
  assert topk(K=4096, wb=1 << 40) == lib.ASM_ENOTSUP

  q = ctypes.c_void_p(0x2000)
  m = L.asm_topk_merge_wide
  assert m(None, p, 4, 3, 101, q, q, None) == lib.ASM_EINVAL
  assert m(p, None, 4, 3, 101, q, q, None) == lib.ASM_EINVAL
  assert m(p, p, 4, 3, 101, None, q, None) == lib.ASM_EINVAL
  assert m(p, p, 4, 3, 101, q, None, None) == lib.ASM_EINVAL
  assert m(p, p, 0, 3, 101, q, q, None) == lib.ASM_EINVAL
  assert m(p, p, 4, 0, 101, q, q, None) == lib.ASM_EINVAL
  assert m(p, p, 4, 3, 0, q, q, None) == lib.ASM_EINVAL
  assert m(p, p, 4, 3, 101, p, q, None) == lib.ASM_EINVAL      # in place
  assert m(p, p, 4, 3, 101, q, p, None) == lib.ASM_EINVAL
  assert m(p, p, 4, 3, 1025, q, q, None) == lib.ASM_ENOTSUP and b'cap of 1024' in L.asm_last_error()


def test_wide_workspace_query_is_positive_monotone_and_small():
  _, L = _lib()
  f = L.asm_retrieval_topk_wide_workspace_bytes
  assert f(0, 10, 6) == 0 and f(10, 0, 6) == 0 and f(10, 10, 0) == 0 and f(-1, 10, 6) == 0
  sizes = [1, 2, 100, 127, 128, 129, 255, 256, 257, 1000, 4096, 8192, 8193, 60502, 65536, 100000]
  ks = (1, 6, 33, 64, 65, 101, 1001, 1024)
  for K in ks:
    for other in sizes:
      prev_q = prev_n = 0
      for v in sizes:
        bq, bn = f(v, other, K), f(other, v, K)
        assert bq > 0 and bn > 0
        assert bq >= prev_q and bn >= prev_n, (v, other, K)
        prev_q, prev_n = bq, bn
  for Q in sizes:
    for N in sizes:
      b = [f(Q, N, K) for K in ks]
      assert all(x <= y for x, y in zip(b, b[1:])), (Q, N)
      assert b[0] < b[-1]
  # candidates, not similarities: a default query chunk against Stanford Online Products at R@1000
  assert f(8192, 60502, 1001) < 8192 * 60502 * 4 // 4


# ---- RecallEvaluator's choice of a selection, over a numpy double -------------------------------------------------
class WideDouble(RetrievalDouble):
  """RetrievalDouble + the three wide entry points; list and wide calls are recorded apart"""
  wide_calls = None

  def asm_retrieval_topk_wide_workspace_bytes(self, Q, N, K):
    return 16

  def asm_retrieval_topk_wide(self, q, ldq, x, ldi, sqq, sqx, Q, N, D, sim, K, base, tv, ti, ws, wsb, stream):
    keep, self.calls = self.calls, None                 # not a list call
    try:
      self.wide_calls.append((Q, N, K, base))
      return self.asm_retrieval_topk(q, ldq, x, ldi, sqq, sqx, Q, N, D, sim, K, base, tv, ti, ws, wsb, stream)
    finally:
      self.calls = keep

  def asm_topk_merge_wide(self, iv, ii, rows, P, K, ov, oi, stream):
    self.asm_topk_merge(iv, ii, rows, P, K, ov, oi, stream)
    T(ov, (rows, K), 'f32')[T(oi, (rows, K), 'i32') < 0] = float('-inf')
    return 0


@pytest.fixture
def wide_double():
  from assembled_cnn_amd import ops
  d = WideDouble()
  d.calls, d.wide_calls = [], []
  ops.set_library(d, is_double=True)
  yield d
  ops.set_library(None, is_double=False)


def _fill(ev, feat, lab, step=256):
  for s in range(0, feat.shape[0], step):
    ev.add(feat[s:s + step], lab[s:s + step])
  return ev


def test_caps_are_public():
  from assembled_cnn_amd import ops
  assert ops.TOPK_LIST_MAX == 64 and ops.TOPK_WIDE_MAX == 1024


def test_small_k_list_stays_on_the_list_selection(wide_double):
  from assembled_cnn_amd.retrieval import RecallEvaluator
  feat, lab = _set()
  want = ref.recall_at_k(feat.float().numpy(), lab.numpy(), (1, 5), 'cosine')
  got = _fill(RecallEvaluator((1, 5)), feat, lab).result()
  assert got == want
  assert wide_double.wide_calls == [] and wide_double.calls == [(630, 700, 6, 0)]
  wide_double.calls.clear()
  assert _fill(RecallEvaluator((1, 63)), feat, lab).result()['count'] == 630       # K = 64: the last list size
  assert wide_double.wide_calls == [] and wide_double.calls == [(630, 700, 64, 0)]


@pytest.mark.parametrize('similarity', ['cosine', 'euclidean'])
@pytest.mark.parametrize('k_list', [(1, 10, 100), (1, 10, 100, 1000), (64,)])
def test_large_k_list_goes_to_the_wide_selection(wide_double, similarity, k_list):
  from assembled_cnn_amd.retrieval import RecallEvaluator
  feat, lab = _set(n=1500, ncls=200)
  want = ref.recall_at_k(feat.float().numpy(), lab.numpy(), k_list, similarity)
  Q = int((lab != -1).sum())
  for chunk in (8192, 1000, 7):
    wide_double.wide_calls.clear()
    got = _fill(RecallEvaluator(k_list, similarity, query_chunk=chunk), feat, lab).result()
    assert got == want
    assert wide_double.calls == []
    assert [c[0] for c in wide_double.wide_calls] == [min(chunk, Q - s) for s in range(0, Q, chunk)]
    assert all(c[1:] == (1500, max(k_list) + 1, 0) for c in wide_double.wide_calls)
  assert 0.0 < want['recall_at_%d' % k_list[0]] and want['recall_at_%d' % k_list[0]] <= want['recall_at_%d' % k_list[-1]]


def test_selection_argument(wide_double):
  from assembled_cnn_amd.retrieval import RecallEvaluator
  feat, lab = _set()
  a = _fill(RecallEvaluator((1, 5), selection='list'), feat, lab).result()
  assert wide_double.wide_calls == [] and len(wide_double.calls) == 1
  wide_double.calls.clear()
  b = _fill(RecallEvaluator((1, 5), selection='wide'), feat, lab).result()
  assert wide_double.calls == [] and wide_double.wide_calls == [(630, 700, 6, 0)]
  assert a == b == ref.recall_at_k(feat.float().numpy(), lab.numpy(), (1, 5), 'cosine')
  with pytest.raises(NotImplementedError, match='64'):
    RecallEvaluator((100,), selection='list')
  with pytest.raises(ValueError):
    RecallEvaluator((1, 5), selection='heap')
  RecallEvaluator((1023,), selection='wide')
  RecallEvaluator((1023,))


def test_k_list_above_the_cap_fails_in_the_constructor(wide_double):
  from assembled_cnn_amd.retrieval import RecallEvaluator
  for kw in (dict(), dict(selection='wide'), dict(selection='auto')):
    with pytest.raises(NotImplementedError, match='1024'):
      RecallEvaluator((1024,), **kw)
  with pytest.raises(NotImplementedError, match='1024'):
    RecallEvaluator((1, 10, 5000))


def test_wide_ops_refuse_what_the_list_ops_refuse(wide_double):
  from assembled_cnn_amd import ops
  feat, _ = _set(n=64)
  sq = ops.embed_sqnorm(feat)
  with pytest.raises(NotImplementedError):
    ops.retrieval_topk_wide(feat, feat, sq, sq, 101, similarity='manhattan')
  with pytest.raises(ValueError):
    ops.retrieval_topk_wide(feat, feat[:, :8].contiguous(), sq, sq, 101)
  with pytest.raises(ValueError):
    ops.topk_merge_wide(torch.zeros(4, 3, 101), torch.zeros(4, 3, 100, dtype=torch.int32))
  assert ops.retrieval_topk_wide_workspace_bytes(10, 10, 101) == 16


def test_topk_merge_wide_takes_lists_in_any_order(wide_double):
  from assembled_cnn_amd import ops
  vals = torch.tensor([[[1.0, 5.0, 0.0], [5.0, 7.0, 2.0]]])          # one row, two lists of three, unsorted, one slot unused
  idxs = torch.tensor([[[4, 9, -1], [3, 0, 8]]], dtype=torch.int32)
  mv, mi = ops.topk_merge_wide(vals, idxs)
  assert mi.tolist() == [[0, 3, 9]] and mv.tolist() == [[7.0, 5.0, 5.0]]
