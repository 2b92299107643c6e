"""Recall@K without a GPU: the fp64 oracle against the reference's own get_recall (tests/golden/reference_recall.json), the
argument checks of the real library (they come before any device call), and the host logic of RecallEvaluator over a numpy
double of the five retrieval entry points."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import retrieval_ref as ref
from tests.cpu_double import CpuDouble, T

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, 'golden', 'reference_recall.json')))


@pytest.mark.parametrize('case', FIXTURE['cases'], ids=[c['name'] for c in FIXTURE['cases']])
def test_oracle_reproduces_the_reference_get_recall(case):
  labels = np.asarray(case['labels'])
  qlab = labels[labels != -1]
  assert qlab.tolist() == case['query_labels']
  got = ref.get_recall(np.asarray(case['sorted_idx']), qlab, labels, case['k_list'])
  assert {str(k): v for k, v in got.items()} == case['recall']


def test_fixture_holds_the_quirk_case():
  """with a distractor in front of it a query keeps its self-match: every query of that case hits at k = 1"""
  case = [c for c in FIXTURE['cases'] if c['name'] == 'distractors_interleaved'][0]
  assert case['labels'][0] == -1 and case['recall']['1'] == 1.0


def test_oracle_top_k_prefers_the_lower_index():
  sim = np.array([[1.0, 3.0, 3.0, 2.0, 3.0]])
  val, idx = ref.top_k(sim, 4)
  assert idx.tolist() == [[1, 2, 4, 3]] and val.tolist() == [[3.0, 3.0, 3.0, 2.0]]


# ---- the real library, no GPU: every refusal comes before the first device call ----------------------------------
def _lib():
  import __graft_entry__
  __graft_entry__.build()
  from assembled_cnn_amd import lib
  return lib, lib.load()


def test_retrieval_argument_checks_need_no_gpu():
  lib, L = _lib()
  p = ctypes.c_void_p(0x1000)                      # never dereferenced: the calls below return before any launch
  ws = L.asm_retrieval_topk_workspace_bytes(100, 1000, 6)

  def topk(q=p, ldq=64, x=p, ldi=64, sqq=p, sqx=p, Q=100, N=1000, D=64, sim=0, K=6, base=0, tv=p, ti=p, w=p, wb=ws):
    return L.asm_retrieval_topk(q, ldq, x, ldi, sqq, sqx, Q, N, D, sim, K, base, tv, ti, w, wb, None)
  for kw in (dict(q=None), dict(x=None), dict(sqq=None), dict(sqx=None), dict(tv=None), dict(ti=None), dict(w=None),
             dict(Q=0), dict(N=0), dict(D=0), dict(K=0), dict(Q=-3), dict(ldq=60), dict(ldi=60), dict(ldq=56), dict(ldi=56),
             dict(D=60, ldq=64, ldi=63), dict(base=-1), dict(base=2**31 - 500), dict(wb=ws - 1), dict(wb=0)):
    assert topk(**kw) == lib.ASM_EINVAL, kw
  assert b'workspace' in L.asm_last_error()
  assert topk(sim=2) == lib.ASM_ENOTSUP and topk(sim=-1) == lib.ASM_ENOTSUP
  assert topk(K=65) == lib.ASM_ENOTSUP and b'cap of 64' in L.asm_last_error()
  assert topk(K=4096, wb=1 << 40) == lib.ASM_ENOTSUP

  assert L.asm_embed_sqnorm(None, 4, 64, 64, p, None) == lib.ASM_EINVAL
  assert L.asm_embed_sqnorm(p, 4, 64, 64, None, None) == lib.ASM_EINVAL
  assert L.asm_embed_sqnorm(p, 0, 64, 64, p, None) == lib.ASM_EINVAL
  assert L.asm_embed_sqnorm(p, 4, 0, 64, p, None) == lib.ASM_EINVAL
  assert L.asm_embed_sqnorm(p, 4, 64, 56, p, None) == lib.ASM_EINVAL
  assert L.asm_embed_sqnorm(p, 4, 60, 60, p, None) == lib.ASM_EINVAL

  q = ctypes.c_void_p(0x2000)
  assert L.asm_topk_merge(None, p, 4, 3, 6, q, q, None) == lib.ASM_EINVAL
  assert L.asm_topk_merge(p, p, 0, 3, 6, q, q, None) == lib.ASM_EINVAL
  assert L.asm_topk_merge(p, p, 4, 0, 6, q, q, None) == lib.ASM_EINVAL
  assert L.asm_topk_merge(p, p, 4, 3, 0, q, q, None) == lib.ASM_EINVAL
  assert L.asm_topk_merge(p, p, 4, 3, 6, p, q, None) == lib.ASM_EINVAL      # in place
  assert L.asm_topk_merge(p, p, 4, 3, 65, q, q, None) == lib.ASM_ENOTSUP

  def rec(ti=p, Q=4, K=6, ql=p, il=p, N=10, base=0, kl=p, nk=2, hits=p):
    return L.asm_recall_accumulate(ti, Q, K, ql, il, N, base, kl, nk, hits, None)
  for kw in (dict(ti=None), dict(ql=None), dict(il=None), dict(kl=None), dict(hits=None), dict(Q=0), dict(K=0), dict(N=0),
             dict(nk=0), dict(base=-1)):
    assert rec(**kw) == lib.ASM_EINVAL, kw


def test_workspace_query_is_positive_and_monotone():
  _, L = _lib()
  f = L.asm_retrieval_topk_workspace_bytes
  assert f(0, 10, 6) == 0 and f(10, 0, 6) == 0 and f(10, 10, 0) == 0
  sizes = [1, 2, 100, 127, 128, 129, 255, 256, 257, 1000, 4096, 8192, 8193, 60502, 65536, 100000]
  for K in (1, 6, 33, 64):
    for other in sizes:
      prev_q = prev_n = 0
      for v in sizes:
        bq, bn = f(v, other, K), f(other, v, K)
        assert bq > 0 and bn > 0
        assert bq >= prev_q and bn >= prev_n, (v, other, K)
        prev_q, prev_n = bq, bn
  for Q in sizes:
    for N in sizes:
      assert f(Q, N, 1) < f(Q, N, 6) < f(Q, N, 33) <= f(Q, N, 64)
  assert f(8192, 60502, 6) < 64 << 20            # a default query chunk against Stanford Online Products: a few MB


# ---- host logic of RecallEvaluator over a numpy double -----------------------------------------------------------
class RetrievalDouble(CpuDouble):
  """the five retrieval entry points in numpy (fp64 similarity of the bf16 values, stable argsort), one list per call"""
  calls = None

  def asm_embed_sqnorm(self, x, N, D, ld, sq, stream):
    v = T(x, (N, ld), 'bf16').float()[:, :D].double()
    T(sq, (N,), 'f32').copy_((v * v).sum(1).float())
    return 0

  def asm_retrieval_topk_workspace_bytes(self, Q, N, K):
    return 16

  def asm_retrieval_topk(self, q, ldq, x, ldi, sqq, sqx, Q, N, D, sim, K, base, tv, ti, ws, wsb, stream):
    if self.calls is not None:
      self.calls.append((Q, N, K, base))
    qv = T(q, (Q, ldq), 'bf16').float()[:, :D].double().numpy()
    xv = T(x, (N, ldi), 'bf16').float()[:, :D].double().numpy()
    val, idx = ref.top_k(ref.similarity(qv, xv, ref.SIMILARITIES[sim]), K)
    ov, oi = T(tv, (Q, K), 'f32'), T(ti, (Q, K), 'i32')
    ov.fill_(float('-inf'))
    oi.fill_(-1)
    ov[:, :val.shape[1]] = torch.from_numpy(val).float()
    oi[:, :idx.shape[1]] = torch.from_numpy(idx + base).to(torch.int32)
    return 0

  def asm_topk_merge(self, iv, ii, rows, P, K, ov, oi, stream):
    v = T(iv, (rows, P * K), 'f32').numpy().astype(np.float64)
    i = T(ii, (rows, P * K), 'i32').numpy().astype(np.int64)
    v = np.where(i < 0, -np.inf, v)
    key = np.where(i < 0, np.iinfo(np.int64).max, i)
    order = np.stack([np.lexsort((key[r], -v[r]))[:K] for r in range(rows)])
    T(ov, (rows, K), 'f32').copy_(torch.from_numpy(np.take_along_axis(v, order, 1)).float())
    T(oi, (rows, K), 'i32').copy_(torch.from_numpy(np.take_along_axis(i, order, 1)).to(torch.int32))
    return 0

  def asm_recall_accumulate(self, ti, Q, K, ql, il, N, base, kl, nk, hits, stream):
    ks = T(kl, (nk,), 'i32').tolist()
    h = ref.get_hits(T(ti, (Q, K), 'i32').numpy(), T(ql, (Q,), 'i32').numpy(), T(il, (N,), 'i32').numpy(), ks, query_base=base)
    out = T(hits, (nk,), 'i32')
    for j, k in enumerate(ks):
      out[j] += h[k]
    return 0


@pytest.fixture
def retrieval_double():
  from assembled_cnn_amd import ops
  d = RetrievalDouble()
  d.calls = []
  ops.set_library(d, is_double=True)
  yield d
  ops.set_library(None, is_double=False)


def _set(n=700, D=16, ncls=20, seed=0, interleave=False):
  rng = np.random.RandomState(seed)
  lab = rng.randint(0, ncls, size=n)
  feat = torch.from_numpy((rng.randn(ncls, D)[lab] + 1.5 * rng.randn(n, D)).astype(np.float32)).to(torch.bfloat16)
  if interleave:
    lab[rng.rand(n) < 0.1] = -1
    lab[0] = -1
  else:
    lab[n - n // 10:] = -1
  return feat, torch.from_numpy(lab)


@pytest.mark.parametrize('similarity', ['cosine', 'euclidean'])
@pytest.mark.parametrize('interleave', [False, True])
def test_evaluator_matches_the_oracle_and_chunking_changes_nothing(retrieval_double, similarity, interleave):
  from assembled_cnn_amd.retrieval import RecallEvaluator
  feat, lab = _set(interleave=interleave)
  want = ref.recall_at_k(feat.float().numpy(), lab.numpy(), (1, 5), similarity)
  results = []
  for chunk in (8192, 100, 7):
    ev = RecallEvaluator((1, 5), similarity, query_chunk=chunk)
    retrieval_double.calls.clear()
    for s in range(0, 700, 64):
      ev.add(feat[s:s + 64], lab[s:s + 64])
    results.append(ev.result())
    Q = int((lab != -1).sum())
    assert [c[0] for c in retrieval_double.calls] == [min(chunk, Q - s) for s in range(0, Q, chunk)]
    assert all(c[1:] == (700, 6, 0) for c in retrieval_double.calls)
  assert sorted(results[0]) == ['count', 'recall_at_1', 'recall_at_5']
  assert results[0] == want and results[1] == want and results[2] == want
  if interleave:      # row 0 is a distractor, so every query keeps its self-match (the reference's quirk): a hit at k = 1
    assert want['recall_at_1'] == 1.0
  else:
    assert 0.05 < want['recall_at_1'] < want['recall_at_5'] < 1.0


def test_evaluator_buffers_grow_geometrically_and_reset(retrieval_double):
  from assembled_cnn_amd.retrieval import RecallEvaluator
  feat, lab = _set(n=5000)
  ev = RecallEvaluator((1, 2, 4))
  caps = set()
  for s in range(0, 5000, 50):
    ev.add(feat[s:s + 50], lab[s:s + 50])
    caps.add(ev._emb.shape[0])
  assert ev.count == 5000 and sorted(caps) == [1024, 2048, 4096, 8192]
  assert torch.equal(ev._emb[:5000], feat) and torch.equal(ev._lab[:5000], lab.to(torch.int32))
  r = ev.result()
  assert sorted(r) == ['count', 'recall_at_1', 'recall_at_2', 'recall_at_4'] and r['count'] == 4500
  assert retrieval_double.calls[-1][2] == 5            # K = max(k_list) + 1
  ev.reset()
  assert ev.count == 0
  with pytest.raises(ValueError):
    ev.result()
  ev.add(feat[:10], torch.full((10,), -1))
  assert ev.result() == {'count': 0, 'recall_at_1': 0.0, 'recall_at_2': 0.0, 'recall_at_4': 0.0}


def test_evaluator_refuses_what_the_reference_refuses(retrieval_double):
  from assembled_cnn_amd import ops
  from assembled_cnn_amd.retrieval import RecallEvaluator
  with pytest.raises(NotImplementedError):
    RecallEvaluator(similarity='dot')
  feat, lab = _set(n=64)
  sq = ops.embed_sqnorm(feat)
  with pytest.raises(NotImplementedError):
    ops.retrieval_topk(feat, feat, sq, sq, 6, similarity='manhattan')
  ev = RecallEvaluator()
  with pytest.raises(ValueError):
    ev.add(feat.float(), lab)
  with pytest.raises(ValueError):
    ev.add(feat[:, :12].contiguous(), lab)
  with pytest.raises(ValueError):
    ev.add(feat, lab[:10])
  ev.add(feat, lab)
  with pytest.raises(ValueError):
    ev.add(torch.zeros(4, 8, dtype=torch.bfloat16), lab[:4])


def test_sharded_index_merges_to_the_whole(retrieval_double):
  """ops level: three uneven shards of the index with index_base, merged by topk_merge, equal one call over the whole index"""
  from assembled_cnn_amd import ops
  feat, _ = _set(n=300)
  feat[40:60] = feat[10:30]                           # exact ties across shards
  sq = ops.embed_sqnorm(feat)
  val, idx = ops.retrieval_topk(feat, feat, sq, sq, 6, 'euclidean')
  vs, is_ = [], []
  for lo, hi in ((0, 37), (37, 250), (250, 300)):
    v, i = ops.retrieval_topk(feat, feat[lo:hi], sq, sq[lo:hi], 6, 'euclidean', index_base=lo)
    vs.append(v)
    is_.append(i)
  mv, mi = ops.topk_merge(torch.stack(vs, 1).contiguous(), torch.stack(is_, 1).contiguous())
  assert torch.equal(mi, idx) and torch.equal(mv, val)
