"""Recall@K on the GPU: the fused similarity + top-K kernel, the list merge, the hit counter and RecallEvaluator against the
fp64 oracle of tests/retrieval_ref.py (which tests/test_retrieval_cpu.py ties to the reference's own get_recall)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import retrieval_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
K = 6


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).cuda()


def _topk(ops, q, x, k, similarity, **kw):
  val, idx = ops.retrieval_topk(q, x, ops.embed_sqnorm(q), ops.embed_sqnorm(x), k, similarity, **kw)
  torch.cuda.synchronize()
  return val.cpu().numpy(), idx.cpu().numpy()


def _exact_set(n, similarity, seed):
  rng = np.random.RandomState(seed)
  if similarity == 'euclidean':
    return rng.randint(-2, 3, size=(n, 64)).astype(np.float32)
  x = np.zeros((n, 64), np.float32)                  # 16 entries of +-1 per row: every |x|^2 is 16, rsqrt(16) is exact
  for r in range(n):
    x[r, rng.permutation(64)[:16]] = rng.choice([-1.0, 1.0], size=16)
  return x


@pytest.mark.parametrize('similarity', ['euclidean', 'cosine'])
@pytest.mark.parametrize('Q,N', [(1000, 1000), (1, 5), (300, 1023), (300, 1025), (129, 127)])
def test_exact_inputs_give_the_stable_argsort_order(hip_lib, similarity, Q, N):
  """Integer-valued embeddings: every product and sum is exact in fp32 and exact ties are plentiful, so the indices must EQUAL
  the stable-argsort reference (tie rule, split merge, tails) and the euclidean values must equal it bit for bit."""
  from assembled_cnn_amd import ops
  x = _exact_set(N, similarity, 3)
  q = x[:Q] if Q <= N else _exact_set(Q, similarity, 4)
  val, idx = _topk(ops, _dev(q), _dev(x), K, similarity)
  sim = ref.similarity(q, x, similarity)
  wv, wi = ref.top_k(sim, K)
  kk = wi.shape[1]
  ties = int((wv[:, 1:] == wv[:, :-1]).sum())
  print('exact %s Q=%d N=%d: %d tied neighbours in the reference rows' % (similarity, Q, N, ties))
  assert np.array_equal(idx[:, :kk], wi)
  assert (idx[:, kk:] == -1).all() and np.isneginf(val[:, kk:]).all()
  if similarity == 'euclidean':
    assert np.array_equal(val[:, :kk], wv.astype(np.float32))
    if N >= 100:
      assert ties > 0
  else:
    assert np.abs(val[:, :kk] - wv).max() <= 2 * 64 * 2.0 ** -24


def _random_set(N, D, ncls, noise, seed=0):
  rng = np.random.RandomState(seed)
  lab = rng.randint(0, ncls, size=N)
  cent = rng.randn(ncls, D)
  x = _dev(cent[lab] + noise * rng.randn(N, D))
  lab[N - N // 37:] = -1
  return x, lab


def _tau(D, similarity, x64):
  """the worst-case bound of a length-D fp32 accumulation of exact products, doubled"""
  t = 2.0 * D * 2.0 ** -24
  return t if similarity == 'cosine' else t * 4.0 * float((x64 * x64).sum(1).max())


def _check_rows(val, idx, sim, tau):
  """the every-row checks; returns the fp64 similarities sorted descending"""
  Q, N = sim.shape
  got = np.take_along_axis(sim, idx.astype(np.int64), 1)
  err = np.abs(val.astype(np.float64) - got).max()
  print('max |value - fp64| = %.3g (tau %.3g)' % (err, tau))
  assert (idx >= 0).all() and (idx < N).all()
  assert err <= tau
  assert (val[:, 1:] <= val[:, :-1]).all()
  same = val[:, 1:] == val[:, :-1]
  assert (idx[:, 1:][same] > idx[:, :-1][same]).all()
  srt = np.sort(idx, 1)
  assert (srt[:, 1:] != srt[:, :-1]).all(), 'an index appears twice'
  rest = sim.copy()
  np.put_along_axis(rest, idx.astype(np.int64), -np.inf, 1)
  over = rest.max(1) - (val[:, -1].astype(np.float64) + tau)
  print('best index left out vs K-th value + tau: max %.3g' % over.max())
  assert (over <= 0).all()


RANDOM_SETS = [(4096, 128, 256, 2.0), (1537, 200, 64, 3.0)]


@pytest.mark.parametrize('similarity', ['cosine', 'euclidean'])
@pytest.mark.parametrize('N,D,ncls,noise', RANDOM_SETS + [(3000, 2048, 100, 3.0)])
def test_random_inputs_against_fp64(hip_lib, similarity, N, D, ncls, noise):
  """Every row: values within tau of the fp64 similarity at the returned indices, ordered, no duplicates, nothing better left
  out.  Rows whose first K + 1 fp64 values are more than 2 tau apart: the indices equal the reference; at most 10 % of the rows
  may be left out of that (the fp64 reference alone leaves out 1.7 % / 4.3 % and 2.3 % / 8.0 % on these inputs).  D = 2048 gets the every-row checks
  only: its worst-case tau makes 44 % of the rows formally ambiguous."""
  from assembled_cnn_amd import ops
  x, lab = _random_set(N, D, ncls, noise)
  q = x[torch.from_numpy(lab != -1).cuda()].contiguous()
  val, idx = _topk(ops, q, x, K, similarity)
  x64 = x.float().cpu().double().numpy()
  sim = ref.similarity(x64[lab != -1], x64, similarity)
  tau = _tau(D, similarity, x64)
  _check_rows(val, idx, sim, tau)
  if D == 2048:
    return
  order = np.argsort(-sim, axis=1, kind='stable')[:, :K + 1]
  top = np.take_along_axis(sim, order, 1)
  clear = ((top[:, :-1] - top[:, 1:]) > 2 * tau).all(1)
  left_out = 1.0 - clear.mean()
  print('%s N=%d D=%d: %.1f %% of the rows left out of the exact-index check' % (similarity, N, D, 100 * left_out))
  assert left_out <= 0.10
  assert np.array_equal(idx[clear], order[clear, :K])


@pytest.mark.parametrize('k_list', [[1, 5], [1, 2, 4]])
def test_recall_accumulate_equals_get_recall_on_the_device_rows(hip_lib, k_list):
  from assembled_cnn_amd import ops
  x, lab = _random_set(1537, 200, 64, 3.0)
  lab[5::11] = -1                                    # interleaved distractors: positions in the query list and the index part
  sel = lab != -1
  q = x[torch.from_numpy(sel).cuda()].contiguous()
  kk = max(k_list) + 1
  _, idx = ops.retrieval_topk(q, x, ops.embed_sqnorm(q), ops.embed_sqnorm(x), kk, 'cosine')
  qlab = torch.from_numpy(lab[sel]).to(torch.int32).cuda()
  ilab = torch.from_numpy(lab).to(torch.int32).cuda()
  kd = torch.tensor(k_list, dtype=torch.int32, device='cuda')
  hits = torch.zeros(len(k_list), dtype=torch.int32, device='cuda')
  Q = q.shape[0]
  for s, e in ((0, 500), (500, 501), (501, Q)):      # query_base != 0
    ops.recall_accumulate(idx[s:e].contiguous(), qlab[s:e].contiguous(), ilab, s, kd, hits)
  want = ref.get_hits(idx.cpu().numpy(), lab[sel], lab, k_list)
  assert hits.cpu().tolist() == [want[k] for k in k_list]
  assert 0 < want[k_list[0]] < Q


def test_recall_accumulate_on_the_reference_fixture(hip_lib):
  from assembled_cnn_amd import ops
  cases = json.load(open(os.path.join(HERE, 'golden', 'reference_recall.json')))['cases']
  for c in cases:
    idx = torch.tensor(c['sorted_idx'], dtype=torch.int32, device='cuda')
    hits = torch.zeros(len(c['k_list']), dtype=torch.int32, device='cuda')
    ops.recall_accumulate(idx, torch.tensor(c['query_labels'], dtype=torch.int32, device='cuda'),
                          torch.tensor(c['labels'], dtype=torch.int32, device='cuda'), 0,
                          torch.tensor(c['k_list'], dtype=torch.int32, device='cuda'), hits)
    got = {str(k): h / float(len(c['query_labels'])) for k, h in zip(c['k_list'], hits.cpu().tolist())}
    assert got == c['recall'], c['name']


@pytest.mark.parametrize('similarity', ['cosine', 'euclidean'])
def test_evaluator_end_to_end(hip_lib, similarity):
  from assembled_cnn_amd import ops
  from assembled_cnn_amd.retrieval import RecallEvaluator
  N, D, ncls, noise = RANDOM_SETS[0]
  x, lab = _random_set(N, D, ncls, noise)
  labels = torch.from_numpy(lab)
  x64 = x.float().cpu().double().numpy()
  want = ref.recall_at_k(x64, lab, (1, 5), similarity)
  sel = lab != -1
  sim = ref.similarity(x64[sel], x64, similarity)
  top = -np.sort(-sim, axis=1)[:, :K + 1]
  left_out = int((~((top[:, :-1] - top[:, 1:]) > 2 * _tau(D, similarity, x64)).all(1)).sum())
  Q = int(sel.sum())
  results = []
  for chunk in (8192, 1000, 7, 8192):                # the last one: a second run of the first
    ev = RecallEvaluator((1, 5), similarity, query_chunk=chunk)
    for s in range(0, N, 500):
      ev.add(x[s:s + 500], labels[s:s + 500])
    results.append(ev.result())
  print(similarity, results[0], 'fp64', want, 'rows left out', left_out)
  assert results[0]['count'] == Q == want['count']
  for k in (1, 5):
    assert abs(results[0]['recall_at_%d' % k] - want['recall_at_%d' % k]) <= left_out / float(Q)
  assert results[1] == results[0] and results[2] == results[0] and results[3] == results[0]
  if similarity == 'cosine':
    assert abs(want['recall_at_1'] - 0.593) < 0.05 and abs(want['recall_at_5'] - 0.882) < 0.05   # non-trivial: a wrong ranking moves it
  # the index cut in three uneven shards by hand, merged with asm_topk_merge
  q = x[torch.from_numpy(sel).cuda()].contiguous()
  sqq, sqx = ops.embed_sqnorm(q), ops.embed_sqnorm(x)
  vals, idxs = [], []
  for lo, hi in ((0, 131), (131, 3000), (3000, N)):
    v, i = ops.retrieval_topk(q, x[lo:hi], sqq, sqx[lo:hi].contiguous(), K, similarity, index_base=lo)
    vals.append(v)
    idxs.append(i)
  mv, mi = ops.topk_merge(torch.stack(vals, 1).contiguous(), torch.stack(idxs, 1).contiguous())
  wv, wi = ops.retrieval_topk(q, x, sqq, sqx, K, similarity)
  assert torch.equal(mi, wi) and torch.equal(mv, wv)
  hits = torch.zeros(2, dtype=torch.int32, device='cuda')
  ops.recall_accumulate(mi, labels[sel].to(torch.int32).cuda(), labels.to(torch.int32).cuda(), 0,
                        torch.tensor([1, 5], dtype=torch.int32, device='cuda'), hits)
  assert [h / float(Q) for h in hits.cpu().tolist()] == [results[0]['recall_at_1'], results[0]['recall_at_5']]


def test_topk_at_the_largest_k(hip_lib):
  """K = 64 (the cap; dynamic LDS above 64 KB) and K = 33 on exact inputs"""
  from assembled_cnn_amd import ops
  x = _exact_set(700, 'euclidean', 5)
  sim = ref.similarity(x, x, 'euclidean')
  for k in (33, 64):
    val, idx = _topk(ops, _dev(x), _dev(x), k, 'euclidean')
    wv, wi = ref.top_k(sim, k)
    assert np.array_equal(idx, wi) and np.array_equal(val, wv.astype(np.float32))
  with pytest.raises(NotImplementedError):
    _topk(ops, _dev(x), _dev(x), 65, 'euclidean')


def test_trainer_embed_is_the_models_embedding_in_bf16(hip_lib):
  from assembled_cnn_amd.retrieval import RecallEvaluator
  from assembled_cnn_amd.train import HParams, Trainer
  tr = Trainer(HParams(resnet_size=101, pool_type='gem', embedding_size=128, batch_size=16), seed=0, device='cuda')
  g = torch.Generator().manual_seed(1)
  ev = RecallEvaluator((1, 5))
  total = 0
  for b in range(2):
    x = (torch.randn(16, 64, 64, 3, generator=g) * 40.0).cuda()
    emb = tr.embed(x)
    assert emb.dtype == torch.bfloat16 and tuple(emb.shape) == (16, 128) and emb.is_contiguous()
    emb = emb.clone()
    full = tr.model(x, False, use_resnet_d=tr.p.use_resnet_d, return_embedding=True)
    assert full.dtype == torch.float32 and torch.equal(emb.float(), full)
    lab = torch.arange(16) % 4
    lab[b::5] = -1
    total += int((lab != -1).sum())
    ev.add(emb, lab)
  r = ev.result()
  assert r['count'] == total and 0.0 <= r['recall_at_1'] <= r['recall_at_5'] <= 1.0
