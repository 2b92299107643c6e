"""Recall@K for K up to 1023 on the GPU: the wide selection (candidate buffers + radix select) against the fp64 oracle of
tests/retrieval_ref.py and against the list selection, whose GEMM and epilogue it shares."""
import numpy as np
import pytest
import torch

from tests import retrieval_ref as ref

pytestmark = pytest.mark.gpu


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).cuda()


def _wide(ops, q, x, k, similarity, **kw):
  val, idx = ops.retrieval_topk_wide(q, x, ops.embed_sqnorm(q), ops.embed_sqnorm(x), k, similarity, **kw)
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
@pytest.mark.parametrize('Q,N,K', [(3000, 3000, 1001), (3000, 3000, 101), (300, 1025, 65), (129, 127, 200), (1, 5, 1024),
                                   (700, 700, 64)])
def test_exact_inputs_give_the_stable_argsort_order(hip_lib, similarity, Q, N, K):
  """Integer-valued embeddings: every product and sum is exact in fp32 and the rows tie heavily across the K boundary, so the
  indices must EQUAL the stable-argsort reference (tie rule, compaction, run merge, tails) and the euclidean values must equal
  it bit for bit."""
  from assembled_cnn_amd import ops
  x = _exact_set(N, similarity, 3)
  q = x[:Q] if Q <= N else _exact_set(Q, similarity, 4)
  val, idx = _wide(ops, _dev(q), _dev(x), K, similarity)
  sim = ref.similarity(q, x, similarity)
  wv, wi = ref.top_k(sim, K)
  kk = wi.shape[1]
  assert kk == min(K, N)
  if N > K:
    full = -np.sort(-sim, axis=1)
    print('exact %s Q=%d N=%d K=%d: K-th and (K+1)-th fp64 value equal in %d of %d rows'
          % (similarity, Q, N, K, int((full[:, K - 1] == full[:, K]).sum()), Q))
  assert np.array_equal(idx[:, :kk], wi)
  assert (idx[:, kk:] == -1).all() and np.isneginf(val[:, kk:]).all()
  if similarity == 'euclidean':
    assert np.array_equal(val[:, :kk], wv.astype(np.float32))
  else:
    assert np.abs(val[:, :kk] - wv).max() <= 2 * 64 * 2.0 ** -24


def _random_set(N, D, ncls, noise, seed=0):
  rng = np.random.RandomState(seed)
  lab = rng.randint(0, ncls, size=N)
  cent = rng.randn(ncls, D)
  x = _dev(cent[lab] + noise * rng.randn(N, D))
  lab[N - N // 37:] = -1
  return x, lab


RANDOM_SETS = [(4096, 128, 256, 2.0), (1537, 200, 64, 3.0)]


@pytest.mark.parametrize('similarity', ['cosine', 'euclidean'])
@pytest.mark.parametrize('N,D,ncls,noise', RANDOM_SETS)
def test_the_two_selections_agree_bit_for_bit(hip_lib, similarity, N, D, ncls, noise):
  """One GEMM and one epilogue serve both kernels: the first 64 of the wide selection's 200 ARE the list selection's 64."""
  from assembled_cnn_amd import ops
  x, lab = _random_set(N, D, ncls, noise)
  q = x[torch.from_numpy(lab != -1).cuda()].contiguous()
  sqq, sqx = ops.embed_sqnorm(q), ops.embed_sqnorm(x)
  wv, wi = ops.retrieval_topk_wide(q, x, sqq, sqx, 200, similarity)
  lv, li = ops.retrieval_topk(q, x, sqq, sqx, 64, similarity)
  assert torch.equal(wi[:, :64], li) and torch.equal(wv[:, :64], lv)
  wv, wi = ops.retrieval_topk_wide(q, x, sqq, sqx, 6, similarity)
  lv, li = ops.retrieval_topk(q, x, sqq, sqx, 6, similarity)
  assert torch.equal(wi, li) and torch.equal(wv, lv)


def _tau(D, similarity, x64):
  """the worst-case bound of a length-D fp32 accumulation of exact products, doubled"""
  t = 2.0 * D * 2.0 ** -24
  return t if similarity == 'cosine' else t * 4.0 * float((x64 * x64).sum(1).max())


def _check_rows(val, idx, sim, tau):
  """the every-row checks"""
  Q, N = sim.shape
  assert (idx >= 0).all() and (idx < N).all()
  got = np.take_along_axis(sim, idx.astype(np.int64), 1)
  err = np.abs(val.astype(np.float64) - got).max()
  print('max |value - fp64| = %.3g (tau %.3g)' % (err, tau))
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


@pytest.mark.parametrize('similarity', ['cosine', 'euclidean'])
@pytest.mark.parametrize('N,D,ncls,noise', [(4096, 128, 256, 2.0), (3000, 2048, 100, 3.0)])
def test_random_inputs_against_fp64_at_k_1001(hip_lib, similarity, N, D, ncls, noise):
  """Every row, no share exempted: indices in range, no duplicates, values within tau of the fp64 similarity at the returned
  index, order and tie rule, nothing better than the K-th value + tau left out; and rank by rank |val[:, j] - sorted fp64[:, j]|
  <= tau (an order statistic moves by at most the largest perturbation of an element)."""
  from assembled_cnn_amd import ops
  K = 1001
  x, lab = _random_set(N, D, ncls, noise)
  q = x[torch.from_numpy(lab != -1).cuda()].contiguous()
  val, idx = _wide(ops, q, x, K, similarity)
  x64 = x.float().cpu().double().numpy()
  sim = ref.similarity(x64[lab != -1], x64, similarity)
  tau = _tau(D, similarity, x64)
  _check_rows(val, idx, sim, tau)
  ranked = -np.sort(-sim, axis=1)[:, :K]
  err = np.abs(val.astype(np.float64) - ranked).max()
  print('%s N=%d D=%d: max rank-wise |value - fp64| = %.3g (tau %.3g)' % (similarity, N, D, err, tau))
  assert err <= tau


@pytest.mark.parametrize('similarity', ['cosine', 'euclidean'])
@pytest.mark.parametrize('K', [101, 1001])
def test_run_to_run_and_shard_invariance(hip_lib, similarity, K):
  from assembled_cnn_amd import ops
  N, D, ncls, noise = RANDOM_SETS[0]
  x, lab = _random_set(N, D, ncls, noise)
  q = x[torch.from_numpy(lab != -1).cuda()].contiguous()
  sqq, sqx = ops.embed_sqnorm(q), ops.embed_sqnorm(x)
  wv, wi = ops.retrieval_topk_wide(q, x, sqq, sqx, K, similarity)
  wv, wi = wv.clone(), wi.clone()
  v2, i2 = ops.retrieval_topk_wide(q, x, sqq, sqx, K, similarity)
  assert torch.equal(i2, wi) and torch.equal(v2, wv)
  vals, idxs = [], []
  for lo, hi in ((0, 131), (131, 3000), (3000, N)):      # at K = 1001 the first shard is shorter than K: unused slots
    v, i = ops.retrieval_topk_wide(q, x[lo:hi], sqq, sqx[lo:hi].contiguous(), K, similarity, index_base=lo)
    vals.append(v.clone())
    idxs.append(i.clone())
  assert int(idxs[0].min()) == (-1 if K > 131 else 0) and int(idxs[1].min()) >= 131 and int(idxs[2].min()) >= 3000
  mv, mi = ops.topk_merge_wide(torch.stack(vals, 1).contiguous(), torch.stack(idxs, 1).contiguous())
  assert torch.equal(mi, wi) and torch.equal(mv, wv)
  with pytest.raises(NotImplementedError):
    ops.retrieval_topk_wide(q, x, sqq, sqx, 1025, similarity)


@pytest.mark.parametrize('similarity', ['euclidean', 'cosine'])
def test_evaluator_end_to_end_at_r_1000(hip_lib, similarity):
  """Exact inputs, so RecallEvaluator must EQUAL the fp64 oracle at every depth.  Distractors are the last rows (interleaved,
  the reference's self-match quirk would saturate every recall at 1)."""
  from assembled_cnn_amd.retrieval import RecallEvaluator
  N = 3000
  k_list = (1, 10, 100, 1000)
  x = _exact_set(N, similarity, 3)
  lab = np.random.RandomState(7).randint(0, 700, size=N)
  lab[N - N // 37:] = -1
  want = ref.recall_at_k(x, lab, k_list, similarity)
  print(similarity, 'fp64', want)
  assert 0.0 < want['recall_at_100'] < want['recall_at_1000'] < 1.0
  xd, labels = _dev(x), torch.from_numpy(lab)
  for chunk in (8192, 1000, 7):
    ev = RecallEvaluator(k_list, similarity, query_chunk=chunk)
    assert ev.selection == 'wide'
    for s in range(0, N, 500):
      ev.add(xd[s:s + 500], labels[s:s + 500])
    got = ev.result()
    print(similarity, 'chunk', chunk, got)
    assert got == want


def test_a_zero_similarity_is_written_as_plus_zero(hip_lib):
  """The header's one stated difference from the list selection: the euclidean similarity of a row with itself is -(0) = -0 in
  the epilogue both kernels share; the wide selection ranks -0 as +0 (as the list's float compare does) and writes +0."""
  from assembled_cnn_amd import ops
  x = _dev(_exact_set(300, 'euclidean', 3))
  sq = ops.embed_sqnorm(x)
  wv, wi = ops.retrieval_topk_wide(x, x, sq, sq, 65, 'euclidean')
  lv, li = ops.retrieval_topk(x, x, sq, sq, 64, 'euclidean')
  assert torch.equal(wi[:, 0].cpu(), torch.arange(300, dtype=torch.int32)) and torch.equal(wi[:, :64], li)
  assert (wv[:, 0] == 0).all() and (lv[:, 0] == 0).all()
  assert not torch.signbit(wv[:, 0]).any() and torch.signbit(lv[:, 0]).all()
