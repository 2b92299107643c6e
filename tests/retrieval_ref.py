"""fp64 numpy restatement of the reference's Recall@K (metric/recall_metric.py), the oracle of the retrieval tests.

  queries = rows with label != -1 in their original order, index = all rows                 :151-159
  similarity: cosine = l2_normalize(q) . l2_normalize(x) (x * rsqrt(max(sum(x^2), 1e-12))),
              euclidean = -(|q|^2 + |x|^2 - 2 q.x)                                           :98-108, :207-215
  top_k(k = max(k_list) + 1, sorted): descending, of equal values the lower index first     :110
  get_recall: drop the entries equal to the query's position IN THE QUERY LIST, map to labels,
              hit for k if the query's label is among the first k                            :217-228
"""
import numpy as np

SIMILARITIES = ('cosine', 'euclidean')


def similarity(q, x, kind):
  q = np.asarray(q, np.float64)
  x = np.asarray(x, np.float64)
  if kind == 'cosine':
    qn = q / np.sqrt(np.maximum((q * q).sum(1, keepdims=True), 1e-12))
    xn = x / np.sqrt(np.maximum((x * x).sum(1, keepdims=True), 1e-12))
    return qn @ xn.T
  if kind == 'euclidean':
    return -((q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * (q @ x.T))
  raise NotImplementedError(kind)


def top_k(sim, K):
  """(values, indices) [Q, min(K, N)]: tf.nn.top_k(sorted=True)"""
  order = np.argsort(-sim, axis=1, kind='stable')[:, :K]
  return np.take_along_axis(sim, order, 1), order


def get_recall(sorted_idx, query_labels, labels, k_list=(1, 5)):
  hits = get_hits(sorted_idx, query_labels, labels, k_list)
  return {k: hits[k] / float(len(query_labels)) for k in k_list}


def get_hits(sorted_idx, query_labels, labels, k_list=(1, 5), query_base=0):
  hits = {k: 0 for k in k_list}
  for row, top in enumerate(sorted_idx):
    qi = query_base + row
    kept = [labels[i] for i in top if i != qi]
    for k in k_list:
      if query_labels[row] in kept[:k]:
        hits[k] += 1
  return hits


def recall_at_k(features, labels, k_list=(1, 5), kind='cosine'):
  """{'recall_at_<k>': ..., 'count': Q} for the whole set, as recall_metric.recall_at_k assembles it (:151-178)"""
  labels = np.asarray(labels)
  sel = labels != -1
  sim = similarity(np.asarray(features, np.float64)[sel], features, kind)
  _, idx = top_k(sim, max(k_list) + 1)
  rec = get_recall(idx, labels[sel], labels, k_list)
  out = {'recall_at_%d' % k: rec[k] for k in k_list}
  out['count'] = int(sel.sum())
  return out
