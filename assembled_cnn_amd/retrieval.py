"""Recall@K of a retrieval model on the device: the reference's ``metric/recall_metric.recall_at_k`` (its evaluation under
``--zeroshot_eval``, nets/run_loop_classification.py:439-445) without the Estimator / TFRecord plumbing around it.

  embeddings of the validation set (Trainer.embed, bf16) + labels        recall_metric.py:132-148
  -> queries = rows with label != -1, in their original order; index = all rows        :151-159
  -> similarity + top_k(max(k_list) + 1), fused (ops.retrieval_topk / _wide)            :98-110
  -> get_recall (ops.recall_accumulate)                                                 :217-228
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops


class RecallEvaluator(object):
  """Collects the embeddings of an evaluation set batch by batch and scores them.

  ``k_list`` / ``similarity`` are the flags ``recall_at_k`` / ``eval_similarity`` (nets/hparams_config.py:39,273).  As in the
  reference, a query's own entry is removed from its result row by comparing the row's INDEX positions with the query's
  position in the QUERY list (:221-222), so a self-match stays in the row of every query that a distractor precedes.

  ``selection`` names the top-K kernel for K = max(k_list) + 1: 'list' (ops.retrieval_topk, K <= 64), 'wide'
  (ops.retrieval_topk_wide, K <= 1024) or 'auto', the list kernel where it applies and the wide one above it.
  """

  def __init__(self, k_list: Sequence[int] = (1, 5), similarity: str = 'cosine', query_chunk: int = 8192,
               selection: str = 'auto'):
    if similarity not in ops.SIMILARITIES:
      raise NotImplementedError('eval_similarity %r (cosine | euclidean)' % (similarity,))     # :107-108
    self.k_list = [int(k) for k in k_list]
    if not self.k_list or min(self.k_list) < 1:
      raise ValueError('k_list must hold positive integers')
    if query_chunk < 1:
      raise ValueError('query_chunk must be positive')
    # K = max(k_list) + 1 (:110); a K above the cap is refused here, before an evaluation set has been embedded
    self.selection = ops.topk_selection(max(self.k_list) + 1, selection)
    self.similarity = similarity
    self.query_chunk = int(query_chunk)
    self.reset()

  def reset(self):
    self.count = 0                                  # rows added so far
    self._emb: Optional[torch.Tensor] = None        # bf16 [capacity, D]
    self._lab: Optional[torch.Tensor] = None        # int32 [capacity]

  def _reserve(self, rows: int, like: torch.Tensor):
    cap = 0 if self._emb is None else self._emb.shape[0]
    if rows <= cap:
      return
    new_cap = max(rows, 2 * cap, 1024)              # geometric growth: O(1) copies per row over a whole evaluation
    emb = torch.empty((new_cap, like.shape[1]), dtype=torch.bfloat16, device=like.device)
    lab = torch.empty((new_cap,), dtype=torch.int32, device=like.device)
    if self.count:
      emb[:self.count].copy_(self._emb[:self.count])
      lab[:self.count].copy_(self._lab[:self.count])
    self._emb, self._lab = emb, lab

  def add(self, embeddings_bf16: torch.Tensor, labels: torch.Tensor):
    """One batch: embeddings bf16 [B, D] (D % 8 == 0), labels [B] integers, -1 for a distractor."""
    e = embeddings_bf16
    if e.dim() != 2 or e.dtype != torch.bfloat16:
      raise ValueError('embeddings must be a 2-D bfloat16 tensor')
    if e.shape[1] % 8:
      raise ValueError('embedding size %d is not a multiple of 8' % e.shape[1])
    if labels.numel() != e.shape[0]:
      raise ValueError('%d labels for %d embeddings' % (labels.numel(), e.shape[0]))
    if self._emb is not None and self._emb.shape[1] != e.shape[1]:
      raise ValueError('embedding size changed from %d to %d' % (self._emb.shape[1], e.shape[1]))
    B = e.shape[0]
    self._reserve(self.count + B, e)
    self._emb[self.count:self.count + B].copy_(e)
    self._lab[self.count:self.count + B].copy_(labels.reshape(-1).to(device=e.device, dtype=torch.int32))
    self.count += B

  def _gathered(self, reduce: bool):
    """(embeddings [N, D], labels [N], rank, world): with a process group, every rank's rows in rank order"""
    emb, lab = self._emb[:self.count], self._lab[:self.count]
    if reduce:
      import torch.distributed as dist
      if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        world, rank = dist.get_world_size(), dist.get_rank()
        n = torch.tensor([self.count], dtype=torch.int64, device=emb.device)
        counts = [torch.zeros_like(n) for _ in range(world)]
        dist.all_gather(counts, n)
        counts = [int(c) for c in counts]
        top = max(counts)
        pe = torch.zeros((top, emb.shape[1]), dtype=emb.dtype, device=emb.device)
        pl = torch.full((top,), -1, dtype=lab.dtype, device=lab.device)
        pe[:self.count].copy_(emb)
        pl[:self.count].copy_(lab)
        es = [torch.empty_like(pe) for _ in range(world)]
        ls = [torch.empty_like(pl) for _ in range(world)]
        dist.all_gather(es, pe)
        dist.all_gather(ls, pl)
        emb = torch.cat([t[:c] for t, c in zip(es, counts)])
        lab = torch.cat([t[:c] for t, c in zip(ls, counts)])
        return emb, lab, rank, world
    return emb, lab, 0, 1

  def result(self, reduce: bool = True) -> dict:
    """{'recall_at_<k>': hits / Q for k in k_list, 'count': Q} (the keys of recall_metric.py:177-178).  With an initialised
    process group and ``reduce``: embeddings and labels are all-gathered in rank order, every rank scores its own contiguous
    range of the queries against the whole index and the hit counts are all-reduced, so every rank reports the whole set."""
    if self.count == 0:
      raise ValueError('no embeddings were added')
    emb, lab, rank, world = self._gathered(reduce)
    N = emb.shape[0]
    qpos = torch.nonzero(lab != -1).reshape(-1)                     # :151-154
    Q = int(qpos.numel())
    out = {'count': Q}
    if Q == 0:
      out.update(('recall_at_%d' % k, 0.0) for k in self.k_list)
      return out
    if Q == N:
      qemb, qlab = emb, lab
    else:
      qemb, qlab = emb.index_select(0, qpos).contiguous(), lab.index_select(0, qpos).contiguous()
    K = max(self.k_list) + 1                                        # :110
    k_dev = torch.tensor(self.k_list, dtype=torch.int32, device=emb.device)
    hits = torch.zeros((len(self.k_list),), dtype=torch.int32, device=emb.device)
    emb = emb.contiguous()
    lab = lab.contiguous()
    sq = ops.embed_sqnorm(emb)
    sqq = sq if Q == N else ops.embed_sqnorm(qemb)
    lo, hi = Q * rank // world, Q * (rank + 1) // world             # this rank's queries
    topk = ops.retrieval_topk if self.selection == 'list' else ops.retrieval_topk_wide
    for s in range(lo, hi, self.query_chunk):
      e = min(hi, s + self.query_chunk)
      _, idx = topk(qemb[s:e], emb, sqq[s:e], sq, K, self.similarity)
      ops.recall_accumulate(idx, qlab[s:e], lab, s, k_dev, hits)
    if world > 1:
      import torch.distributed as dist
      dist.all_reduce(hits, op=dist.ReduceOp.SUM)
    h = hits.cpu().tolist()
    out.update(('recall_at_%d' % k, h[i] / float(Q)) for i, k in enumerate(self.k_list))
    return out
