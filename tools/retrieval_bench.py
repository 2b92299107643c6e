#!/usr/bin/env python
"""Time asm_retrieval_topk (K <= 64) / asm_retrieval_topk_wide (K above it, or --selection wide) against the materialising form
of the reference (metric/recall_metric.py:98-110, 182-205) on the same GPU, in the same process, alternating, three runs each:

  fused          ops.retrieval_topk[_wide] over query chunks of 8192 (RecallEvaluator's default) -- the [Q, N] matrix is never stored
  materialising  torch.matmul of the normalised bf16 operands + torch.topk, queries cut into pieces of 10 000 as the
                 reference cuts them (a framework GEMM: this tool only, the product links no BLAS)

    python tools/retrieval_bench.py [--shapes 8192x128,60502x128,60502x2048] [--k 6] [--runs 3] [--similarity cosine]
                                    [--selection auto|list|wide]

Prints per shape the best and median time of each side, TFLOP/s (2 Q N D) and the ratio; one JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def counted(ops, x, sq, k, similarity):
  """one pass through asm_debug_retrieval_topk_wide_counted (include/asm_hip_debug.h): the counters, per query"""
  from assembled_cnn_amd import lib
  L = lib.load()
  N, D = x.shape
  cnt = torch.zeros(3, dtype=torch.int64, device='cuda')
  for s in range(0, N, 8192):
    q, sqq = x[s:s + 8192], sq[s:s + 8192]
    Q = q.shape[0]
    need = ops.retrieval_topk_wide_workspace_bytes(Q, N, k)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    val = torch.empty((Q, k), dtype=torch.float32, device='cuda')
    idx = torch.empty((Q, k), dtype=torch.int32, device='cuda')
    rc = L.asm_debug_retrieval_topk_wide_counted(ops._ptr(q), D, ops._ptr(x), D, ops._ptr(sqq), ops._ptr(sq), Q, N, D,
                                                 ops.SIMILARITIES[similarity], k, 0, ops._ptr(val), ops._ptr(idx), ops._ptr(ws),
                                                 need, ops._stream(), ops._ptr(cnt))
    assert rc == 0, L.asm_last_error()
    torch.cuda.synchronize()
  c = cnt.cpu().tolist()
  return dict(appended_per_query=c[0] / N, walk_compactions_per_query=c[1] / N, end_compactions_per_query=c[2] / N)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', default='8192x128,60502x128,60502x2048')
  ap.add_argument('--k', type=int, default=6)
  ap.add_argument('--runs', type=int, default=3)
  ap.add_argument('--similarity', default='cosine')
  ap.add_argument('--selection', default='auto', choices=['auto', 'list', 'wide'])
  ap.add_argument('--counters', action='store_true', help='wide selection: one more, untimed pass through the counting test entry')
  a = ap.parse_args()
  from assembled_cnn_amd import ops
  wide = ops.topk_selection(a.k, a.selection) == 'wide'
  topk = ops.retrieval_topk_wide if wide else ops.retrieval_topk
  out = []
  for shape in a.shapes.split(','):
    N, D = (int(v) for v in shape.split('x'))
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn((N, D), generator=g, device='cuda').to(torch.bfloat16)
    sq = ops.embed_sqnorm(x)

    def fused():
      idx = []
      for s in range(0, N, 8192):
        idx.append(topk(x[s:s + 8192], x, sq[s:s + 8192], sq, a.k, a.similarity)[1])
      return torch.cat(idx)

    def materialising():
      if a.similarity == 'cosine':
        xn = (x.float() / x.float().norm(dim=1, keepdim=True).clamp_min(1e-6)).to(torch.bfloat16)
      idx = []
      for s in range(0, N, 10000):
        if a.similarity == 'cosine':
          sim = torch.matmul(xn[s:s + 10000], xn.t()).float()
        else:
          sim = -(sq[s:s + 10000, None] + sq[None, :] - 2.0 * torch.matmul(x[s:s + 10000], x.t()).float())
        idx.append(torch.topk(sim, a.k, dim=1, sorted=True)[1])
      return torch.cat(idx)

    def timed(fn):
      torch.cuda.synchronize()
      t = time.perf_counter()
      r = fn()
      torch.cuda.synchronize()
      return time.perf_counter() - t, r
    timed(fused), timed(materialising)                      # warm-up (allocator, kernel load)
    tf, tm = [], []
    for _ in range(a.runs):                                 # alternating: both sides see the same box in the same state
      t, fi = timed(fused)
      tf.append(t)
      t, mi = timed(materialising)
      tm.append(t)
    agree = float((fi[:, 0] == mi[:, 0].to(torch.int32)).float().mean())
    flop = 2.0 * N * N * D
    rec = dict(Q=N, N=N, D=D, K=a.k, selection='wide' if wide else 'list', similarity=a.similarity,
               fused_ms=[round(t * 1e3, 3) for t in tf],
               materialising_ms=[round(t * 1e3, 3) for t in tm], fused_tflops=round(flop / min(tf) / 1e12, 2),
               materialising_tflops=round(flop / min(tm) / 1e12, 2), ratio=round(min(tm) / min(tf), 3),
               top1_agreement=round(agree, 4))
    print('Q=N=%d D=%d K=%d %s: fused best %.2f ms median %.2f ms (%.1f TFLOP/s) | materialising best %.2f ms median %.2f ms '
          '(%.1f TFLOP/s) | materialising / fused = %.2f | top-1 agreement %.4f'
          % (N, D, a.k, a.similarity, min(tf) * 1e3, sorted(tf)[len(tf) // 2] * 1e3, rec['fused_tflops'], min(tm) * 1e3,
             sorted(tm)[len(tm) // 2] * 1e3, rec['materialising_tflops'], rec['ratio'], agree), flush=True)
    if a.counters and wide:
      rec.update(counted(ops, x, sq, a.k, a.similarity))
      print('  per query: %.1f candidates appended, %.2f compactions during the walk, %.2f at the end of a run'
            % (rec['appended_per_query'], rec['walk_compactions_per_query'], rec['end_compactions_per_query']), flush=True)
    out.append(rec)
    del x, sq
    torch.cuda.empty_cache()
  print(json.dumps(out))


if __name__ == '__main__':
  main()
