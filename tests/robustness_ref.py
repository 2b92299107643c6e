"""Plain reference of asm_eval_groups, written from the rules in include/asm_hip.h (mce/eval_robustness.py:186-226 with
tf.nn.top_k / tf.nn.in_top_k semantics): numpy loops on the CPU, nothing here calls the product or tests/cpu_double.py.
tests/test_robustness_cpu.py pins the rules with known answers; tests/test_gpu_eval_groups.py compares the kernel with it."""
from __future__ import annotations

import numpy as np


def eval_groups(logits, labels, groups, G, counts=None):
  """logits float32 [B, C]; labels, groups int [B].
  pred: the lowest index among the largest non-NaN logits, -1 for a row without one.  top-1 hit: pred == label.  top-5 hit:
  the label lies in [0, C), its logit is finite and fewer than 5 logits are STRICTLY larger.  A row whose group lies outside
  [0, G) adds one image to row G and never a hit.
  -> (counts int64 [G + 1, 3] = {images, top-1 hits, top-5 hits}, added to ``counts`` if given; pred int64 [B])"""
  z = np.asarray(logits, np.float32)
  B, C = z.shape
  out = np.zeros((G + 1, 3), np.int64) if counts is None else np.array(counts, np.int64)
  assert out.shape == (G + 1, 3)
  pred = np.zeros(B, np.int64)
  for b in range(B):
    best = -1
    for c in range(C):
      v = z[b, c]
      if v != v:
        continue
      if best < 0 or v > z[b, best]:
        best = c
    pred[b] = best
    lab, g = int(labels[b]), int(groups[b])
    if not 0 <= g < G:
      out[G, 0] += 1
      continue
    out[g, 0] += 1
    if not 0 <= lab < C:
      continue
    if best == lab:
      out[g, 1] += 1
    zl = z[b, lab]
    if np.isfinite(zl) and int((z[b] > zl).sum()) < 5:       # a NaN is not larger than anything
      out[g, 2] += 1
  return out, pred
