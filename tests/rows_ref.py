"""Plain references of the row, loss, metric, DropBlock and bookkeeping kernels, written from the definitions the kernel
comments quote (losses/cls_losses.py, nets/blocks.py GeM and DropBlock, tf.nn.in_top_k, tf.argmax, the layout comments of
include/asm_hip.h).  numpy on the CPU, float64 unless ``dtype`` says otherwise; nothing here calls the product or
tests/cpu_double.py.  tests/test_rows_ref_cpu.py checks every function against oracle/assembled_oracle.py;
tests/test_gpu_rows_edges.py checks the HIP kernels against them.

The references whose kernel writes bf16 take ``dtype``: evaluated once in float64 and once with float32 arithmetic, the
largest difference between the two is that case's REFERENCE FLOOR (``floor_of``): what a correct fp32 evaluation may differ
from the exact answer by, measured on the reference alone.
"""
from __future__ import annotations

import numpy as np

F64 = np.float64
F32 = np.float32
U24 = 2.0 ** -24      # half an ulp of float32, relative
BF16_ULP = 2.0 ** -8  # one ulp of bfloat16, relative


# ---- number formats ---------------------------------------------------------------------------------------
def to_bf16(x) -> np.ndarray:
  """float32 -> the nearest bfloat16 (ties to even), returned as float32 (finite inputs)"""
  b = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
  b = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
  return b.astype(np.uint32).view(F32).reshape(np.shape(x))


def ulp32(x) -> np.ndarray:
  """one float32 ulp at |x|"""
  return np.spacing(np.abs(np.asarray(x, dtype=F32))).astype(F64)


def floor_of(fn):
  """reference floor of a case: max |fn(float64) - fn(float32)| over every array fn returns"""
  a, b = fn(F64), fn(F32)
  if not isinstance(a, (tuple, list)):
    a, b = (a,), (b,)
  return max(float(np.max(np.abs(np.asarray(x, F64) - np.asarray(y, F64)))) if np.size(x) else 0.0 for x, y in zip(a, b))


# ---- losses -------------------------------------------------------------------------------------------------
def sigmoid_ce(logits, targets, scale, dtype=F64):
  """losses/cls_losses.py:34-38: ce = max(z, 0) - z t + log(1 + exp(-|z|)) (tf.nn.sigmoid_cross_entropy_with_logits),
  loss = sum(ce) / sum(targets).  -> (loss, sum(targets), d(scale * loss) / dz [B, C])"""
  z, t = np.asarray(logits, dtype), np.asarray(targets, dtype)
  ce = np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))
  tot = t.sum(dtype=dtype)
  e = np.exp(-np.abs(z))
  sig = np.where(z >= 0, 1 / (1 + e), e / (1 + e))
  return ce.sum(dtype=dtype) / tot, tot, (sig - t) * dtype(scale) / tot


def _log_softmax(z):
  d = z - z.max(axis=1, keepdims=True)
  return d - np.log(np.exp(d).sum(axis=1, keepdims=True))


def softmax_ce(logits, targets, teacher, eps, T, scale, dtype=F64):
  """tf.losses.softmax_cross_entropy with label smoothing y (1 - eps) + eps / C, plus (teacher given) the distillation term
  T^2 * CE(logits / T, teacher) of nets/run_loop_classification.py:156-162; ``teacher`` holds probabilities.
  -> (loss per row [B], d(scale * mean over rows) / dz [B, C])"""
  z, y = np.asarray(logits, dtype), np.asarray(targets, dtype)
  B, C = z.shape
  yy = y * dtype(1.0 - eps) + dtype(eps / C)
  lp = _log_softmax(z)
  rows = -(yy * lp).sum(axis=1)
  g = np.exp(lp) * yy.sum(axis=1, keepdims=True) - yy
  if teacher is not None:
    t = np.asarray(teacher, dtype)
    lpt = _log_softmax(z / dtype(T))
    rows = rows + dtype(T * T) * -(t * lpt).sum(axis=1)
    g = g + dtype(T) * (np.exp(lpt) * t.sum(axis=1, keepdims=True) - t)
  return rows, g * dtype(scale / B)


# ---- evaluation metrics ---------------------------------------------------------------------------------------
def eval_rows(logits, labels):
  """nets/run_loop_classification.py:208-219.  pred = tf.argmax (the LOWEST index among equal maxima); conf = the largest
  softmax probability; top1 = [pred == label]; top5 = tf.nn.in_top_k(k=5): the label is in the top 5 unless 5 or more logits
  are STRICTLY larger than the label's (ties count for the label), and never for a label outside [0, C).
  -> pred int64 [B], conf f64 [B], top1 [B], top5 [B]"""
  z = np.asarray(logits, F64)
  B, C = z.shape
  pred, conf, top1, top5 = np.zeros(B, np.int64), np.zeros(B), np.zeros(B), np.zeros(B)
  for b in range(B):
    best = 0
    for c in range(1, C):
      if z[b, c] > z[b, best]:
        best = c
    pred[b] = best
    conf[b] = 1.0 / np.exp(z[b] - z[b, best]).sum()
    lab = int(labels[b])
    top1[b] = 1.0 if best == lab else 0.0
    if 0 <= lab < C:
      top5[b] = 1.0 if int((z[b] > z[b, lab]).sum()) < 5 else 0.0
  return pred, conf, top1, top5


# ---- GeM ---------------------------------------------------------------------------------------------------------
GEM_EPS = float(F32(1e-6))      # the definition's epsilon is a float32 constant of the graph
GEM_MAX = float(F32(1e12))


def gem(x, p, dy=None, dtype=F64):
  """nets/blocks.py:22-42 on x [N, HW, C]: s = max(sum_hw clip(x, eps, 1e12)^p, eps); y = HW^(-1/p) s^(1/p).
  Gradient: the clip passes it only strictly inside (eps, 1e12), the max only where the sum exceeds eps.
  -> (y [N, C], s [N, C], dx [N, HW, C] or None)"""
  x = np.asarray(x, dtype)
  N, HW, C = x.shape
  p = dtype(p)
  xc = np.clip(x, dtype(GEM_EPS), dtype(GEM_MAX))
  raw = (xc ** p).sum(axis=1)
  s = np.maximum(raw, dtype(GEM_EPS))
  k = dtype(HW) ** (-1 / p)
  y = k * s ** (1 / p)
  dx = None
  if dy is not None:
    g = np.asarray(dy, dtype).reshape(N, 1, C) * k * (s ** (1 / p - 1)).reshape(N, 1, C) * xc ** (p - 1)
    inside = (x > dtype(GEM_EPS)) & (x < dtype(GEM_MAX)) & (raw > dtype(GEM_EPS)).reshape(N, 1, C)
    dx = np.where(inside, g, dtype(0))
  return y, s, dx


# ---- DropBlock -----------------------------------------------------------------------------------------------------
def dropblock_keep(u, gamma, H, W, bs):
  """nets/blocks.py:187-244 with the draw ``u`` [H-bs+1, W-bs+1, C] given: seeds = relu(sign(gamma - u)) in float32 (a draw
  EQUAL to gamma is no seed), zero padded by (tl, br) = (bs - 1 - (bs - 1) // 2, (bs - 1) // 2) to H x W, dilated by a
  bs x bs stride-1 SAME max-pool ([TF-sem] SAME at stride 1 pads (bs - 1) // 2 before, the rest after); keep = 1 - that."""
  u = np.asarray(u, F32)
  hs, ws, C = u.shape
  assert hs == H - bs + 1 and ws == W - bs + 1
  seed = ((F32(gamma) - u) > 0).astype(F64)
  br = (bs - 1) // 2
  tl = (bs - 1) - br
  padded = np.zeros((H, W, C))
  padded[tl:tl + hs, tl:tl + ws] = seed
  before = (bs - 1) // 2
  pool_in = np.full((H + bs - 1, W + bs - 1, C), -np.inf)
  pool_in[before:before + H, before:before + W] = padded
  keep = np.zeros((H, W, C))
  for h in range(H):
    for w in range(W):
      keep[h, w] = 1.0 - pool_in[h:h + bs, w:w + bs].reshape(bs * bs, C).max(axis=0)
  return keep


def dropblock_scale(keep):
  """nets/blocks.py:245-250: size(mask) / (sum(mask) + 1e-8), a float32 expression of the graph"""
  return F32(keep.size) / (F32(keep.sum()) + F32(1e-8))


def dropblock_apply(x, keep, scale, relu=False, relu_mask_from=None, dtype=F64):
  """x [N, H, W, C] * keep * scale, then the ReLU (forward) or the gate [relu_mask_from > 0] (backward through the ReLU)"""
  y = np.asarray(x, dtype) * (np.asarray(keep, dtype) * dtype(scale))[None]
  if relu_mask_from is not None:
    return np.where(np.asarray(relu_mask_from) > 0, y, dtype(0))
  return np.maximum(y, dtype(0)) if relu else y


# ---- UpSampling2D((2, 2)) backward ----------------------------------------------------------------------------------
def unpack_mask(mask_bits, C):
  """packed ReLU mask [rows, C / 8] bytes -> [rows, C] 0/1: bit e of byte v gates channel 8 v + e"""
  m = np.asarray(mask_bits, np.uint8)
  return ((m[:, :, None] >> np.arange(8, dtype=np.uint8)[None, None, :]) & 1).reshape(m.shape[0], C)


def upsample2x_bwd(dy, mask_bits=None, dtype=F64):
  """dx[n, h, w] = sum over the 2 x 2 block of dy [N, 2 Hs, 2 Ws, C] [* mask bit]"""
  g = np.asarray(dy, dtype)
  N, H, W, C = g.shape
  if mask_bits is not None:
    g = g * unpack_mask(mask_bits, C).reshape(N, H, W, C).astype(dtype)
  g = g.reshape(N, H // 2, 2, W // 2, 2, C)
  return (g[:, :, 0, :, 0] + g[:, :, 0, :, 1]) + (g[:, :, 1, :, 0] + g[:, :, 1, :, 1])


# ---- batch-norm partials ----------------------------------------------------------------------------------------------
def compact(partials, groups):
  """[blocks, 2, C] -> [groups, 2, C]: group g sums blocks [g per, (g + 1) per), per = ceil(blocks / groups) (float64)"""
  p = np.asarray(partials, F64)
  per = -(-p.shape[0] // groups)
  return np.stack([p[g * per:(g + 1) * per].sum(axis=0) for g in range(groups)])


def bn_finalize(partials, M, gamma, beta, eps, momentum, mm, mv):
  """(sum x, sum x^2) partials over M rows -> tf.layers.batch_normalization(fused=True) training statistics [TF-sem]:
  biased variance for the normalisation, Bessel-corrected variance into the moving average, ``momentum`` weighs the OLD
  moving value.  eps and momentum are float32 arguments of the ABI."""
  p = np.asarray(partials, F64).sum(axis=0)
  eps, mom = float(F32(eps)), float(F32(momentum))
  mu = p[0] / M
  var = np.maximum(p[1] / M - mu * mu, 0.0)
  invstd = 1.0 / np.sqrt(var + eps)
  scale = np.asarray(gamma, F64) * invstd
  out = dict(mean=mu, invstd=invstd, scale=scale, shift=np.asarray(beta, F64) - mu * scale)
  if mm is not None:
    unbiased = var * (M / max(M - 1, 1))
    out['mm_terms'] = (np.asarray(mm, F64) * mom, mu * (1.0 - mom))
    out['mv_terms'] = (np.asarray(mv, F64) * mom, unbiased * (1.0 - mom))
    out['moving_mean'] = sum(out['mm_terms'])
    out['moving_var'] = sum(out['mv_terms'])
  return out


def bn_bwd_finalize(partials, M, gamma, mean, invstd, raw=False):
  """(sum dz, sum dz xhat) partials [raw: (sum dz, sum dz y), y the batch norm's input] -> dbeta, dgamma and the coefficients
  of dx = A dz + B x + C:  dx = gamma invstd (dz - dbeta / M - xhat dgamma / M), xhat = (x - mean) invstd."""
  p = np.asarray(partials, F64).sum(axis=0)
  g, mu, is_ = np.asarray(gamma, F64), np.asarray(mean, F64), np.asarray(invstd, F64)
  db, dg = p[0], p[1]
  if raw:
    dg = is_ * (dg - mu * db)
  A = g * is_
  B = -g * is_ * is_ * dg / M
  return dict(dbeta=db, dgamma=dg, A=A, B=B, C=-g * is_ * db / M - B * mu)


# ---- layouts ------------------------------------------------------------------------------------------------------------
def stem_lanes(ksize):
  return (4 * ksize + 7) & ~7


def stem_pack(w):
  """master [K][k][k][3] float32 -> bf16 rows [K][k][L], L = round_up(4 k, 8): element s * 4 + c, every other lane zero"""
  w = np.asarray(w, F32)
  K, k = w.shape[0], w.shape[1]
  out = np.zeros((K, k, stem_lanes(k)), F32)
  for s in range(k):
    for c in range(3):
      out[:, :, s * 4 + c] = to_bf16(w[:, :, s, c])
  return out


def stem_unpack(dwp, ksize):
  """gradient [K][k][L] float32 -> [K][k][k][3]: dw[k][r][s][c] = dwp[k][r][s * 4 + c]"""
  dwp = np.asarray(dwp, F32)
  out = np.zeros((dwp.shape[0], ksize, ksize, 3), F32)
  for s in range(ksize):
    for c in range(3):
      out[:, :, s, c] = dwp[:, :, s * 4 + c]
  return out


def filter_transpose(w, ldk=0):
  """KRSC -> CRSK with rows of ldk >= K elements; columns K .. ldk - 1 zero"""
  w = np.asarray(w)
  K = w.shape[0]
  out = np.zeros((w.shape[3], w.shape[1], w.shape[2], max(ldk, K)), w.dtype)
  out[..., :K] = np.transpose(w, (3, 1, 2, 0))
  return out


# ---- the step's first and last kernels: mixup + mean subtraction + stem halo, SGD with momentum -----------------------------------
CHANNEL_MEANS = np.array([123.68, 116.78, 103.94], F32)     # preprocessing/imagenet_preprocessing.py:46-49, float32 constants


def mixup_operands(a, mixup_type, lam1=None, lam2=None, dtype=F64):
  """utils/data_util.py:97-158 on the leading axis of ``a`` [Bin, ...] -> (first operand, second operand, lambda [Bout]), the
  last two None without mixup.  type 1 (2B -> B): a[b] with a[B + b] under lam1[b]; type 2 (B -> B): the first half as type 1,
  the second half a[b] with the REVERSED second half, a[Bin - 1 - b], under lam2[b]."""
  a = np.asarray(a, dtype)
  if mixup_type == 0:
    return a, None, None
  h = a.shape[0] // 2
  if mixup_type == 1:
    return a[:h], a[h:], np.asarray(lam1, dtype)
  return (np.concatenate([a[:h], a[:h]]), np.concatenate([a[h:], a[h:][::-1]]),
          np.concatenate([np.asarray(lam1, dtype), np.asarray(lam2, dtype)]))


def mixup_terms(a, mixup_type, lam1=None, lam2=None, dtype=F64):
  """the mixed rows as the terms of their sum: (lam a, (1 - lam) b), or (a,) without mixup"""
  fa, fb, lam = mixup_operands(a, mixup_type, lam1, lam2, dtype)
  if fb is None:
    return (fa,)
  lam = lam.reshape((-1,) + (1,) * (fa.ndim - 1))
  return lam * fa, (dtype(1) - lam) * fb


def stem_pad(x):
  """[N, H, W, 3] -> [N, H + 6, W + 6, 4]: a zero halo of 3 pixels and a zero fourth channel"""
  x = np.asarray(x)
  N, H, W, _ = x.shape
  out = np.zeros((N, H + 6, W + 6, 4), x.dtype)
  out[:, 3:3 + H, 3:3 + W, :3] = x
  return out


def mixup_meansub(images, mixup_type, lam1=None, lam2=None, dtype=F64):
  """asm_mixup_meansub before its bf16 rounding: images [Bin, H, W, 3] in 0..255 minus CHANNEL_MEANS
  (mean_image_subtraction), mixed (mixup), in the stem's padded layout"""
  x = np.asarray(images, dtype) - CHANNEL_MEANS.astype(dtype)
  return stem_pad(sum(mixup_terms(x, mixup_type, lam1, lam2, dtype)))


def sgd_terms(w, accum, grad, lr, momentum, weight_decay, grad_scale, dtype=F64):
  """tf.train.MomentumOptimizer with the L2 term folded in: g' = g grad_scale + wd w; a' = momentum a + g'; w' = w - lr a'.
  The scalars are float32 arguments of the ABI.  -> (terms of a', terms of w'): each result is the sum of its terms"""
  w, a, g = np.asarray(w, dtype), np.asarray(accum, dtype), np.asarray(grad, dtype)
  lr, mom, wd, gs = (dtype(F32(v)) for v in (lr, momentum, weight_decay, grad_scale))
  ta = (mom * a, g * gs, wd * w)
  return ta, (w,) + tuple(-lr * t for t in ta)


# ---- seeded inputs shared by the CPU and the GPU module ---------------------------------------------------------------------
def rng(*key):
  return np.random.default_rng([int(k) for k in key])


def bf16_randn(r, shape, scale=1.0):
  return to_bf16((r.standard_normal(shape) * scale).astype(F32))


def sigmoid_inputs(B, C, soft):
  """logits * 3 with +/-80 planted; one-hot targets, or (soft) the mixup blend of two one-hot rows"""
  r = rng(101, B, C, soft)
  z = (r.standard_normal((B, C)) * 3).astype(F32)
  z.reshape(-1)[::7] = 80.0
  z.reshape(-1)[3::11] = -80.0
  y = np.zeros((B, C), F32)
  y[np.arange(B), r.integers(0, C, B)] = 1.0
  if soft:
    y2 = np.zeros((B, C), F32)
    y2[np.arange(B), r.integers(0, C, B)] = 1.0
    lam = r.beta(0.2, 0.2, (B, 1)).astype(F32)
    y = lam * y + (F32(1) - lam) * y2
  return z, y


def softmax_inputs(B, C, offset):
  r = rng(102, B, C, int(offset))
  z = (r.standard_normal((B, C)) * 3).astype(F32)
  if offset:
    z[::2] += F32(offset)          # a large common offset on every other row (all rows when B = 1)
  y = np.zeros((B, C), F32)
  y[np.arange(B), r.integers(0, C, B)] = 1.0
  tl = (r.standard_normal((B, C)) * 3).astype(F64)
  t = np.exp(tl - tl.max(1, keepdims=True))
  return z, y, (t / t.sum(1, keepdims=True)).astype(F32)


def gem_inputs(N, HW, C):
  """bf16 activations with exact zeros and negatives (the clip), one all-negative column (the zero-gradient branch)"""
  r = rng(103, N, HW, C)
  x = bf16_randn(r, (N, HW, C))
  x.reshape(-1)[::5] = 0.0
  x[:, :, C // 2] = -np.abs(x[:, :, C // 2])
  return x, bf16_randn(r, (N, C))


def dropblock_gamma(kind, H, W, bs):
  """'none': 0 (keeps everything), 'all': 2 (drops everything), 'mid': the recipe's formula at keep_prob 0.8"""
  if kind == 'none':
    return F32(0.0)
  if kind == 'all':
    return F32(2.0)
  return F32(0.2 * (W * H) / (bs ** 2) / ((W - bs + 1) * (H - bs + 1)))


def dropblock_uniform(H, W, C, bs, gamma):
  """the draw [H-bs+1, W-bs+1, C] with every fifth entry EQUAL to gamma (no seed: the comparison is strict)"""
  r = rng(104, H, W, C, bs)
  u = r.random((H - bs + 1, W - bs + 1, C)).astype(F32)
  u.reshape(-1)[::5] = F32(gamma)
  return u


def partials(blocks, C, seed, positive_second=False):
  """[blocks, 2, C] float32, signs and magnitudes mixed over two decades: one dropped or doubled row moves a column sum by
  >= 1e-5 of sum |terms|, a hundred float32 ulps.  positive_second: the second row of each pair behaves like a sum of squares
  (positive, and large enough for a variance well away from zero)."""
  r = rng(105, blocks, C, seed)
  p = (r.choice([-1.0, 1.0], (blocks, 2, C)) * 10.0 ** r.uniform(-1, 1, (blocks, 2, C))).astype(F32)
  if positive_second:
    p[:, 1] = np.abs(p[:, 1]) * 400
  return p
