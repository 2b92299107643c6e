"""Plain references of the batch-norm passes of csrc/bn.hip on activations viewed as [M, C], written from the formulas in the
kernel comments and csrc/common.h (bn_fwd_channel, bn_bwd_coefs, bwd_dx, relu_mask8 / mask8).  numpy on the CPU, float64
unless ``dtype`` says otherwise (the float32 evaluation gives a case's reference floor, rows_ref.floor_of); nothing here
calls the product.  tests/test_bn_ref_cpu.py proves every function against oracle/assembled_oracle.py and its autograd;
tests/test_gpu_bn_edges.py checks the HIP kernels against them.
"""
from __future__ import annotations

import numpy as np

from tests import rows_ref as R

F64 = np.float64
F32 = np.float32


# ---- packed ReLU mask -------------------------------------------------------------------------------------------------
def pack_mask(bits):
  """[M, C] 0/1 -> [M, C / 8] bytes: bit e of byte v gates channel 8 v + e (the inverse of rows_ref.unpack_mask)"""
  b = np.asarray(bits).astype(np.uint8)
  M, C = b.shape
  return (b.reshape(M, C // 8, 8) << np.arange(8, dtype=np.uint8)).sum(axis=2).astype(np.uint8)


def gate_of(relu, yout, C):
  """the 0/1 gate [M, C] of the three mask kinds: 0 none, 1 [forward output > 0] (zeros of either sign gate off),
  2 the packed mask bytes [M, C / 8]"""
  if relu == 0:
    return None
  if relu == 1:
    return (np.asarray(yout, F64) > 0).astype(F64)
  return R.unpack_mask(yout, C).astype(F64)


# ---- forward ----------------------------------------------------------------------------------------------------------
def stats(x, dtype=F64):
  """per-channel (sum x, sum x^2) over the M rows"""
  x = np.asarray(x, dtype)
  return x.sum(axis=0, dtype=dtype), (x * x).sum(axis=0, dtype=dtype)


def upsample2x(res, N, H, W):
  """[N (H/2) (W/2), C] -> [N H W, C]: nearest-neighbour 2 x (UpSampling2D((2, 2)))"""
  C = res.shape[1]
  r = np.asarray(res).reshape(N, H // 2, W // 2, C)
  return np.repeat(np.repeat(r, 2, axis=1), 2, axis=2).reshape(N * H * W, C)


def apply(x, scale, shift, residual=None, res_mode=0, relu=False, H=0, W=0, dtype=F64):
  """pre = x scale + shift [+ residual (res_mode 1) | + upsample2x(residual) (res_mode 2)]; y = relu ? max(pre, 0) : pre.
  -> (y before the bf16 rounding, mask bits [pre > 0], pre)"""
  x = np.asarray(x, dtype)
  pre = x * np.asarray(scale, dtype) + np.asarray(shift, dtype)
  if res_mode == 1:
    pre = pre + np.asarray(residual, dtype)
  elif res_mode == 2:
    pre = pre + upsample2x(np.asarray(residual, dtype), x.shape[0] // (H * W), H, W)
  bits = pre > 0
  return (np.maximum(pre, dtype(0)) if relu else pre), bits, pre


def fwd(x, gamma, beta, eps, momentum=0.9, mm=None, mv=None, residual=None, res_mode=0, relu=False, H=0, W=0, dtype=F64):
  """training-mode batch norm of [M, C] (bn_fwd_channel): mean = sum x / M, var = max(sum x^2 / M - mean^2, 0) (biased),
  invstd = 1 / sqrt(var + eps), scale = gamma invstd, shift = beta - mean scale, then ``apply``.  The statistics and the
  moving-statistics terms are rows_ref.bn_finalize's (float64); with another ``dtype`` the sums, E[x^2] - mean^2 and the
  coefficients are evaluated in it, which measures the cancellation of the one-pass variance.
  -> dict(y, bits, pre, mean, invstd, scale, shift [, mm_terms, mv_terms, moving_mean, moving_var])"""
  x = np.asarray(x)
  M = x.shape[0]
  out = R.bn_finalize(np.stack(stats(x))[None], M, gamma, beta, eps, momentum, mm, mv)
  if dtype != F64:
    s0, s1 = stats(x, dtype)
    mu = s0 / dtype(M)
    var = np.maximum(s1 / dtype(M) - mu * mu, dtype(0))
    invstd = dtype(1) / np.sqrt(var + dtype(eps))
    scale = np.asarray(gamma, dtype) * invstd
    out.update(mean=mu, invstd=invstd, scale=scale, shift=np.asarray(beta, dtype) - mu * scale)
  out['y'], out['bits'], out['pre'] = apply(x, out['scale'], out['shift'], residual, res_mode, relu, H, W, dtype)
  return out


def apply_dual(xa, xb, sa, ha, sb, hb, relu=False, dtype=F64):
  """out = [relu](xa sa + ha + bf16(xb sb + hb)): the shortcut's batch norm is rounded to bf16 where its own pass stored it
  -> (y before the bf16 rounding, mask bits)"""
  short = R.to_bf16(np.asarray(xb, dtype) * np.asarray(sb, dtype) + np.asarray(hb, dtype)).astype(dtype)
  pre = np.asarray(xa, dtype) * np.asarray(sa, dtype) + np.asarray(ha, dtype) + short
  return (np.maximum(pre, dtype(0)) if relu else pre), pre > 0


# ---- backward ---------------------------------------------------------------------------------------------------------
def gated(dy, gate, dtype=F64):
  dz = np.asarray(dy, dtype)
  return dz if gate is None else dz * np.asarray(gate, dtype)


def bwd_sums(dy, x, gate, mean, invstd, dtype=F64):
  """(sum dz, sum dz xhat) per channel; dz = dy gate, xhat = (x - mean) invstd"""
  dz = gated(dy, gate, dtype)
  xhat = (np.asarray(x, dtype) - np.asarray(mean, dtype)) * np.asarray(invstd, dtype)
  return dz.sum(axis=0, dtype=dtype), (dz * xhat).sum(axis=0, dtype=dtype)


def bwd_dx(dz, x, A, B, C, dtype=F64):
  """dx = A dz + B x + C"""
  return np.asarray(A, dtype) * np.asarray(dz, dtype) + np.asarray(B, dtype) * np.asarray(x, dtype) + np.asarray(C, dtype)


def bwd(dy, x, gate, gamma, mean, invstd, M):
  """-> dict(dgamma, dbeta, A, B, C, dz, dx): dx = gamma invstd (dz - dbeta / M - xhat dgamma / M) through
  rows_ref.bn_bwd_finalize's coefficients"""
  out = R.bn_bwd_finalize(np.stack(bwd_sums(dy, x, gate, mean, invstd))[None], M, gamma, mean, invstd)
  out['dz'] = gated(dy, gate)
  out['dx'] = bwd_dx(out['dz'], x, out['A'], out['B'], out['C'])
  return out


def bwd2(dy, xa, xb, gate, bn_a, bn_b, M):
  """two batch norms behind one ReLU: both consume dz = dy gate.  bn_a / bn_b = (gamma, mean, invstd) -> (bwd of a, bwd of b)"""
  return bwd(dy, xa, gate, bn_a[0], bn_a[1], bn_a[2], M), bwd(dy, xb, gate, bn_b[0], bn_b[1], bn_b[2], M)
