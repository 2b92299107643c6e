"""One eager training step of a small Assemble network -- selective-kernel units, anti-aliased strided blocks, BigLittle
merges (tests/model_parity.py: 'a-r50-beta1-d') -- with the folded resampling steps on (default) and off
(ASM_SK_BLUR=0 ASM_BL_SUM=0): loss rows, logits and the whole gradient arena must be the same bits.  The launch count of the
step must fall by what the folds remove: two launches per strided unit that qualifies, one per merge."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BATCH, SIZE = 4, 64


def _step(monkeypatch, **env):
  from assembled_cnn_amd import ops
  from assembled_cnn_amd.model import Model
  from tests import model_parity as mp
  for k in ('ASM_SK_BLUR', 'ASM_BL_SUM'):
    monkeypatch.delenv(k, raising=False)
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  ops.refresh_tuning()
  try:
    pm = Model(num_classes=1001, device='cuda', zero_gamma=False, seed=0, **mp.CONFIGS['a-r50-beta1-d'])
    pm.build((SIZE, SIZE), use_resnet_d=True)
    _, x, labels = mp.inputs(BATCH, SIZE)
    n0 = ops.L().asm_launch_count()
    logits = pm(x.cuda(), True, use_resnet_d=True)
    oh = ops.onehot(labels.cuda(), BATCH, 1001)
    rows, dz = ops.softmax_ce(pm.logits_padded, pm.ldc, oh, None, BATCH, 1001, 0.1, 0.0, 1.0, pm.ldc)
    pm.backward(dz)
    torch.cuda.synchronize()
    launches = ops.L().asm_launch_count() - n0
    return dict(rows=rows.cpu(), logits=logits.float().cpu().contiguous(), grads=pm.arena.g32.cpu()), launches
  finally:
    for k in env:
      monkeypatch.delenv(k, raising=False)
    ops.refresh_tuning()


def test_training_step_is_bit_identical_with_the_folds_on_and_off(hip_lib, monkeypatch):
  on, n_on = _step(monkeypatch)
  off, n_off = _step(monkeypatch, ASM_SK_BLUR='0', ASM_BL_SUM='0')
  assert torch.isfinite(on['grads']).all() and float(on['grads'].abs().sum()) > 0
  for k in on:
    assert torch.equal(on[k].view(torch.int32), off[k].view(torch.int32)), '%s differs' % k
  assert n_on < n_off, 'the folded step launches %d kernels, the un-folded one %d' % (n_on, n_off)
