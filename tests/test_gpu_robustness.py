"""CorruptionEvaluator on the GPU: a seeded Assemble-ResNet-50 at 64 x 64, batches of 8 that span severities and
corruptions, entries partly decoded arrays and partly JPEG files.  Teacher-forced: the counters are compared with
tests/robustness_ref.eval_groups applied to the logits the same forward left in model.logits_padded, so the comparison is
exact; result() is compared with the formulae of mce/eval_robustness.py:231-232, :278, :297-300 in float64."""
import io

import numpy as np
import pytest
import torch

from tests import preprocess_ref as P
from tests import robustness_ref as RR

pytestmark = pytest.mark.gpu

SIDE, BATCH = 64, 8
NAMES = ['shot_noise', 'fog', 'saturate']


def _jpeg_bytes(img):
  try:
    from PIL import Image
  except ImportError:
    return None
  buf = io.BytesIO()
  Image.fromarray(img).save(buf, format='JPEG', quality=90)
  return buf.getvalue()


def _entries():
  """two images per (corruption, severity), in that order; every other one as a JPEG file where Pillow is there"""
  rng = np.random.default_rng(11)
  entries, names, sev = [], [], []
  for n in NAMES:
    for s in range(1, 6):
      for k in range(2):
        img = rng.integers(0, 256, (SIDE // 8, SIDE // 8, 3), dtype=np.uint8).repeat(8, 0).repeat(8, 1)
        img = (img.astype(np.int32) + rng.integers(-8, 9, img.shape)).clip(0, 255).astype(np.uint8)
        data = _jpeg_bytes(img) if k else None
        entries.append(data if data is not None else img)
        names.append(n)
        sev.append(s)
  return entries, names, sev


def test_counters_follow_the_forward_and_result_the_formulae(hip_lib):
  from assembled_cnn_amd import jpeg, robustness as R
  from assembled_cnn_amd.train import HParams, Trainer
  hp = HParams(resnet_version=2, use_sk_block=True, anti_alias_type='sconv', anti_alias_filter_size=3, use_resnet_d=True,
               zero_gamma=True, batch_size=BATCH)
  tr = Trainer(hp, seed=3, device='cuda', recorded=False)
  ev = R.CorruptionEvaluator(tr, SIDE, NAMES)
  entries, names, sev = _entries()
  n = len(entries)
  assert n == 30
  # the bypass pixels: a decoded entry is its bytes minus the means bit for bit, an encoded one the device's own decode
  x = ev.preprocess(entries[:4]).cpu().numpy()
  for k in range(4):
    px = entries[k]
    if jpeg.is_encoded(px):
      buf, offs, sizes = jpeg.decode_batch([px], 'cuda')
      assert tuple(sizes[0]) == (SIDE, SIDE)
      px = buf[int(offs[0]):int(offs[0]) + 3 * SIDE * SIDE].cpu().numpy()
    assert np.array_equal(x[k], np.asarray(px).reshape(SIDE, SIDE, 3).astype(np.float32) - P.CHANNEL_MEANS), k

  C, ldc = hp.num_classes, tr.model.ldc
  assert ldc % 4 == 0 and ldc >= C
  rng = np.random.default_rng(12)
  labels = rng.integers(1, C, n)
  want = np.zeros((R.GROUPS + 1, 3), np.int64)
  logits = []
  for rnd in range(2):        # the second round repeats the images, with every other label set to the first round's prediction
    for s in range(0, n, BATCH):
      e = min(n, s + BATCH)
      ev.add(entries[s:e], labels[s:e], names[s:e], sev[s:e])
      z = tr.model.logits_padded.view(-1, ldc)[:e - s, :C].float().cpu().numpy()
      assert np.isfinite(z).all()
      groups = [R.DISTORTIONS.index(nm) * 5 + sv - 1 for nm, sv in zip(names[s:e], sev[s:e])]
      want, pred = RR.eval_groups(z, labels[s:e], groups, R.GROUPS, counts=want)
      if rnd == 0:
        logits.append(pred)
    if rnd == 0:
      pred = np.concatenate(logits)
      labels = np.where(np.arange(n) % 2 == 0, pred, labels)
  got = ev.counts.cpu().numpy().astype(np.int64)
  assert np.array_equal(got, want), np.argwhere(got != want)[:5]
  assert want[:, 0].sum() == 2 * n and want[R.GROUPS].sum() == 0 and want[:, 1].sum() >= n // 2
  used = sorted(R.DISTORTIONS.index(nm) for nm in NAMES)
  assert sorted(set(np.flatnonzero(want[:95, 0]) // 5)) == used and (want[:95, 0][want[:95, 0] > 0] == 4).all()

  res = ev.result()
  g = want[:95].reshape(19, 5, 3).astype(np.float64)
  for nm in NAMES:
    i = R.DISTORTIONS.index(nm)
    err = 1.0 - g[i, :, 1].sum() / g[i, :, 0].sum()
    assert res['error'][nm] == err and res['ce'][nm] == err / R.ALEXNET_CE[nm]
    assert res['top5_error'][nm] == 1.0 - g[i, :, 2].sum() / g[i, :, 0].sum()
    assert [res['error_by_severity'][nm][s] for s in range(1, 6)] == [1.0 - g[i, s, 1] / g[i, s, 0] for s in range(5)]
  assert list(res['error']) == NAMES and res['images'] == 2 * n and res['skipped'] == 0
  assert res['mce'] == float(np.mean([res['ce'][nm] for nm in NAMES]))
  assert res['mce_unnormalized'] == float(np.mean([res['error'][nm] for nm in NAMES]))
  assert len(R.report(res)) == len(NAMES) + 2


def test_a_wrong_size_is_refused_before_anything_runs(hip_lib):
  from assembled_cnn_amd import ops, robustness as R
  from assembled_cnn_amd.train import HParams, Trainer
  tr = Trainer(HParams(zero_gamma=True, batch_size=2), seed=1, device='cuda', recorded=False)
  ev = R.CorruptionEvaluator(tr, SIDE)
  small = _jpeg_bytes(np.zeros((SIDE, SIDE - 8, 3), np.uint8))
  bad = small if small is not None else np.zeros((SIDE, SIDE - 8, 3), np.uint8)
  calls = ops.abi_calls()
  with pytest.raises(ValueError, match=r'entry 1 is 64 x 56, the evaluation needs 64 x 64'):
    ev.add([np.zeros((SIDE, SIDE, 3), np.uint8), bad], [1, 2], 'fog', 1)
  assert ops.abi_calls() == calls and int(ev.counts.sum()) == 0
