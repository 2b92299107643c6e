"""Corruption robustness (mCE on ImageNet-C) on the device: the reference's ``mce/eval_robustness.py`` without the
TensorFlow session around it.

  data_dir/<corruption>/<severity 1..5>/<synset>/<file>  (list_images)                 eval_robustness.py:191-196
  -> label = synsets2idx[synset folder] + label_offset  (label_of)                      :151-158, :216-219
  -> "bypass" preprocessing: decode, exactly image_size x image_size, minus the means   :123-137
  -> inference forward (Trainer.eval_logits), arg-max, top-1 hit                        :183-187, :222-226
  -> error per corruption pooled over its five severities, / AlexNet's, mean = mCE      :231-232, :276-281, :297-302

The tail runs as one launch per batch (ops.eval_groups): every row's hit is added into the int32 counters of its group,
group = corruption * 5 + severity - 1, so a batch may span severities and corruptions and nothing is read back before
``result``.  The flip-rate metric (``robustness_type=fr``) is not implemented, as in the reference (:323-324).
"""
from __future__ import annotations

import glob
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import input_pipeline, jpeg as _jpeg, ops, staging

# AlexNet's error per corruption, the normaliser of CE (:91-97, in that order)
ALEXNET_CE = {
    'gaussian_noise': 0.8864, 'shot_noise': 0.8945, 'impulse_noise': 0.9226,
    'defocus_blur': 0.8199, 'glass_blur': 0.8263, 'motion_blur': 0.7860, 'zoom_blur': 0.7984,
    'snow': 0.8668, 'frost': 0.8266, 'fog': 0.8193, 'brightness': 0.5646,
    'contrast': 0.8532, 'elastic_transform': 0.6461, 'pixelate': 0.7178, 'jpeg_compression': 0.6065,
    'speckle_noise': 0.8454, 'gaussian_blur': 0.7871, 'spatter': 0.7175, 'saturate': 0.6583,
}
# AlexNet's flip probabilities (:115-120): data only, the reference never reads them either
ALEXNET_FP = {
    'gaussian_noise': 0.23653, 'shot_noise': 0.30062, 'motion_blur': 0.09297,
    'zoom_blur': 0.05942, 'spatter': 0.05053, 'brightness': 0.04889,
    'translate': 0.11007, 'rotate': 0.13104, 'tilt': 0.07050, 'scale': 0.23531,
    'speckle_noise': 0.18649, 'gaussian_blur': 0.02775, 'snow': 0.11928, 'shear': 0.10658,
}
DISTORTIONS = list(ALEXNET_CE)
SEVERITIES = 5                                   # :192
GROUPS = len(DISTORTIONS) * SEVERITIES           # 95; row GROUPS of the counters takes the rows outside every group


def split_distortions(num_workers: int) -> List[List[str]]:
  """The corruptions of each of ``num_workers`` workers (process, :249-273): consecutive runs of DISTORTIONS, the first
  19 % num_workers workers taking one more; a worker beyond the 19th gets none."""
  if num_workers < 1:
    raise ValueError('num_workers must be positive')
  base, extra = divmod(len(DISTORTIONS), num_workers)
  ends, at = [], 0
  for i in range(num_workers):
    at += base + (1 if i < extra else 0)
    ends.append(at)
  return [DISTORTIONS[(ends[i - 1] if i else 0):ends[i]] for i in range(num_workers)]


def synsets_to_index(label_file: str) -> Dict[str, int]:
  """get_synsets2idx (:151-158): line i of the label file, stripped, blanks to underscores, lower case -> i"""
  with open(label_file, 'r') as f:
    synsets = [l.strip().replace(' ', '_').lower() for l in f.readlines()]
  return {s: i for i, s in enumerate(synsets)}


def label_of(path, synsets2idx: Dict[str, int], label_offset: int = 1) -> int:
  """:216-219: the name of the folder a file lies in is its synset; the label is that synset's line + label_offset"""
  if isinstance(path, bytes):
    path = path.decode('utf-8')
  fn = os.path.splitext(path)[0]
  return synsets2idx[os.path.basename(os.path.dirname(fn))] + label_offset


def list_images(data_dir: str, distortion: str) -> List[Tuple[str, int, str]]:
  """(path, severity, synset folder) of every file of a corruption, severities 1..5 (:191-196); folders and files in sorted
  order (the reference takes the directory's own order; the counters do not depend on it)"""
  out = []
  for severity in range(1, SEVERITIES + 1):
    severity_dir = os.path.join(data_dir, distortion, str(severity))
    for d in sorted(os.listdir(severity_dir)):
      for f in sorted(glob.glob(os.path.join(severity_dir, d) + '/*')):
        out.append((f, severity, d))
  return out


def _frame_size(data) -> Optional[Tuple[int, int]]:
  """(height, width) from the frame header of an encoded JPEG, None for anything else.  A walk over the marker segments in
  front of the first scan: the size check of the bypass preprocessing must not depend on who parses the file later."""
  a = _jpeg._as_array(data)
  n = a.size
  if n < 4 or a[0] != 0xFF or a[1] != 0xD8:
    return None
  at = 2
  while at + 4 <= n:
    if a[at] != 0xFF:
      return None
    m = int(a[at + 1])
    if m == 0xFF:                                  # fill byte
      at += 1
      continue
    if m == 0xD9 or m == 0xDA:
      return None
    seglen = (int(a[at + 2]) << 8) | int(a[at + 3])
    if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):      # SOFn
      if seglen < 7 or at + 9 > n:
        return None
      return (int(a[at + 5]) << 8) | int(a[at + 6]), (int(a[at + 7]) << 8) | int(a[at + 8])
    if seglen < 2:
      return None
    at += 2 + seglen
  return None


def summarize(errors: Dict[str, float]) -> dict:
  """CE and mCE from the error rate of every evaluated corruption: ce = error / AlexNet's (:278), the two means (:297-300)
  over the corruptions given"""
  ce = {n: e / ALEXNET_CE[n] for n, e in errors.items()}
  return {'ce': ce, 'mce': float(np.mean(list(ce.values()))), 'mce_unnormalized': float(np.mean(list(errors.values())))}


def report(result: dict) -> List[str]:
  """the reference's lines: one per corruption (:282-284), then the two means (:301-302)"""
  lines = ['Distortion: {:15s}  | CE (unnormalized) (%): {:.2f}  | CE (normalized) (%): {:.2f}'.format(
      n, 100 * result['error'][n], 100 * result['ce'][n]) for n in result['error']]
  lines.append('mCE (normalized by AlexNet errors) (%): {:.2f}'.format(100 * result['mce']))
  lines.append('mCE (unnormalized) (%): {:.2f}'.format(100 * result['mce_unnormalized']))
  return lines


class CorruptionEvaluator(object):
  """Top-1 / top-5 error per corruption and severity, accumulated on the device batch by batch.

  ``trainer``: a train.Trainer holding the model under evaluation; ``image_size``: the side every image must have (the bypass
  preprocessing does not resize); ``distortions``: the corruptions this evaluator is asked for -- a worker's quota.  The
  counters are int32 [96, 3] = {images, top-1 hits, top-5 hits} per group of ALL 19 corruptions whatever the quota, so the
  counters of workers with different quotas add up element by element."""

  def __init__(self, trainer, image_size: int, distortions: Sequence[str] = DISTORTIONS):
    distortions = list(distortions)
    for n in distortions:
      if n not in ALEXNET_CE:
        raise ValueError('unknown corruption %r' % (n,))
    if len(set(distortions)) != len(distortions):
      raise ValueError('a corruption is named twice')
    if image_size < 1:
      raise ValueError('image_size must be positive')
    self.trainer = trainer
    self.image_size = int(image_size)
    self.distortions = distortions
    self._index = {n: DISTORTIONS.index(n) for n in distortions}
    self._window = dict(crop_y=0, crop_x=0, crop_h=self.image_size, crop_w=self.image_size, resize_h=self.image_size,
                        resize_w=self.image_size, out_y=0, out_x=0, flip=0)
    self.reset()

  def reset(self):
    self.counts = torch.zeros((GROUPS + 1, 3), dtype=torch.int32, device=self.trainer.model.device)

  def preprocess(self, entries: Sequence, dct_method: str = 'INTEGER_ACCURATE', jpeg_fallback=None,
                 jpeg_progressive: bool = False, jpeg_entropy: str = 'sequential', jpeg_parse: str = 'host',
                 jpeg_resident=None) -> torch.Tensor:
    """The bypass preprocessing (:123-137) of encoded JPEGs and decoded uint8 [H, W, 3] arrays: float32 NHWC on the
    device, float32(pixel) - CHANNEL_MEANS bit for bit.  It is input_pipeline.preprocess_batch with identity windows: at
    scale 1 the legacy bilinear returns its top-left tap exactly.  ValueError for an entry that is not image_size x
    image_size.  An encoded entry without a JPEG frame header is decoded by ``jpeg_fallback`` here."""
    entries = list(entries)
    S = self.image_size
    for k, e in enumerate(entries):
      if _jpeg.is_encoded(e):
        size = _frame_size(e)
        if size is None:
          if jpeg_fallback is None:
            raise NotImplementedError('entry %d is not a JPEG file and no jpeg_fallback was given' % k)
          e = entries[k] = _jpeg._check_decoded(jpeg_fallback(e), k)
          size = e.shape[:2]
      else:
        size = _jpeg._check_decoded(e, k).shape[:2]
      if tuple(size) != (S, S):
        raise ValueError('entry %d is %d x %d, the evaluation needs %d x %d (the bypass preprocessing does not resize)'
                         % (k, size[0], size[1], S, S))
    return input_pipeline.preprocess_batch(
        entries, False, self.trainer.model.device, image_size=S, preprocessing_type='imagenet',
        windows=[self._window] * len(entries), dct_method=dct_method, jpeg_fallback=jpeg_fallback,
        jpeg_progressive=jpeg_progressive, jpeg_entropy=jpeg_entropy, jpeg_parse=jpeg_parse, jpeg_resident=jpeg_resident)

  def groups_of(self, n: int, distortion, severities) -> np.ndarray:
    """int32 [n] group ids: corruption * 5 + severity - 1; -1 (counted as skipped) for a severity outside 1..5.
    ``distortion`` / ``severities``: one value for the whole batch or one per entry."""
    names = [distortion] * n if isinstance(distortion, str) else list(distortion)
    sev = [int(severities)] * n if np.ndim(severities) == 0 else [int(s) for s in severities]
    if len(names) != n or len(sev) != n:
      raise ValueError('one corruption and one severity per entry')
    for name in set(names):
      if name not in self._index:
        raise ValueError('corruption %r is not one this evaluator was asked for' % (name,))
    return np.asarray([self._index[name] * SEVERITIES + s - 1 if 1 <= s <= SEVERITIES else -1
                       for name, s in zip(names, sev)], dtype=np.int32)

  def add(self, entries: Sequence, labels: Sequence[int], distortion, severities, **jpeg_options):
    """One batch: preprocess, forward, and the hits added into the counters of every entry's group.  Nothing is read back.
    ``jpeg_options``: dct_method, jpeg_fallback, jpeg_progressive, jpeg_entropy, jpeg_parse, jpeg_resident of
    input_pipeline.preprocess_batch."""
    B = len(entries)
    if B == 0:
      return
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    if labels.size != B:
      raise ValueError('%d labels for %d entries' % (labels.size, B))
    table = np.stack([labels.astype(np.int32), self.groups_of(B, distortion, severities)])
    images = self.preprocess(entries, **jpeg_options)
    m = self.trainer.model
    tab = staging.upload_table(table, m.device).view(torch.int32).view(2, B)
    self.trainer.eval_logits(images)
    ops.eval_groups(m.logits_padded, m.ldc, tab[0], tab[1], B, self.trainer.p.num_classes, GROUPS, self.counts)

  def result(self, reduce: bool = True) -> dict:
    """Reads the counters once.  With an initialised process group and ``reduce`` they are all-reduced (SUM) first, so every
    rank reports every rank's corruptions.  Keys: 'error' / 'top5_error' / 'ce' per corruption that has images (1 - hits /
    images pooled over the severities, :231-232; ce = error / AlexNet's, :278), 'error_by_severity'[name][severity] (None
    for a severity without images), 'mce' / 'mce_unnormalized' (means over those corruptions, :297-300), 'images',
    'skipped'.  A corruption this evaluator was asked for that has no image is an AssertionError (:231)."""
    c = self.counts.clone()
    names = list(self.distortions)
    if reduce:
      import torch.distributed as dist
      if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(c, op=dist.ReduceOp.SUM)
        names = None                                # every rank's quota: whatever has images
    c = c.cpu().numpy().astype(np.int64)
    g = c[:GROUPS].reshape(len(DISTORTIONS), SEVERITIES, 3)
    pooled = g.sum(axis=1)
    for n in self.distortions:
      assert pooled[self._index[n], 0] > 0, 'no image of corruption %r was evaluated' % (n,)
    if names is None:
      names = [n for i, n in enumerate(DISTORTIONS) if pooled[i, 0] > 0]
    error, top5, by_sev = {}, {}, {}
    for n in names:
      i = DISTORTIONS.index(n)
      error[n] = 1 - 1. * int(pooled[i, 1]) / int(pooled[i, 0])
      top5[n] = 1 - 1. * int(pooled[i, 2]) / int(pooled[i, 0])
      by_sev[n] = {s + 1: (1 - 1. * int(g[i, s, 1]) / int(g[i, s, 0])) if g[i, s, 0] else None for s in range(SEVERITIES)}
    out = {'error': error, 'top5_error': top5, 'error_by_severity': by_sev, 'images': int(c[:GROUPS, 0].sum()),
           'skipped': int(c[GROUPS, 0])}
    out.update(summarize(error))
    return out


def _read(path: str) -> bytes:
  with open(path, 'rb') as f:
    return f.read()


def evaluate_tree(trainer, data_dir: str, label_file: str, image_size: int, batch_size: int,
                  distortions: Optional[Iterable[str]] = None, label_offset: int = 1, evaluator=None, **jpeg_options):
  """The loop of show_corruption_error_by_distortion (:161-234) over ``distortions`` (default: all 19): every file of
  data_dir/<corruption>/<1..5>/<synset>/ in batches of ``batch_size`` (the last one short: drop_remainder=False, :146).
  Returns the CorruptionEvaluator (``evaluator``, or a fresh one); call result() on it."""
  if batch_size < 1:
    raise ValueError('batch_size must be positive')
  distortions = list(DISTORTIONS if distortions is None else distortions)
  ev = evaluator if evaluator is not None else CorruptionEvaluator(trainer, image_size, distortions)
  synsets2idx = synsets_to_index(label_file)
  for name in distortions:
    files = list_images(data_dir, name)
    for s in range(0, len(files), batch_size):
      chunk = files[s:s + batch_size]
      ev.add([_read(p) for p, _, _ in chunk], [label_of(p, synsets2idx, label_offset) for p, _, _ in chunk], name,
             [sev for _, sev, _ in chunk], **jpeg_options)
  return ev
