#!/usr/bin/env python
"""Generate tests/golden/reference_autoaugment.{npz,json} by RUNNING the reference's preprocessing/autoaugment.py,
unmodified, under the torch-backed `tensorflow` stand-in (oracle/tf_shim) in float32:

  the four policy tables (imagenet_policies, good_policies, policy_v0, policy_vtest)          autoaugment.py:70-313
  level_to_arg for every op name at levels 0..10 with the sign draw forced each way             :702-764
  every NAME_TO_FUNC function on small images (random 24x40, random 17x17, constant 9x9)        :316-699
  distort_image_with_autoaugment end to end with a scripted tf.random_uniform                   :767-903

The shim lacks the calls only this module uses; this generator attaches its own stand-ins to the imported shim module,
in process (oracle/ stays as it is).  Each restates the TensorFlow 1.14 rule in general form, marked [TF-sem] (DESIGN.md
section 1(c)); none is derived from tests/autoaugment_ref.py or from the product.  Three arguments the policies can
produce have no defined TensorFlow result; the stand-ins implement this project's choice for two (posterize with
bits = 0 shifts by 8 -> 0; cutout with pad size 0 fills nothing) and the third (solarize with threshold 256, outside
uint8) is not recorded.

Run in the build container (needs the reference checkout); tests only read the committed fixture.
usage: python tests/golden/make_reference_autoaugment.py [--check]
"""
import inspect
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_taps as T  # noqa: E402  (import hooks)

OUT_NPZ = os.path.join(HERE, 'reference_autoaugment.npz')
OUT_JSON = os.path.join(HERE, 'reference_autoaugment.json')
F = np.float32


# ---- stand-ins attached to the shim module ------------------------------------------------------------------------
def attach_stand_ins(tf):
  Tensor, _t = tf.Tensor, tf._t
  state = dict(script=[], pos=0, log=[])

  def wrap_like(t, like):
    return Tensor(t, getattr(like, 'dtype', None))

  def np_of(x):
    return _t(x).detach().cpu().numpy()

  # tf.constant honours `shape` (the shim's ignores it) [TF-sem: the values fill a tensor of that shape]
  shim_constant = tf.constant

  def constant(value, dtype=None, shape=None, name=None):
    out = shim_constant(value, dtype)
    return Tensor(out.t.reshape([int(s) for s in shape]), out.dtype) if shape is not None else out

  # tf.cond [TF-sem]: the branch result is a tensor; a Python float becomes a float32 constant
  def cond(pred, true_fn=None, false_fn=None, **_):
    r = true_fn() if bool(_t(pred).item()) else false_fn()
    return tf.constant(r, tf.float32) if isinstance(r, float) else r

  def random_uniform(shape, minval=0, maxval=None, dtype=tf.float32, seed=None, name=None):   # noqa: A002
    """replays the scripted list: u in [0, 1) -> minval + u * (maxval - minval), floored for integer dtypes"""
    assert list(shape) == [], 'only scalar draws are scripted'
    u = state['script'][state['pos']]
    state['pos'] += 1
    lo = float(_t(minval))
    hi = 1.0 if maxval is None else float(_t(maxval))
    if dtype.is_floating:
      v = F(lo + u * (hi - lo))
      state['log'].append(float(v))
      return Tensor(torch.tensor(float(v), dtype=torch.float32), dtype)
    v = int(math.floor(lo + u * (hi - lo)))
    state['log'].append(v)
    return Tensor(torch.tensor(v, dtype=torch.int64), dtype)

  def floor(x, name=None):
    return wrap_like(torch.floor(_t(x)), x)

  def ones(shp, dtype=tf.float32, name=None):
    z = tf.zeros(shp, dtype)
    return Tensor(z.t + 1, dtype)

  def ones_like(x, dtype=None, name=None, optimize=True):
    dt = dtype if dtype is not None else x.dtype
    return ones(list(_t(x).shape), dt)

  def zeros_like(x, dtype=None, name=None, optimize=True):
    dt = dtype if dtype is not None else x.dtype
    return tf.zeros(list(_t(x).shape), dt)

  def not_equal(a, b, name=None):
    return Tensor(torch.ne(_t(a), _t(b)), tf.bool)

  def reduce_min(x, axis=None, keepdims=None, name=None, reduction_indices=None, keep_dims=None):
    return tf._reduce(torch.amin, x, axis if axis is not None else reduction_indices, keepdims, keep_dims)

  def where(condition, x=None, y=None, name=None):
    """[TF-sem] one argument: the coordinates of the true elements, [n, rank]; three: x where true else y, and a
    rank-1 condition over higher-rank x / y selects whole rows"""
    c = _t(condition)
    if x is None and y is None:
      return Tensor(torch.nonzero(c), tf.int64)
    tx, ty = _t(x), _t(y)
    if c.dim() == 1 and tx.dim() > 1:
      c = c.reshape([-1] + [1] * (tx.dim() - 1))
    if ty.dtype != tx.dtype:
      ty = ty.to(tx.dtype)
    return wrap_like(torch.where(c, tx, ty), x if isinstance(x, Tensor) else y)

  def gather(params, indices, name=None, axis=0):
    """[TF-sem] output shape = indices.shape + params.shape[1:]"""
    assert axis == 0
    return wrap_like(_t(params)[_t(indices).long()], params)

  def cumsum(x, axis=0, exclusive=False, reverse=False, name=None):
    assert not exclusive and not reverse
    return wrap_like(torch.cumsum(_t(x), dim=axis), x)

  def histogram_fixed_width(values, value_range, nbins=100, dtype=tf.int32, name=None):
    """[TF-sem, 1.14 histogram_ops.py]: scaled = (values - lo) / (hi - lo) (true division), index = floor(nbins * scaled)
    clipped to [0, nbins - 1], counted.  For integers 0..255, range [0, 255], 256 bins: bin = value."""
    v = np_of(values).astype(np.float64).reshape(-1)
    lo, hi = float(value_range[0]), float(value_range[1])
    idx = np.clip(np.floor(nbins * ((v - lo) / (hi - lo))), 0, nbins - 1).astype(np.int64)
    return Tensor(torch.from_numpy(np.bincount(idx, minlength=nbins).astype(np.int64)), tf.int32)

  class _Bitwise(object):
    """[TF-sem] element-wise shifts on the integer type; a shift by the full width (8 on uint8) is implementation-defined
    in TensorFlow: this project defines right_shift by >= 8 as 0"""
    @staticmethod
    def right_shift(x, y, name=None):
      y = int(_t(y))
      v = np_of(x).astype(np.int64)
      return wrap_like(torch.from_numpy((v >> y if y < 8 else v * 0).astype(np.uint8)), x)

    @staticmethod
    def left_shift(x, y, name=None):
      y = int(_t(y))
      v = np_of(x).astype(np.int64)
      return wrap_like(torch.from_numpy(((v << y) & 255).astype(np.uint8)), x)

  def rgb_to_grayscale(images, name=None):
    """[TF-sem, 1.14 image_ops_impl.py]: convert_image_dtype(uint8 -> float32) multiplies by 1 / 255; the weighted sum
    with [0.2989, 0.5870, 0.1140] runs over the channel axis in order; convert_image_dtype(float32 -> uint8) multiplies
    by 255.5 and casts (truncation).  Keeps the channel axis (size 1)."""
    v = np_of(images)
    assert v.dtype == np.uint8
    f = v.astype(F) * F(1.0 / 255.0)
    w = np.array([0.2989, 0.5870, 0.1140], dtype=F)
    s = np.zeros(v.shape[:-1], dtype=F)
    for c in range(3):
      s = (s + (f[..., c] * w[c]).astype(F)).astype(F)
    g = (s * F(255.5)).astype(F)
    return Tensor(torch.from_numpy(g.astype(np.int32).astype(np.uint8)[..., None]), tf.uint8)

  def grayscale_to_rgb(images, name=None):
    return wrap_like(_t(images).repeat(*([1] * (_t(images).dim() - 1) + [3])), images)

  def depthwise_conv2d(input, filter, strides, padding, rate=None, name=None, data_format=None):   # noqa: A002
    """[TF-sem] NHWC input, filter [kh, kw, C, multiplier], cross-correlation per channel, float32; the taps are
    accumulated in row-major order.  General in kernel size, stride and channel multiplier; VALID padding."""
    assert padding == 'VALID' and (rate is None or list(rate) == [1, 1])
    x, w = np_of(input).astype(F), np_of(filter).astype(F)
    n, H, W, C = x.shape
    kh, kw, fc, mult = w.shape
    assert fc == C
    sh, sw = int(strides[1]), int(strides[2])
    oh, ow = (H - kh) // sh + 1, (W - kw) // sw + 1
    out = np.zeros((n, max(oh, 0), max(ow, 0), C * mult), dtype=F)
    for i in range(kh):
      for j in range(kw):
        patch = x[:, i:i + (oh - 1) * sh + 1:sh, j:j + (ow - 1) * sw + 1:sw, :]
        for m in range(mult):
          out[..., m::mult] = (out[..., m::mult] + (patch * w[i, j, :, m]).astype(F)).astype(F)
    return Tensor(torch.from_numpy(out), tf.float32)

  def transform(images, transforms, interpolation='NEAREST', name=None):
    """[TF-sem, tf.contrib.image.transform, kernels/image_ops.h]: output pixel (x, y) reads input
    ((a0 x + a1 y + a2) / k, (b0 x + b1 y + b2) / k), k = c0 x + c1 y + 1, in float32; NEAREST rounds each coordinate half
    away from zero (std::round); a read outside the image returns zero in every channel."""
    assert interpolation == 'NEAREST'
    img = np_of(images)
    t = np.array([float(_t(v)) for v in transforms] if isinstance(transforms, (list, tuple))
                 else np_of(transforms).reshape(-1), dtype=F)
    assert img.ndim == 3 and t.shape == (8,)
    H, W = img.shape[:2]
    x = np.arange(W, dtype=F)[None, :]
    y = np.arange(H, dtype=F)[:, None]
    k = ((t[6] * x).astype(F) + (t[7] * y).astype(F)).astype(F) + F(1)
    sx = ((((t[0] * x).astype(F) + (t[1] * y).astype(F)).astype(F) + t[2]).astype(F) / k).astype(F)
    sy = ((((t[3] * x).astype(F) + (t[4] * y).astype(F)).astype(F) + t[5]).astype(F) / k).astype(F)

    def rnd(v):
      v = v.astype(np.float64)
      return np.sign(v) * np.floor(np.abs(v) + 0.5)
    rx, ry = rnd(sx), rnd(sy)
    ok = (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
    out = np.zeros_like(img)
    out[ok] = img[ry[ok].astype(np.int64), rx[ok].astype(np.int64)]
    return wrap_like(torch.from_numpy(out), images)

  def rotate(images, angles, interpolation='NEAREST', name=None):
    """[TF-sem, angles_to_projective_transforms]: rotation by `angles` about ((W - 1) / 2, (H - 1) / 2), float32;
    cosine and sine taken in double and rounded to float32"""
    H, W = [int(s) for s in _t(images).shape[:2]]
    a = F(float(_t(angles)))
    c, s = F(math.cos(float(a))), F(math.sin(float(a)))
    w1, h1 = F(W - 1), F(H - 1)
    x_off = (w1 - (c * w1 - s * h1)) / F(2)
    y_off = (h1 - (s * w1 + c * h1)) / F(2)
    return transform(images, [c, -s, x_off, s, c, y_off, F(0), F(0)], interpolation)

  def translate(images, translations, interpolation='NEAREST', name=None):
    """[TF-sem, translations_to_projective_transforms]: [1, 0, -dx, 0, 1, -dy, 0, 0]"""
    dx, dy = [F(float(_t(v))) for v in translations]
    return transform(images, [F(1), F(0), -dx, F(0), F(1), -dy, F(0), F(0)], interpolation)

  class HParams(object):
    def __init__(self, **kw):
      self.__dict__.update(kw)

  for name, fn in dict(constant=constant, cond=cond, random_uniform=random_uniform, floor=floor, ones=ones,
                       ones_like=ones_like, zeros_like=zeros_like, not_equal=not_equal, reduce_min=reduce_min, where=where,
                       gather=gather, cumsum=cumsum, histogram_fixed_width=histogram_fixed_width,
                       bitwise=_Bitwise).items():
    setattr(tf, name, fn)
  tf.image.rgb_to_grayscale = staticmethod(rgb_to_grayscale)
  tf.image.grayscale_to_rgb = staticmethod(grayscale_to_rgb)
  type(tf.image).rgb_to_grayscale = staticmethod(rgb_to_grayscale)
  type(tf.image).grayscale_to_rgb = staticmethod(grayscale_to_rgb)
  type(tf.nn).depthwise_conv2d = staticmethod(depthwise_conv2d)
  tf.contrib.image = tf._Namespace(rotate=rotate, translate=translate, transform=transform)
  tf.contrib.training = tf._Namespace(HParams=HParams)
  return state


# ---- what is recorded ------------------------------------------------------------------------------------------------
LEVELS_BIG, LEVELS_SMALL = (0, 3, 7, 10), (5, 10)
E2E_RUNS = [   # (policy, first op, second op, every slot fires?, seed)
    ('imagenet', 'Posterize', 'Rotate', True, 1), ('imagenet', 'Color', 'Contrast', True, 2),
    ('imagenet', 'Sharpness', 'Invert', True, 3), ('imagenet', 'ShearX', 'Equalize', True, 4),
    ('good', 'Cutout', 'Equalize', True, 5), ('good', 'TranslateY', 'Cutout', True, 6),
    ('good', 'AutoContrast', 'Brightness', True, 7), ('v0', 'Equalize', 'SolarizeAdd', True, 8),
    ('test', 'TranslateX', 'Equalize', True, 9), ('imagenet', None, None, False, 10), ('good', None, None, False, 11),
    ('v0', None, None, False, 12)]


def images():
  rng = np.random.default_rng(51)
  return {'rand24x40': rng.integers(0, 256, size=(24, 40, 3), dtype=np.uint8),
          'rand17x17': rng.integers(0, 256, size=(17, 17, 3), dtype=np.uint8),
          'const9x9': np.full((9, 9, 3), 93, dtype=np.uint8)}


def plain(v):
  return int(v) if isinstance(v, (int, np.integer)) else float(v)


def generate():
  T.install_import_hooks()
  import tensorflow as tf
  assert 'tf_shim' in tf.__file__, tf.__file__
  tf.set_compute_dtype(torch.float32)
  state = attach_stand_ins(tf)
  from preprocessing import autoaugment as A
  hp = tf.contrib.training.HParams(cutout_max_pad_fraction=0.75, cutout_const=100, translate_const=250)
  replace = [128, 128, 128]
  arrays, meta = {}, {'_generator': 'tests/golden/make_reference_autoaugment.py', '_reference': T.REF}

  def script(values):
    state['script'], state['pos'], state['log'] = list(values), 0, []

  tables = {'imagenet': A.imagenet_policies, 'good': A.good_policies, 'v0': A.policy_v0, 'test': A.policy_vtest}
  meta['policies'] = {k: [[[n, float(p), int(lv)] for (n, p, lv) in sub] for sub in fn()] for k, fn in tables.items()}
  meta['op_names'] = list(A.NAME_TO_FUNC.keys())

  # level_to_arg: every name, levels 0..10, the sign draw forced each way (u = 0.75 keeps the sign, u = 0.25 negates)
  meta['level_to_arg'] = []
  for name in A.NAME_TO_FUNC:
    for level in range(11):
      for u in (0.75, 0.25):
        script([u])
        args = A.level_to_arg(hp)[name](level)
        meta['level_to_arg'].append(dict(name=name, level=level, u=u, draws=state['pos'], args=[plain(a) for a in args]))

  # every op function on small images
  meta['ops'] = []
  imgs = images()
  for key, img in imgs.items():
    arrays['image/' + key] = img
    for name in A.NAME_TO_FUNC:
      for level in (LEVELS_BIG if key == 'rand24x40' else LEVELS_SMALL):
        if name == 'Solarize' and level == 10:
          level = 9            # threshold 256 does not exist in uint8: no TensorFlow result to record
        for u in ((0.75, 0.25) if name in ('Rotate', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY') else (0.75,)):
          centre_u = [((level * 37 + 11) % 100) / 100.0, ((level * 53 + 29) % 100) / 100.0]
          script([u] + centre_u)
          func, _, args = A._parse_policy_info(name, 1.0, level, replace, hp)
          n_sign = state['pos']
          out = func(tf.constant(img, tf.uint8), *args)
          k = 'op/%s/%s/%d/%s' % (key, name, level, 'neg' if u < 0.5 else 'pos')
          arrays[k] = out.numpy().astype(np.uint8)
          rec = dict(image=key, name=name, level=level, out=k,
                     args=[plain(a) for a in args if not isinstance(a, list)])
          if name == 'Cutout':
            rec['args'] += [int(v) for v in state['log'][n_sign:]]      # the centre drawn: row, column
          meta['ops'].append(rec)

  # distort_image_with_autoaugment end to end, tf.random_uniform replaying a stored list
  meta['runs'] = []
  img = imgs['rand24x40']
  for r, (pol, first, second, fire, seed) in enumerate(E2E_RUNS):
    table = meta['policies'][pol]
    rng = np.random.default_rng(seed)
    n_signed = sum(n in ('Rotate', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY') for sub in table for (n, _, _) in sub)
    values = [round(float(v), 6) for v in rng.random(n_signed + 8)]
    if first is not None:
      want = [i for i, sub in enumerate(table) if sub[0][0] == first and sub[1][0] == second][0]
      values[n_signed] = (want + 0.5) / len(table)
    if fire:     # 0.97 + prob >= 1 for every probability the tables hold but 0.0; also the cutout centre draws
      values[n_signed + 1:] = [0.97] * (len(values) - n_signed - 1)
    script(values)
    out = A.distort_image_with_autoaugment(tf.constant(img, tf.uint8), pol)
    used = state['pos']
    k = 'run/%d' % r
    arrays[k] = out.numpy().astype(np.uint8)
    # the draws after the signs: sub-policy index, then per slot the "apply" draw (and a fired cutout's centre)
    log = state['log']
    selected = int(log[n_signed])
    fired, pos = [], n_signed + 1
    for (n, p, lv) in table[selected]:
      f = bool(math.floor(F(log[pos]) + F(p)) >= 1)
      pos += 1
      if f and n == 'Cutout':
        pos += 2
      fired.append(f)
    assert pos == used, (pos, used)
    meta['runs'].append(dict(policy=pol, image='rand24x40', script=values[:used], selected=selected, fired=fired, out=k))
  with pytest_raises(ValueError):
    A.distort_image_with_autoaugment(tf.constant(img, tf.uint8), 'nope')
  return arrays, meta


class pytest_raises(object):
  def __init__(self, exc):
    self.exc = exc

  def __enter__(self):
    return self

  def __exit__(self, tp, val, tb):
    assert tp is not None and issubclass(tp, self.exc), 'expected %s' % self.exc
    return True


def main():
  arrays, meta = generate()
  if '--check' in sys.argv:
    old = np.load(OUT_NPZ)
    assert sorted(old.files) == sorted(arrays), 'regenerated fixture has other arrays than the committed file'
    for k in arrays:
      assert np.array_equal(old[k], arrays[k]), k
    assert json.dumps(meta, sort_keys=True) == json.dumps(json.load(open(OUT_JSON)), sort_keys=True), \
        'regenerated fixture differs from the committed file'
    print('fixture reproduces')
    return
  np.savez_compressed(OUT_NPZ, **arrays)
  json.dump(meta, open(OUT_JSON, 'w'), sort_keys=True)
  print('wrote', OUT_NPZ, os.path.getsize(OUT_NPZ), 'bytes;', OUT_JSON, os.path.getsize(OUT_JSON), 'bytes;',
        len(meta['ops']), 'op outputs,', len(meta['runs']), 'runs')


if __name__ == '__main__':
  main()
