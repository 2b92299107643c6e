"""Host side of AutoAugment (preprocessing/autoaugment.py): the policy tables, the level -> argument rules, the random
draws and the affine matrices, resolved into one ``struct asm_augment_desc`` per image for ``ops.autoaugment``.

The device applies a descriptor; everything random or transcendental happens here, in float32 where the reference's
graph computes in float32.  Nothing in this module touches the library (pure numpy), so it is tested without a GPU.
TensorFlow's random stream cannot be reproduced: ``sample`` reproduces the distribution (uniform sub-policy, a slot
fires as floor(u + prob), signs flip with probability one half, the cutout centre is uniform over the image).
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

from . import lib

_MAX_LEVEL = 10.          # autoaugment.py:28
CUTOUT_CONST = 100        # autoaugment.py:899-901 (augmentation_hparams)
TRANSLATE_CONST = 250
REPLACE_VALUE = 128       # autoaugment.py:836

# NAME_TO_FUNC (autoaugment.py:682-699) in order: op id = index + 1; 0 = slot not applied
OP_NAMES = ('AutoContrast', 'Equalize', 'Invert', 'Rotate', 'Posterize', 'Solarize', 'SolarizeAdd', 'Color', 'Contrast',
            'Brightness', 'Sharpness', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'Cutout')
OP_IDS = {name: i + 1 for i, name in enumerate(OP_NAMES)}
SIGNED = ('Rotate', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY')      # _randomly_negate_tensor (:702-706)
_BLEND = ('Color', 'Contrast', 'Brightness', 'Sharpness')

OP_DTYPE = np.dtype(lib.AugmentOp)           # struct asm_augment_op
DESC_DTYPE = np.dtype(lib.AugmentDesc)       # struct asm_augment_desc


def _p(*rows):
  return [[(a, pa, la), (b, pb, lb)] for (a, pa, la, b, pb, lb) in rows]


# The tables of imagenet_policies (:70-106), good_policies (:148-267), policy_v0 (:270-302) and policy_vtest (:305-313):
# (op, probability, level) x 2 per sub-policy.  Pinned against the reference by tests/golden/reference_autoaugment.json.
POLICIES = {
    'imagenet': _p(
        ('Posterize', 0.4, 8, 'Rotate', 0.6, 9), ('Solarize', 0.6, 5, 'AutoContrast', 0.6, 5),
        ('Equalize', 0.8, 8, 'Equalize', 0.6, 3), ('Posterize', 0.6, 7, 'Posterize', 0.6, 6),
        ('Equalize', 0.4, 7, 'Solarize', 0.2, 4),
        ('Equalize', 0.4, 4, 'Rotate', 0.8, 8), ('Solarize', 0.6, 3, 'Equalize', 0.6, 7),
        ('Posterize', 0.8, 5, 'Equalize', 1.0, 2), ('Rotate', 0.2, 3, 'Solarize', 0.6, 8),
        ('Equalize', 0.6, 8, 'Posterize', 0.4, 6),
        ('Rotate', 0.8, 8, 'Color', 0.4, 0), ('Rotate', 0.4, 9, 'Equalize', 0.6, 2),
        ('Equalize', 0.0, 7, 'Equalize', 0.8, 8), ('Invert', 0.6, 4, 'Equalize', 1.0, 8),
        ('Color', 0.6, 4, 'Contrast', 1.0, 8),
        ('Rotate', 0.8, 8, 'Color', 1.0, 2), ('Color', 0.8, 8, 'Solarize', 0.8, 7),
        ('Sharpness', 0.4, 7, 'Invert', 0.6, 8), ('ShearX', 0.6, 5, 'Equalize', 1.0, 9),
        ('Color', 0.4, 0, 'Equalize', 0.6, 3),
        ('Equalize', 0.4, 7, 'Solarize', 0.2, 4), ('Solarize', 0.6, 5, 'AutoContrast', 0.6, 5),
        ('Invert', 0.6, 4, 'Equalize', 1.0, 8), ('Color', 0.6, 4, 'Contrast', 1.0, 8),
        ('Equalize', 0.8, 8, 'Equalize', 0.6, 3)),
    'good': _p(
        # exp0_0 .. exp0_3
        ('Invert', 0.1, 7, 'Contrast', 0.2, 6), ('Rotate', 0.7, 2, 'TranslateX', 0.3, 9),
        ('Sharpness', 0.8, 1, 'Sharpness', 0.9, 3), ('ShearY', 0.5, 8, 'TranslateY', 0.7, 9),
        ('AutoContrast', 0.5, 8, 'Equalize', 0.9, 2),
        ('Solarize', 0.4, 5, 'AutoContrast', 0.9, 3), ('TranslateY', 0.9, 9, 'TranslateY', 0.7, 9),
        ('AutoContrast', 0.9, 2, 'Solarize', 0.8, 3), ('Equalize', 0.8, 8, 'Invert', 0.1, 3),
        ('TranslateY', 0.7, 9, 'AutoContrast', 0.9, 1),
        ('Solarize', 0.4, 5, 'AutoContrast', 0.0, 2), ('TranslateY', 0.7, 9, 'TranslateY', 0.7, 9),
        ('AutoContrast', 0.9, 0, 'Solarize', 0.4, 3), ('Equalize', 0.7, 5, 'Invert', 0.1, 3),
        ('TranslateY', 0.7, 9, 'TranslateY', 0.7, 9),
        ('Solarize', 0.4, 5, 'AutoContrast', 0.9, 1), ('TranslateY', 0.8, 9, 'TranslateY', 0.9, 9),
        ('AutoContrast', 0.8, 0, 'TranslateY', 0.7, 9), ('TranslateY', 0.2, 7, 'Color', 0.9, 6),
        ('Equalize', 0.7, 6, 'Color', 0.4, 9),
        # exp1_0 .. exp1_6
        ('ShearY', 0.2, 7, 'Posterize', 0.3, 7), ('Color', 0.4, 3, 'Brightness', 0.6, 7),
        ('Sharpness', 0.3, 9, 'Brightness', 0.7, 9), ('Equalize', 0.6, 5, 'Equalize', 0.5, 1),
        ('Contrast', 0.6, 7, 'Sharpness', 0.6, 5),
        ('Brightness', 0.3, 7, 'AutoContrast', 0.5, 8), ('AutoContrast', 0.9, 4, 'AutoContrast', 0.5, 6),
        ('Solarize', 0.3, 5, 'Equalize', 0.6, 5), ('TranslateY', 0.2, 4, 'Sharpness', 0.3, 3),
        ('Brightness', 0.0, 8, 'Color', 0.8, 8),
        ('Solarize', 0.2, 6, 'Color', 0.8, 6), ('Solarize', 0.2, 6, 'AutoContrast', 0.8, 1),
        ('Solarize', 0.4, 1, 'Equalize', 0.6, 5), ('Brightness', 0.0, 0, 'Solarize', 0.5, 2),
        ('AutoContrast', 0.9, 5, 'Brightness', 0.5, 3),
        ('Contrast', 0.7, 5, 'Brightness', 0.0, 2), ('Solarize', 0.2, 8, 'Solarize', 0.1, 5),
        ('Contrast', 0.5, 1, 'TranslateY', 0.2, 9), ('AutoContrast', 0.6, 5, 'TranslateY', 0.0, 9),
        ('AutoContrast', 0.9, 4, 'Equalize', 0.8, 4),
        ('Brightness', 0.0, 7, 'Equalize', 0.4, 7), ('Solarize', 0.2, 5, 'Equalize', 0.7, 5),
        ('Equalize', 0.6, 8, 'Color', 0.6, 2), ('Color', 0.3, 7, 'Color', 0.2, 4),
        ('AutoContrast', 0.5, 2, 'Solarize', 0.7, 2),
        ('AutoContrast', 0.2, 0, 'Equalize', 0.1, 0), ('ShearY', 0.6, 5, 'Equalize', 0.6, 5),
        ('Brightness', 0.9, 3, 'AutoContrast', 0.4, 1), ('Equalize', 0.8, 8, 'Equalize', 0.7, 7),
        ('Equalize', 0.7, 7, 'Solarize', 0.5, 0),
        ('Equalize', 0.8, 4, 'TranslateY', 0.8, 9), ('TranslateY', 0.8, 9, 'TranslateY', 0.6, 9),
        ('TranslateY', 0.9, 0, 'TranslateY', 0.5, 9), ('AutoContrast', 0.5, 3, 'Solarize', 0.3, 4),
        ('Solarize', 0.5, 3, 'Equalize', 0.4, 4),
        # exp2_0 .. exp2_7
        ('Color', 0.7, 7, 'TranslateX', 0.5, 8), ('Equalize', 0.3, 7, 'AutoContrast', 0.4, 8),
        ('TranslateY', 0.4, 3, 'Sharpness', 0.2, 6), ('Brightness', 0.9, 6, 'Color', 0.2, 8),
        ('Solarize', 0.5, 2, 'Invert', 0.0, 3),
        ('AutoContrast', 0.1, 5, 'Brightness', 0.0, 0), ('Cutout', 0.2, 4, 'Equalize', 0.1, 1),
        ('Equalize', 0.7, 7, 'AutoContrast', 0.6, 4), ('Color', 0.1, 8, 'ShearY', 0.2, 3),
        ('ShearY', 0.4, 2, 'Rotate', 0.7, 0),
        ('ShearY', 0.1, 3, 'AutoContrast', 0.9, 5), ('TranslateY', 0.3, 6, 'Cutout', 0.3, 3),
        ('Equalize', 0.5, 0, 'Solarize', 0.6, 6), ('AutoContrast', 0.3, 5, 'Rotate', 0.2, 7),
        ('Equalize', 0.8, 2, 'Invert', 0.4, 0),
        ('Equalize', 0.9, 5, 'Color', 0.7, 0), ('Equalize', 0.1, 1, 'ShearY', 0.1, 3),
        ('AutoContrast', 0.7, 3, 'Equalize', 0.7, 0), ('Brightness', 0.5, 1, 'Contrast', 0.1, 7),
        ('Contrast', 0.1, 4, 'Solarize', 0.6, 5),
        ('Solarize', 0.2, 3, 'ShearX', 0.0, 0), ('TranslateX', 0.3, 0, 'TranslateX', 0.6, 0),
        ('Equalize', 0.5, 9, 'TranslateY', 0.6, 7), ('ShearX', 0.1, 0, 'Sharpness', 0.5, 1),
        ('Equalize', 0.8, 6, 'Invert', 0.3, 6),
        ('AutoContrast', 0.3, 9, 'Cutout', 0.5, 3), ('ShearX', 0.4, 4, 'AutoContrast', 0.9, 2),
        ('ShearX', 0.0, 3, 'Posterize', 0.0, 3), ('Solarize', 0.4, 3, 'Color', 0.2, 4),
        ('Equalize', 0.1, 4, 'Equalize', 0.7, 6),
        ('Equalize', 0.3, 8, 'AutoContrast', 0.4, 3), ('Solarize', 0.6, 4, 'AutoContrast', 0.7, 6),
        ('AutoContrast', 0.2, 9, 'Brightness', 0.4, 8), ('Equalize', 0.1, 0, 'Equalize', 0.0, 6),
        ('Equalize', 0.8, 4, 'Equalize', 0.0, 4),
        ('Equalize', 0.5, 5, 'AutoContrast', 0.1, 2), ('Solarize', 0.5, 5, 'AutoContrast', 0.9, 5),
        ('AutoContrast', 0.6, 1, 'AutoContrast', 0.7, 8), ('Equalize', 0.2, 0, 'AutoContrast', 0.1, 2),
        ('Equalize', 0.6, 9, 'Equalize', 0.4, 4)),
    'v0': _p(
        ('Equalize', 0.8, 1, 'ShearY', 0.8, 4), ('Color', 0.4, 9, 'Equalize', 0.6, 3),
        ('Color', 0.4, 1, 'Rotate', 0.6, 8), ('Solarize', 0.8, 3, 'Equalize', 0.4, 7),
        ('Solarize', 0.4, 2, 'Solarize', 0.6, 2), ('Color', 0.2, 0, 'Equalize', 0.8, 8),
        ('Equalize', 0.4, 8, 'SolarizeAdd', 0.8, 3), ('ShearX', 0.2, 9, 'Rotate', 0.6, 8),
        ('Color', 0.6, 1, 'Equalize', 1.0, 2), ('Invert', 0.4, 9, 'Rotate', 0.6, 0),
        ('Equalize', 1.0, 9, 'ShearY', 0.6, 3), ('Color', 0.4, 7, 'Equalize', 0.6, 0),
        ('Posterize', 0.4, 6, 'AutoContrast', 0.4, 7), ('Solarize', 0.6, 8, 'Color', 0.6, 9),
        ('Solarize', 0.2, 4, 'Rotate', 0.8, 9), ('Rotate', 1.0, 7, 'TranslateY', 0.8, 9),
        ('ShearX', 0.0, 0, 'Solarize', 0.8, 4), ('ShearY', 0.8, 0, 'Color', 0.6, 4),
        ('Color', 1.0, 0, 'Rotate', 0.6, 2), ('Equalize', 0.8, 4, 'Equalize', 0.0, 8),
        ('Equalize', 1.0, 4, 'AutoContrast', 0.6, 2), ('ShearY', 0.4, 7, 'SolarizeAdd', 0.6, 7),
        ('Posterize', 0.8, 2, 'Solarize', 0.6, 10), ('Solarize', 0.6, 8, 'Equalize', 0.6, 1),
        ('Color', 0.8, 6, 'Rotate', 0.4, 5)),
    'test': _p(('TranslateX', 1.0, 4, 'Equalize', 1.0, 10)),
}


def check_policy_name(name):
  if name not in POLICIES:
    raise ValueError('Invalid augmentation_name: {}'.format(name))      # autoaugment.py:894-895


def _check_op_name(name):
  if name not in OP_IDS:
    raise ValueError('Invalid augmentation op: %r (one of %s)' % (name, ', '.join(OP_NAMES)))


def _f32(x):
  return np.float32(x)


def level_to_arg(name: str, level, negate: bool = False) -> tuple:
  """autoaugment.py:709-764 with cutout_const=100, translate_const=250: the arguments the op function receives for a
  magnitude `level` (0..10).  `negate` is the outcome of _randomly_negate_tensor for Rotate / Shear / Translate (ignored
  by the others); those three are float32 tensors in the reference and come back rounded to float32."""
  _check_op_name(name)
  if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 0 <= level <= _MAX_LEVEL:
    raise ValueError('level must be an integer in 0..10, got %r' % (level,))
  level = int(level)
  if name in ('AutoContrast', 'Equalize', 'Invert'):
    return ()
  if name == 'Posterize':
    return (int((level / _MAX_LEVEL) * 4),)
  if name == 'Solarize':
    return (int((level / _MAX_LEVEL) * 256),)
  if name == 'SolarizeAdd':
    return (int((level / _MAX_LEVEL) * 110),)
  if name in _BLEND:
    return ((level / _MAX_LEVEL) * 1.8 + 0.1,)
  if name == 'Cutout':
    return (int((level / _MAX_LEVEL) * CUTOUT_CONST),)
  if name == 'Rotate':
    v = (level / _MAX_LEVEL) * 30.
  elif name in ('ShearX', 'ShearY'):
    v = (level / _MAX_LEVEL) * 0.3
  else:
    v = (level / _MAX_LEVEL) * float(TRANSLATE_CONST)
  v = float(_f32(v))
  return (-v if negate else v,)


# ---- affine coefficients, float32 like the graph: output (x, y) reads input (f0 x + f1 y + f2, f3 x + f4 y + f5) --------
def rotate_matrix(degrees, height: int, width: int) -> np.ndarray:
  """rotate (:462-484) -> tf.contrib.image.rotate -> angles_to_projective_transforms: a rotation about
  ((W - 1) / 2, (H - 1) / 2).  Cosine and sine are taken in double and rounded to float32."""
  radians = _f32(degrees) * _f32(math.pi / 180.0)
  c, s = _f32(math.cos(float(radians))), _f32(math.sin(float(radians)))
  w1, h1, two = _f32(width - 1), _f32(height - 1), _f32(2.0)
  x_offset = (w1 - (c * w1 - s * h1)) / two
  y_offset = (h1 - (s * w1 + c * h1)) / two
  return np.array([c, -s, x_offset, s, c, y_offset], dtype=np.float32)


def affine_matrix(name: str, arg, height: int, width: int) -> np.ndarray:
  one, zero, v = _f32(1), _f32(0), _f32(arg)
  if name == 'Rotate':
    return rotate_matrix(arg, height, width)
  if name == 'ShearX':         # :499-507
    return np.array([one, v, zero, zero, one, zero], dtype=np.float32)
  if name == 'ShearY':         # :510-518
    return np.array([one, zero, zero, v, one, zero], dtype=np.float32)
  # translate_x / translate_y (:487-496) call translate with -pixels and translations_to_projective_transforms negates
  # again: output (x, y) reads input (x + pixels, y)
  if name == 'TranslateX':
    return np.array([one, zero, v, zero, one, zero], dtype=np.float32)
  if name == 'TranslateY':
    return np.array([one, zero, zero, zero, one, v], dtype=np.float32)
  raise ValueError('%s is not a geometric op' % name)


def _int_arg(name, what, v, lo, hi):
  if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
    raise ValueError('%s: %s must be an integer in %d..%d, got %r' % (name, what, lo, hi, v))
  return int(v)


def _fill_slot(slot, spec, height, width):
  """one (name, arg...) tuple (the arguments the reference's op function takes after the image, without `replace`)"""
  if spec is None:
    return
  name, args = spec[0], tuple(spec[1:])
  _check_op_name(name)
  slot['op'] = OP_IDS[name]
  want = {'AutoContrast': 0, 'Equalize': 0, 'Invert': 0, 'SolarizeAdd': (1, 2), 'Cutout': 3}.get(name, 1)
  if len(args) != want and not (isinstance(want, tuple) and len(args) in want):
    raise ValueError('%s takes %s argument(s), got %r' % (name, want, args))
  if name == 'Posterize':
    slot['a'] = 8 - _int_arg(name, 'bits', args[0], 0, 8)
  elif name == 'Solarize':
    slot['a'] = _int_arg(name, 'threshold', args[0], 0, 256)
  elif name == 'SolarizeAdd':
    slot['a'] = _int_arg(name, 'addition', args[0], -255, 255)
    slot['b'] = _int_arg(name, 'threshold', args[1] if len(args) > 1 else 128, 0, 256)
  elif name == 'Cutout':
    slot['a'] = _int_arg(name, 'pad_size', args[0], 0, 1 << 15)
    cy = _int_arg(name, 'centre row', args[1], 0, height - 1)
    cx = _int_arg(name, 'centre column', args[2], 0, width - 1)
    slot['b'] = (cy << 16) | cx
  elif name in _BLEND:
    f = _f32(args[0])
    if not np.isfinite(f) or f < 0:
      raise ValueError('%s: the blend factor must be finite and >= 0, got %r' % (name, args[0]))
    slot['f'][0] = f
  elif name in SIGNED:
    if not np.isfinite(_f32(args[0])):
      raise ValueError('%s: the argument must be finite, got %r' % (name, args[0]))
    slot['f'][:] = affine_matrix(name, args[0], height, width)


def _check_size(height, width):
  if not (0 < height <= 32767 and 0 < width <= 32767 and height * width < (1 << 24)):
    raise ValueError('image size %r x %r is out of range (sides <= 32767, area < 2^24)' % (height, width))


def descriptor(ops: Sequence[Optional[tuple]], height: int, width: int) -> np.ndarray:
  """One descriptor (structured array of shape (1,)) from an explicit list of at most two ``(name, arg...)`` tuples, applied
  in order; ``None`` leaves a slot unapplied.  The arguments are the reference op's own: ('Rotate', degrees),
  ('ShearX', level), ('TranslateX', pixels), ('Posterize', bits), ('Solarize', threshold), ('SolarizeAdd', addition[,
  threshold]), ('Color' | 'Contrast' | 'Brightness' | 'Sharpness', factor), ('Cutout', pad_size, centre_y, centre_x),
  ('AutoContrast',), ('Equalize',), ('Invert',)."""
  _check_size(height, width)
  if len(ops) > 2:
    raise ValueError('a descriptor holds at most two ops, got %d' % len(ops))
  d = np.zeros(1, dtype=DESC_DTYPE)
  for k, spec in enumerate(ops):
    _fill_slot(d['slot'][0, k], spec, height, width)
  return d


def sample(name: str, n: int, height: int, width: int, rng: np.random.Generator, return_index: bool = False):
  """n descriptors drawn as distort_image_with_autoaugment (:872-903) draws them: a uniform sub-policy
  (select_and_apply_random_policy, :807-817); every slot fires iff floor(u + prob) is 1 with u uniform in [0, 1) in
  float32 (_apply_func_with_prob, :797-799): 0.0 never, 1.0 always; the sign of Rotate / Shear / Translate is negative
  iff floor(u + 0.5) is 0 (:702-706); the cutout centre is uniform over the image (:382-388).  With `return_index` the
  sub-policy index drawn for every image comes back as well."""
  check_policy_name(name)
  _check_size(height, width)
  policy = POLICIES[name]
  d = np.zeros(n, dtype=DESC_DTYPE)
  index = rng.integers(0, len(policy), size=n)
  for i in range(n):
    sub = policy[int(index[i])]
    for k, (op, prob, level) in enumerate(sub):
      fires = np.floor(rng.random(dtype=np.float32) + _f32(prob)) >= 1
      negate = op in SIGNED and not np.floor(rng.random(dtype=np.float32) + _f32(0.5)) >= 1
      centre = (int(rng.integers(0, height)), int(rng.integers(0, width))) if op == 'Cutout' else ()
      if fires:
        _fill_slot(d['slot'][i, k], (op,) + level_to_arg(op, level, negate) + centre, height, width)
  return (d, index) if return_index else d


def validate(descs: np.ndarray, height: int, width: int):
  """What the kernel accepts; anything else raises ValueError here (the kernel would leave the image unchanged)."""
  _check_size(height, width)
  if not isinstance(descs, np.ndarray) or descs.dtype != DESC_DTYPE or descs.ndim != 1:
    raise ValueError('descriptors must be a 1-D array of autoaugment.DESC_DTYPE')
  slots = descs['slot'].reshape(-1)
  op, a, b, f = slots['op'], slots['a'], slots['b'], slots['f']

  def bad(mask, what):
    if mask.any():
      k = int(np.flatnonzero(mask)[0])
      raise ValueError('descriptor %d slot %d: %s (op %d, a %d, b %d)' % (k // 2, k % 2, what, op[k], a[k], b[k]))
  bad((op < 0) | (op > len(OP_NAMES)), 'unknown op id')
  bad((op == OP_IDS['Posterize']) & ((a < 0) | (a > 8)), 'posterize shift outside 0..8')
  bad((op == OP_IDS['Solarize']) & ((a < 0) | (a > 256)), 'solarize threshold outside 0..256')
  bad((op == OP_IDS['SolarizeAdd']) & ((a < -255) | (a > 255) | (b < 0) | (b > 256)), 'solarize-add arguments out of range')
  cut = op == OP_IDS['Cutout']
  bad(cut & ((a < 0) | (a > (1 << 15)) | (b < 0) | ((b >> 16) >= height) | ((b & 0xffff) >= width)),
      'cutout pad size or centre out of range')
  blend = np.isin(op, [OP_IDS[n] for n in _BLEND])
  bad(blend & ~(np.isfinite(f[:, 0]) & (f[:, 0] >= 0)), 'blend factor must be finite and >= 0')
  geo = np.isin(op, [OP_IDS[n] for n in SIGNED])
  bad(geo & ~np.isfinite(f).all(axis=1), 'affine coefficients must be finite')
