#!/usr/bin/env python
"""Generate tests/golden/reference_preprocessing.{npz,json} by RUNNING the reference's preprocessing/reid_preprocessing.py
and preprocessing/inception_preprocessing.py, unmodified, under the torch-backed `tensorflow` stand-in (oracle/tf_shim) with
the float32 compute dtype:

  reid_preprocessing.preprocess_image, training: selector 0 (resize to 256 x 256, crop) and 1 (resize to the output), the
    flip after them, the mean subtraction; evaluation with and without eval_large_resolution                    :489-540
  inception_preprocessing.preprocess_image, evaluation (convert_image_dtype, central_crop, resize_bilinear) and training
    (sampled box, resize, flip, distort_color_fast), at a non-square output and at 331                          :117-368

The shim lacks the calls only these modules use; this generator attaches its own stand-ins to the imported shim module, in
process (oracle/ stays as it is).  Each restates the TensorFlow 1.14 rule in general form, marked [TF-sem] (DESIGN.md
section 1.4); none is derived from tests/preprocess_ref.py or from the product.  TensorFlow's random stream cannot be
reproduced: the selector, the crop offsets, the flips, the boxes and the colour draws are the stand-ins' own, replayed from a
scripted list and recorded in the fixture.

Run in the build container (needs the reference checkout); tests only read the committed fixture.
usage: python tests/golden/make_reference_preprocessing.py [--check]
"""
import json
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_taps as T  # noqa: E402  (import hooks)
from name_seeded import tap_summary  # noqa: E402

OUT_NPZ = os.path.join(HERE, 'reference_preprocessing.npz')
OUT_JSON = os.path.join(HERE, 'reference_preprocessing.json')
F = np.float32
WHOLE_BYTES = 16 * 1024      # outputs up to this size are stored whole, larger ones as tap_summary digests
SHAPES = {'75x100': (75, 100), '100x67': (100, 67), '49x49': (49, 49), '2x3': (2, 3), '1x1': (1, 1)}


# ---- stand-ins attached to the shim module ------------------------------------------------------------------------
def attach_stand_ins(tf):
  """-> state: `script` is the list of uniform draws u in [0, 1) the stand-ins replay in call order, `boxes` the crop
  boxes sample_distorted_bounding_box hands out, `log` what each draw became"""
  Tensor, _t = tf.Tensor, tf._t
  state = dict(script=[], pos=0, boxes=[], log=[], branches=[], dead=False)

  def next_u():
    u = state['script'][state['pos']]
    state['pos'] += 1
    return u

  def random_uniform(shape, minval=0, maxval=None, dtype=tf.float32, seed=None, name=None):   # noqa: A002
    """[TF-sem] a scalar uniform draw in [minval, maxval): u -> minval + u * (maxval - minval), float32 for a floating
    dtype, floored for an integer one.  An op on the untaken side of a switch does not run: it draws nothing."""
    assert list(shape) == [], 'only scalar draws are scripted'
    lo = float(_t(minval))
    hi = 1.0 if maxval is None else float(_t(maxval))
    if state['dead']:
      return Tensor(torch.tensor(lo if dtype.is_floating else int(lo)), dtype)
    u = next_u()
    if dtype.is_floating:
      v = F(lo + u * (hi - lo))
      state['log'].append(('uniform', float(v)))
      return Tensor(torch.tensor(float(v), dtype=torch.float32), dtype)
    v = int(math.floor(lo + u * (hi - lo)))
    state['log'].append(('uniform_int', v))
    return Tensor(torch.tensor(v, dtype=torch.int64), dtype)

  class _FlipDraws(object):
    """what the shim's random_flip_left_right draws from (shim_state().rng): the next scripted u; u < 0.5 flips"""
    @staticmethod
    def random():
      return next_u()

  def switch(data, pred, dtype=None, name=None):
    """[TF-sem] control_flow_ops.switch -> (output_false, output_true): `data` goes to the output `pred` selects and the
    other one is dead: nothing that consumes it runs.  Python executes the reference's branches one after the other, so the
    stand-in notes whether the branch that follows is the dead one (its draws are skipped, its value never merged)."""
    live = bool(_t(pred).item())
    state['branches'].append(live)
    state['dead'] = not live
    return data, data

  def merge(inputs, name=None):
    """[TF-sem] control_flow_ops.merge -> (the one input that is not dead, its index)"""
    live = state['branches'][-len(inputs):]
    assert sum(live) == 1, 'merge needs exactly one live input'
    del state['branches'][-len(inputs):]
    state['dead'] = False
    k = live.index(True)
    return inputs[k], Tensor(torch.tensor(k, dtype=torch.int64), tf.int32)

  def with_dependencies(dependencies, output_tensor, name=None):
    """[TF-sem] the output tensor, evaluated after the dependencies (assertions, inert under the shim)"""
    return output_tensor

  def convert_image_dtype(image, dtype, saturate=False, name=None):
    """[TF-sem, 1.14 image_ops_impl.py] integer -> float: cast, then multiply by scale = 1.0 / image.dtype.max, a Python
    double that becomes a constant of the float dtype; a float input of the same dtype is returned as it is"""
    t = _t(image)
    if t.dtype.is_floating_point:
      return image
    assert t.dtype == torch.uint8 and dtype == tf.float32
    scale = 1.0 / 255
    return Tensor(torch.from_numpy(t.numpy().astype(F) * F(scale)), tf.float32)

  def central_crop(image, central_fraction):
    """[TF-sem, 1.14 image_ops_impl.py] for [H, W, C]: start = int((size - size * central_fraction) / 2) in Python doubles,
    extent = size - 2 * start, per axis; a slice"""
    t = _t(image)
    assert t.dim() == 3 and 0.0 < central_fraction <= 1.0
    if central_fraction == 1.0:
      return image
    H, W = int(t.shape[0]), int(t.shape[1])
    y, x = int((H - H * central_fraction) / 2), int((W - W * central_fraction) / 2)
    return Tensor(t[y:y + (H - 2 * y), x:x + (W - 2 * x)], getattr(image, 'dtype', None))

  def resize_bilinear(images, size, align_corners=False, name=None):
    """[TF-sem] the kernel behind tf.image.resize_images(BILINEAR) on a [N, H, W, C] batch: the shim's own legacy resize"""
    t = _t(images)
    assert t.dim() == 4
    oh, ow = [int(_t(v)) for v in size]
    return Tensor(torch.stack([tf._resize_bilinear_legacy(e, oh, ow, align_corners) for e in t], 0), tf.float32)

  def sample_distorted_bounding_box(image_size, bounding_boxes, min_object_covered=0.1, aspect_ratio_range=None,
                                    area_range=None, max_attempts=None, use_image_if_no_bounding_boxes=None, **_):
    """hands out the next box of state['boxes'] (y, x, h, w) and checks what the caller constrains it with"""
    H, W = [int(v) for v in _t(image_size).reshape(-1).tolist()[:2]]
    assert tuple(aspect_ratio_range) == (3. / 4., 4. / 3.) and tuple(area_range) == (0.1, 1.0) and max_attempts == 100
    assert float(min_object_covered) == 0.1 and use_image_if_no_bounding_boxes
    y, x, h, w = state['boxes'].pop(0)
    assert 0 <= y and 0 <= x and h > 0 and w > 0 and y + h <= H and x + w <= W
    state['log'].append(('box', y, x, h, w))
    begin = Tensor(torch.tensor([y, x, 0], dtype=torch.int64), tf.int32)
    size = Tensor(torch.tensor([h, w, -1], dtype=torch.int64), tf.int32)
    return begin, size, None

  def greater_equal(a, b, name=None):
    return Tensor(torch.ge(_t(a), _t(b)), tf.bool)

  tf.random_uniform = random_uniform
  tf.greater_equal = greater_equal
  image_cls = type(tf.image)
  image_cls.convert_image_dtype = staticmethod(convert_image_dtype)
  image_cls.central_crop = staticmethod(central_crop)
  image_cls.resize_bilinear = staticmethod(resize_bilinear)
  image_cls.sample_distorted_bounding_box = staticmethod(sample_distorted_bounding_box)
  from tensorflow.python.ops import control_flow_ops
  control_flow_ops.switch, control_flow_ops.merge = switch, merge
  control_flow_ops.with_dependencies = with_dependencies
  # modules the shim does not have: random_ops, and absl.flags with the three flags inception_preprocessing.py defines
  random_ops = types.ModuleType('tensorflow.python.ops.random_ops')
  random_ops.random_uniform = random_uniform
  sys.modules['tensorflow.python.ops.random_ops'] = random_ops
  sys.modules['tensorflow.python.ops'].random_ops = random_ops

  class _Flags(object):
    pass
  values = _Flags()

  def define(name, default, help=None, **_):   # noqa: A002
    setattr(values, name, default)
  flags = types.ModuleType('absl.flags')
  flags.FLAGS = values
  flags.DEFINE_float = flags.DEFINE_boolean = flags.DEFINE_integer = flags.DEFINE_string = define
  absl = types.ModuleType('absl')
  absl.flags = flags
  absl.__path__ = []
  sys.modules['absl'], sys.modules['absl.flags'] = absl, flags
  state['flip_draws'] = _FlipDraws
  state['flags'] = values
  return state


# ---- what is recorded ------------------------------------------------------------------------------------------------
def images():
  return {k: np.random.default_rng(200 + i).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
          for i, (k, (h, w)) in enumerate(SHAPES.items())}


def u_int(v, n):
  """a u that random_uniform([], maxval=n, int32) floors to v"""
  return (v + 0.5) / n


REID_TRAIN = [   # (image, S, selector, offset or None, flip)
    ('75x100', 32, 0, (0, 0), 0), ('75x100', 32, 0, (0, 0), 1), ('100x67', 32, 0, (224, 224), 0),
    ('100x67', 32, 0, (224, 224), 1), ('49x49', 32, 0, (57, 130), 0), ('2x3', 32, 0, (57, 130), 1),
    ('1x1', 32, 0, (3, 200), 1), ('100x67', 256, 0, (0, 0), 0), ('49x49', 256, 0, (0, 0), 1),
    ('75x100', 32, 1, None, 0), ('75x100', 32, 1, None, 1), ('2x3', 32, 1, None, 1), ('1x1', 32, 1, None, 0),
    ('49x49', 32, 1, None, 1)]
REID_EVAL = [('75x100', 32, True), ('100x67', 32, False), ('2x3', 32, True), ('1x1', 32, False), ('49x49', 28, True)]
INCEPTION_EVAL = [('75x100', 24, 40), ('100x67', 24, 40), ('49x49', 24, 40), ('2x3', 24, 40), ('1x1', 24, 40),
                  ('100x67', 331, 331)]
INCEPTION_TRAIN = [   # (image, out_h, out_w, box (y, x, h, w), flip, (u_br, u_cb, u_cr))
    ('75x100', 24, 40, (10, 20, 50, 61), 0, (0.93, 0.12, 0.71)), ('75x100', 24, 40, (10, 20, 50, 61), 1, (0.93, 0.12, 0.71)),
    ('100x67', 24, 40, (0, 0, 100, 67), 1, (0.02, 0.99, 0.01)), ('49x49', 24, 40, (17, 3, 31, 29), 0, (0.999, 0.5, 0.98)),
    ('2x3', 24, 40, (0, 1, 2, 2), 1, (0.4, 0.6, 0.3)), ('1x1', 24, 40, (0, 0, 1, 1), 1, (0.0, 0.0, 0.999)),
    ('75x100', 331, 331, (5, 7, 64, 83), 1, (0.25, 0.8, 0.35))]


def generate():
  T.install_import_hooks()
  import tensorflow as tf
  assert 'tf_shim' in tf.__file__, tf.__file__
  tf.set_compute_dtype(torch.float32)
  state = attach_stand_ins(tf)
  from preprocessing import inception_preprocessing as I
  from preprocessing import reid_preprocessing as R
  tf.reset_default_graph()
  st = tf.shim_state()
  st.rng = state['flip_draws']
  arrays, meta = {}, {'_generator': 'tests/golden/make_reference_preprocessing.py', '_reference': T.REF}
  imgs = images()
  for k, im in imgs.items():
    arrays['image/' + k] = im
  meta['channel_means'] = list(R._CHANNEL_MEANS)
  meta['reid_resize'] = int(R._RESIZE_MIN)
  meta['flags'] = {k: getattr(state['flags'], k) for k in ('cb_distortion_range', 'cr_distortion_range',
                                                           'use_fast_color_distort')}

  def script(values, boxes=()):
    state['script'], state['pos'], state['log'], state['boxes'] = list(values), 0, [], list(boxes)
    st.window_draws = []

  def record(rec, key, out):
    out = out.numpy()
    assert out.dtype == np.float32
    if out.nbytes <= WHOLE_BYTES:
      arrays[key] = out
      rec['out'] = key
    else:
      rec['digest'] = tap_summary(out, 96)
    rec['shape'] = list(out.shape)
    return rec

  meta['reid_train'] = []
  for n, (name, S, sel, off, flip) in enumerate(REID_TRAIN):
    values = [u_int(sel, 2)]
    if sel == 0:
      values += [u_int(off[0], R._RESIZE_MIN - S + 1), u_int(off[1], R._RESIZE_MIN - S + 1)]
    values.append(0.25 if flip else 0.75)
    script(values)
    out = R.preprocess_image(tf.constant(imgs[name]), S, S, 3, is_training=True)
    assert state['pos'] == len(values), 'the reference drew %d values, %d were scripted' % (state['pos'], len(values))
    ints = [d[1] for d in state['log'] if d[0] == 'uniform_int']
    flips = [d[1] for d in st.window_draws if d[0] == 'flip']
    assert ints[0] == sel and flips == [flip] and (sel == 1 or tuple(ints[1:]) == tuple(off))
    meta['reid_train'].append(record(dict(image=name, size=S, selector=ints[0], offset=ints[1:] if sel == 0 else None,
                                          flip=flips[0]), 'reid_train/%d' % n, out))

  meta['reid_eval'] = []
  for n, (name, S, large) in enumerate(REID_EVAL):
    script([])
    out = R.preprocess_image(tf.constant(imgs[name]), S, S, 3, is_training=False, eval_large_resolution=large)
    meta['reid_eval'].append(record(dict(image=name, size=S, large=large), 'reid_eval/%d' % n, out))

  meta['inception_eval'] = []
  for n, (name, oh, ow) in enumerate(INCEPTION_EVAL):
    script([])
    out = I.preprocess_image(tf.constant(imgs[name]), oh, ow, is_training=False)
    meta['inception_eval'].append(record(dict(image=name, out_h=oh, out_w=ow), 'inception_eval/%d' % n, out))

  meta['inception_train'] = []
  for n, (name, oh, ow, box, flip, us) in enumerate(INCEPTION_TRAIN):
    values = [0.5, 0.25 if flip else 0.75] + list(us)      # the one-case resize selector, the flip, br / cb / cr
    script(values, [box])
    out = I.preprocess_image(tf.constant(imgs[name]), oh, ow, is_training=True)
    assert state['pos'] == len(values) and not state['boxes']
    color = [d[1] for d in state['log'] if d[0] == 'uniform']
    flips = [d[1] for d in st.window_draws if d[0] == 'flip']
    boxes = [list(d[1:]) for d in state['log'] if d[0] == 'box']
    assert len(color) == 3 and flips == [flip] and boxes == [list(box)]
    meta['inception_train'].append(record(dict(image=name, out_h=oh, out_w=ow, box=boxes[0], flip=flips[0], color=color),
                                          'inception_train/%d' % n, out))
  return arrays, meta


def main():
  arrays, meta = generate()
  if '--check' in sys.argv:
    old = np.load(OUT_NPZ)
    assert sorted(old.files) == sorted(arrays), 'regenerated fixture has other arrays than the committed file'
    for k in arrays:
      assert old[k].dtype == arrays[k].dtype and np.array_equal(old[k], arrays[k]), k
    assert json.dumps(meta, sort_keys=True) == json.dumps(json.load(open(OUT_JSON)), sort_keys=True), \
        'regenerated fixture differs from the committed file'
    print('fixture reproduces')
    return
  np.savez_compressed(OUT_NPZ, **arrays)
  json.dump(meta, open(OUT_JSON, 'w'), sort_keys=True)
  print('wrote', OUT_NPZ, os.path.getsize(OUT_NPZ), 'bytes;', OUT_JSON, os.path.getsize(OUT_JSON), 'bytes;',
        sum(len(meta[k]) for k in ('reid_train', 'reid_eval', 'inception_eval', 'inception_train')), 'cases')


if __name__ == '__main__':
  main()
