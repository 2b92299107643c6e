"""GPU tail of the input pipeline.

Mirrors ``utils/data_util.py:267-386 preprocess_image`` + ``preprocessing/imagenet_preprocessing.py:269-313`` from
the point where the reference holds a decoded uint8 image: window selection (random box / whole image), flip,
legacy bilinear resize, central crop and mean subtraction.  Record parsing stays on the host (out of scope); the
window arithmetic below is host integer/float32 math done exactly as the reference's graph does it, and the pixel work
is one HIP launch for the whole ragged batch (ops.resize_crop_flip).  An entry of the batch may also be the ENCODED file
(tf.image.decode_jpeg / decode_and_crop_jpeg, imagenet_preprocessing.py:81,92-93,296): those are decoded on the device
(jpeg.py, csrc/jpeg.hip) straight into the packed buffer the resize reads.

The output of ``preprocess_batch(..., subtract_mean=True)`` is what the reference's ``preprocess_image`` returns
before ``tf.cast(image, dtype)`` (float32, mean-subtracted, NHWC) and feeds ``Model.__call__`` directly; with
``subtract_mean=False`` it feeds ``Trainer.train_step`` (whose fused mixup kernel subtracts the means).

The flag's other values -- 'reid', 'reid_224' (``preprocessing/reid_preprocessing.py:489-540``) and 'inception_331',
'inception_600' (``preprocessing/inception_preprocessing.py:117-368``) -- are window functions of the same kind and one launch
of ops.preprocess_window, the same kernel body with the flip after the resize, the source scaled to [0, 1] and the colour
offset + clamp those modules need.
"""
from __future__ import annotations

import math
import re
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import autoaugment as _aa
from . import jpeg as _jpeg
from . import lib, ops, staging

_RESIZE_MIN = 256   # preprocessing/imagenet_preprocessing.py:54


def output_size_and_crop_type(preprocessing_type: str, is_training: bool, image_size: int = 224) -> Tuple[int, int]:
  """utils/data_util.py:275-343: (output side, crop_type) for the imagenet* preprocessing types."""
  if preprocessing_type == 'imagenet':
    return image_size, 0
  if preprocessing_type == 'imagenet_224_256':
    return (224 if is_training else 256), 0
  if preprocessing_type == 'imagenet_224_256a':
    return (224 if is_training else 256), 1
  if re.compile('imagenet_[0-9]{3}a').match(preprocessing_type):
    return int(preprocessing_type.split('_')[1][0:3]), 1
  if re.compile('imagenet_[0-9]{3}').match(preprocessing_type):
    return int(preprocessing_type.split('_')[1]), 0
  raise NotImplementedError('preprocessing_type %r (only the imagenet* family is on the hot path)' % preprocessing_type)


def smallest_size_at_least(height: int, width: int, resize_min) -> Tuple[int, int]:
  """preprocessing/imagenet_preprocessing.py:158-186, in float32 like the graph."""
  resize_min = np.float32(resize_min)
  h, w = np.float32(height), np.float32(width)
  scale_ratio = resize_min / np.minimum(h, w)
  return int(np.float32(h * scale_ratio)), int(np.float32(w * scale_ratio))


def eval_window(height: int, width: int, out_h: int, out_w: int, crop_type: int = 0):
  """Whole image -> aspect-preserving resize -> central crop (imagenet_preprocessing.py:303-310, :97-120)."""
  if crop_type == 1:
    resize_min = int(min(out_h, out_w) + 1)
  else:
    resize_min = int(min(out_h, out_w) * (1.0 / 0.875))
  rh, rw = smallest_size_at_least(height, width, resize_min)
  if rh < out_h or rw < out_w:
    raise ValueError('resized image %dx%d is smaller than the %dx%d crop' % (rh, rw, out_h, out_w))
  return dict(crop_y=0, crop_x=0, crop_h=height, crop_w=width, resize_h=rh, resize_w=rw,
              out_y=(rh - out_h) // 2, out_x=(rw - out_w) // 2, flip=0)


def sample_distorted_bounding_box(height: int, width: int, rng: np.random.Generator, min_object_covered=0.1,
                                  aspect_ratio_range=(0.75, 1.33), area_range=(0.05, 1.0), max_attempts=100):
  """tf.image.sample_distorted_bounding_box with no annotated box and use_image_if_no_bounding_boxes=True
  (imagenet_preprocessing.py:66-76).  TensorFlow 1.14's published algorithm (sample_distorted_bounding_box_op.cc,
  GenerateRandomCrop): draw an aspect ratio, derive the admissible height range from the area range, draw a height,
  width = round(height * ratio), fix up the area by one row, draw the offsets; accept the first attempt that
  covers at least min_object_covered of the (whole-image) box, else fall back to the whole image.  TF's own
  random stream cannot be reproduced; `rng` supplies the draws.  Returns (y, x, h, w)."""
  lo, hi = aspect_ratio_range
  min_area = area_range[0] * width * height
  max_area = area_range[1] * width * height
  eps = 1e-7
  for _ in range(max_attempts):
    ratio = float(rng.uniform(lo, hi))
    h = int(round(math.sqrt(min_area / ratio)))
    max_h = int(round(math.sqrt(max_area / ratio)))
    if int(round(max_h * ratio)) > width:
      max_h = int((width + 0.5 - eps) / ratio)
    max_h = min(max_h, height)
    h = min(h, max_h)
    if h < max_h:
      h += int(rng.integers(0, max_h - h + 1))
    w = int(round(h * ratio))
    area = w * h
    if area < min_area:
      h += 1
      w = int(round(h * ratio))
      area = w * h
    if area > max_area:
      h -= 1
      w = int(round(h * ratio))
      area = w * h
    if area < min_area or area > max_area or w > width or h > height or w <= 0 or h <= 0:
      continue
    y = int(rng.integers(0, height - h + 1)) if h < height else 0
    x = int(rng.integers(0, width - w + 1)) if w < width else 0
    if area >= min_object_covered * width * height:     # coverage of the whole-image box by the crop
      return y, x, h, w
  return 0, 0, height, width


def train_window(height: int, width: int, out_h: int, out_w: int, rng: np.random.Generator,
                 use_random_crop: bool = True):
  """_decode_crop_and_flip + _resize_image (imagenet_preprocessing.py:57-97, :283-287)."""
  y, x, h, w = sample_distorted_bounding_box(height, width, rng,
                                             min_object_covered=0.1 if use_random_crop else 1.0)
  flip = int(rng.random() < 0.5)     # tf.image.random_flip_left_right
  return dict(crop_y=y, crop_x=x, crop_h=h, crop_w=w, resize_h=out_h, resize_w=out_w, out_y=0, out_x=0, flip=flip)


# ---- the re-ID and Inception types (utils/data_util.py:346-378) ------------------------------------------------------
FLIP_NONE, FLIP_BEFORE, FLIP_AFTER = 0, 1, 2      # asm_image_desc.flip as asm_preprocess_window reads it
_REID_RESIZE = 256                                 # preprocessing/reid_preprocessing.py:57 _RESIZE_MIN
_INCEPTION_SIDE = {'inception_331': 331, 'inception_600': 600}
_F = np.float32


def preprocessing_family(preprocessing_type: str) -> str:
  """'reid' | 'inception' | 'imagenet': which module of the reference a preprocessing_type goes to.  Everything that is
  neither of the first two is left to output_size_and_crop_type, which raises NotImplementedError for an unknown type."""
  if preprocessing_type in ('reid', 'reid_224'):
    return 'reid'
  if preprocessing_type in _INCEPTION_SIDE:
    return 'inception'
  return 'imagenet'


def reid_output_side(preprocessing_type: str, is_training: bool, image_size: int) -> int:
  """reid_preprocessing.py:506-538: training gives image_size; evaluation gives int(image_size * (1.0 / 0.875)) for 'reid'
  (eval_large_resolution, Python doubles) and image_size for 'reid_224'"""
  if is_training or preprocessing_type == 'reid_224':
    return int(image_size)
  return int(image_size * (1.0 / 0.875))


def reid_eval_window(height: int, width: int, side: int):
  """reid_preprocessing.py:530-538: the whole image resized to side x side regardless of aspect; no crop, no flip"""
  return dict(crop_y=0, crop_x=0, crop_h=height, crop_w=width, resize_h=side, resize_w=side, out_y=0, out_x=0,
              flip=FLIP_NONE)


def reid_train_window(height: int, width: int, size: int, rng: Optional[np.random.Generator] = None,
                      selector: Optional[int] = None, offset: Optional[Tuple[int, int]] = None,
                      flip: Optional[int] = None):
  """apply_with_random_selector(resize_func) + random_flip_left_right (reid_preprocessing.py:489-516).
  selector 0: the whole image resized to 256 x 256, then a size x size crop at uniform offsets in [0, 256 - size];
  selector 1: the whole image resized to size x size.  The flip comes after resize and crop.  selector, offset (y, x) and
  flip (0 / 1) override the draws; what is not given is drawn from rng in that order."""
  if selector is None:
    selector = int(rng.integers(0, 2))
  if selector not in (0, 1):
    raise ValueError('selector must be 0 or 1')
  if selector == 0:
    if size > _REID_RESIZE:
      raise ValueError('Crop size greater than the image size.')       # reid_preprocessing.py:414-418
    if offset is None:
      offset = (int(rng.integers(0, _REID_RESIZE - size + 1)), int(rng.integers(0, _REID_RESIZE - size + 1)))
    resize, (oy, ox) = _REID_RESIZE, (int(offset[0]), int(offset[1]))
  else:
    resize, (oy, ox) = int(size), (0, 0)
  if flip is None:
    flip = int(rng.random() < 0.5)
  return dict(crop_y=0, crop_x=0, crop_h=height, crop_w=width, resize_h=resize, resize_w=resize, out_y=oy, out_x=ox,
              flip=FLIP_AFTER if flip else FLIP_NONE)


def central_crop_window(height: int, width: int) -> Tuple[int, int, int, int]:
  """tf.image.central_crop(image, 0.875) -> (y, x, h, w): start = int((size - size * 0.875) / 2) = size // 16 and
  extent = size - 2 * start.  DESIGN.md 1.4."""
  y, x = height // 16, width // 16
  return y, x, height - 2 * y, width - 2 * x


def inception_eval_window(height: int, width: int, out_h: int, out_w: int):
  """preprocess_for_eval (inception_preprocessing.py:302-340): central_crop(0.875), then resize_bilinear to the output"""
  y, x, h, w = central_crop_window(height, width)
  return dict(crop_y=y, crop_x=x, crop_h=h, crop_w=w, resize_h=out_h, resize_w=out_w, out_y=0, out_x=0, flip=FLIP_NONE)


def inception_train_window(height: int, width: int, out_h: int, out_w: int, rng: Optional[np.random.Generator] = None,
                           box: Optional[Tuple[int, int, int, int]] = None, flip: Optional[int] = None,
                           min_object_covered: float = 0.1):
  """preprocess_for_train (inception_preprocessing.py:253-284): distorted_bounding_box_crop with the whole-image box
  (aspect 3/4..4/3, area min_object_covered..1), resize to the output, then random_flip_left_right.  box (y, x, h, w) and
  flip (0 / 1) override the draws."""
  if box is None:
    box = sample_distorted_bounding_box(height, width, rng, min_object_covered=min_object_covered,
                                        aspect_ratio_range=(3. / 4., 4. / 3.), area_range=(min_object_covered, 1.0))
  if flip is None:
    flip = int(rng.random() < 0.5)
  y, x, h, w = [int(v) for v in box]
  return dict(crop_y=y, crop_x=x, crop_h=h, crop_w=w, resize_h=out_h, resize_w=out_w, out_y=0, out_x=0,
              flip=FLIP_AFTER if flip else FLIP_NONE)


def sample_color_draws(rng: np.random.Generator, brightness_range: float = 32. / 255., cb_distortion_range: float = 0.1,
                       cr_distortion_range: float = 0.1) -> Tuple[float, float, float]:
  """the three uniform draws of distort_color_fast (inception_preprocessing.py:129-133) as float32: (br, cb, cr)"""
  return tuple(_F(rng.uniform(-r, r)) for r in (brightness_range, cb_distortion_range, cr_distortion_range))


def color_offsets(br, cb, cr) -> np.ndarray:
  """distort_color_fast's per-channel offsets (inception_preprocessing.py:136-138) -> float32 [3] (R, G, B), in float32 in
  the reference's order, every constant rounded to float32 first"""
  br, cb, cr = _F(br), _F(cb), _F(cr)
  r = _F(_F(1.402) * cr) + br
  g = _F(_F(_F(-0.344136) * cb) - _F(_F(0.714136) * cr)) + br
  b = _F(_F(1.772) * cb) + br
  return np.array([r, g, b], dtype=_F)


def _validate(win: dict, Hs: int, Ws: int, out_h: int, out_w: int):
  ok = (win['crop_h'] > 0 and win['crop_w'] > 0 and win['crop_y'] >= 0 and win['crop_x'] >= 0 and
        win['crop_y'] + win['crop_h'] <= Hs and win['crop_x'] + win['crop_w'] <= Ws and win['resize_h'] > 0 and
        win['resize_w'] > 0 and win['out_y'] >= 0 and win['out_x'] >= 0 and
        win['out_y'] + out_h <= win['resize_h'] and win['out_x'] + out_w <= win['resize_w'])
  if not ok:
    raise ValueError('window %r does not fit a %dx%d image / %dx%d output' % (win, Hs, Ws, out_h, out_w))


_DESC_DTYPE = np.dtype(lib.ImageDesc)       # struct asm_image_desc


def _fill_table(desc: np.ndarray, offs, sizes, windows, out_h: int, out_w: int):
  """rows [0, n) of a struct asm_image_desc table from the slot offsets, the (height, width) of every image and its window;
  raises ValueError for a window that does not fit"""
  n = len(sizes)
  for (h, w), win in zip(sizes, windows):
    _validate(win, h, w, out_h, out_w)
  if n:
    desc['src_offset'][:n] = offs
    desc['Hs'][:n] = [s[0] for s in sizes]
    desc['Ws'][:n] = [s[1] for s in sizes]
    for f in ('crop_y', 'crop_x', 'crop_h', 'crop_w', 'resize_h', 'resize_w', 'out_y', 'out_x', 'flip'):
      desc[f][:n] = [int(w[f]) for w in windows]


def pack_batch(images: Sequence[np.ndarray], windows: Sequence[dict], out_h: int, out_w: int, pin: bool = False):
  """Decoded images (uint8 [H, W, 3], any sizes) -> (packed uint8 buffer, descriptor table bytes) as CPU tensors
  (pinned when ``pin``): the host half of preprocess_batch for a batch without encoded files.  The buffer is the staging
  buffer itself, valid until the next batch is packed.  One memcpy per image and a vectorised descriptor table: ~10 GB/s
  on one core, so the host side keeps up with the GPU (the per-image tensor ops of the first version did 670 img/s)."""
  n = len(images)
  if n != len(windows):
    raise ValueError('one window per image')
  for im in images:
    if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
      raise ValueError('Input must be of size [height, width, 3] uint8')     # imagenet_preprocessing.py:143-144
  offs, total = staging.slot_layout([im.size for im in images])
  table = torch.zeros(n * _DESC_DTYPE.itemsize, dtype=torch.uint8, pin_memory=pin)
  _fill_table(table.numpy().view(_DESC_DTYPE), offs, [im.shape[:2] for im in images], windows, out_h, out_w)
  return staging.fill(max(total, 16), images, offs, pin), table


def _augment_tail(resize, n, side, is_training, dev, rng, subtract_mean, autoaugment_type, augment):
  """resize (+ AutoAugment in training) of a packed device buffer: the tail of preprocess_batch for the types that end in
  the mean subtraction.  resize(subtract_mean) -> float32 [n, side, side, 3] is the family's launch."""
  if autoaugment_type is None or not is_training:
    return resize(subtract_mean)
  if augment is None:
    rng = rng if rng is not None else np.random.default_rng()
    augment = _aa.sample(autoaugment_type, n, side, side, rng)
  _aa.validate(augment, side, side)
  if len(augment) != n:
    raise ValueError('one augmentation descriptor per image')
  return ops.autoaugment(resize(False), staging.upload_table(augment, dev), subtract_mean)


def _draw(draws, k, key):
  return None if draws is None else draws[k].get(key)


def preprocess_batch(images: Sequence[np.ndarray], is_training: bool, device, image_size: int = 224,
                     preprocessing_type: str = 'imagenet', use_random_crop: bool = True,
                     rng: Optional[np.random.Generator] = None, subtract_mean: bool = True,
                     windows: Optional[List[dict]] = None, autoaugment_type: Optional[str] = None,
                     augment: Optional[np.ndarray] = None, dct_method: str = '',
                     jpeg_fallback=None, jpeg_progressive: bool = False,
                     jpeg_entropy: str = 'sequential', jpeg_parse: str = 'host', jpeg_resident=None,
                     draws: Optional[List[dict]] = None, use_fast_color_distort: bool = True,
                     brightness_range: float = 32. / 255., cb_distortion_range: float = 0.1,
                     cr_distortion_range: float = 0.1) -> torch.Tensor:
  """data_util.preprocess_image for a batch of decoded images; float32 NHWC on `device`.
  `windows` overrides the sampled / computed windows (tests share them with the oracle).
  `autoaugment_type` ('imagenet' | 'good' | 'v0' | 'test'): in training mode the policy runs on the resized image, clipped
  and cast to uint8, before the mean subtraction (imagenet_preprocessing.py:280-289), as a second launch; the reference
  applies it in the training branch only, so evaluation ignores it.  `augment` overrides the sampled descriptors
  (autoaugment.sample / autoaugment.descriptor), the way `windows` overrides the windows.
  An entry of `images` that is bytes, a bytearray or a 1-D uint8 array is an encoded JPEG file: it is decoded on the device
  (`dct_method` '' or 'INTEGER_ACCURATE'; 'INTEGER_FAST' raises NotImplementedError), its size for the window arithmetic
  comes from its header, and a file of a kind the device does not decode goes through `jpeg_fallback(bytes) -> uint8
  [H, W, 3]` (NotImplementedError without one).  A training crop is a window of the full decode.
  `jpeg_progressive`: decode progressive files on the device as well (opt-in; they go to `jpeg_fallback` otherwise).
  `jpeg_entropy`: 'parallel' decodes each sequential file's scan on all lanes of a workgroup (opt-in, jpeg.py; the same
  pixels).
  `jpeg_parse`: 'device' reads the files' headers on the device as well (opt-in, jpeg.pack_device; the same pixels), and
  `jpeg_resident` then names files that lie on the device already -- records.Batch.payloads -- so that they are not
  uploaded again; `images` still holds the host bytes, read only for a file the device hands back.
  `preprocessing_type`: the imagenet* family, and
    'reid' / 'reid_224' (reid_preprocessing.py:497-540): training resizes the whole image to 256 x 256 and crops image_size
      at a random offset, or resizes it to image_size (a per-image selector), flips AFTER that, applies AutoAugment if
      asked and subtracts the means; evaluation resizes the whole image to reid_output_side(...) squared -- that, not
      image_size, is the output side -- and subtracts the means;
    'inception_331' / 'inception_600' (inception_preprocessing.py:204-368; image_size and autoaugment_type are ignored as in
      the reference): pixels scaled to [0, 1] before the interpolation; evaluation takes central_crop(0.875); training takes
      a sampled box, flips after the resize, adds color_offsets(br, cb, cr) per image and clamps to [0, 1].  The output has
      no mean to subtract, so subtract_mean=False raises ValueError; use_fast_color_distort=False raises
      NotImplementedError.  The three ranges are the reference's flag defaults.
  `draws`: one dict per image overriding what these two families sample in training -- 'selector', 'offset' (y, x), 'flip'
  (0 / 1) for re-ID; 'box' (y, x, h, w), 'flip', 'color' (br, cb, cr) for Inception; a missing key is drawn from `rng`.
  With `windows` given only 'color' is read."""
  segment_bytes = _jpeg.check_modes(jpeg_entropy, None, jpeg_parse, jpeg_resident, prefix='jpeg_')
  family = preprocessing_family(preprocessing_type)
  if family == 'inception':
    if not use_fast_color_distort:
      raise NotImplementedError('use_fast_color_distort=False (the hue / saturation / contrast orderings of distort_color) '
                                'is not implemented')
    if not subtract_mean:
      raise ValueError('preprocessing_type %r gives pixels in [0, 1] with no channel mean for the trainer to subtract: '
                       'subtract_mean=False does not apply' % preprocessing_type)
    autoaugment_type = None       # inception_preprocessing.preprocess_image takes no policy
  if autoaugment_type is not None:
    _aa.check_policy_name(autoaugment_type)
  if family == 'reid':
    side = reid_output_side(preprocessing_type, is_training, image_size)
  elif family == 'inception':
    side = _INCEPTION_SIDE[preprocessing_type]
  else:
    side, crop_type = output_size_and_crop_type(preprocessing_type, is_training, image_size)
  if draws is not None and len(draws) != len(images):
    raise ValueError('one dict of draws per image')
  if any(_jpeg.is_encoded(im) for im in images):
    _jpeg.check_dct_method(dct_method)
  # encoded files are decoded on the device into their slots of the packed buffer, decoded arrays (given, or returned by
  # the fallback) travel to theirs in one staged copy; one window and one descriptor per slot
  if jpeg_parse == 'device':
    pk = _jpeg.pack_device(images, device, jpeg_resident, jpeg_fallback, progressive=jpeg_progressive,
                           segment_bytes=segment_bytes)
  else:
    pk = _jpeg.pack(images, jpeg_fallback, progressive=jpeg_progressive, segment_bytes=segment_bytes)
  if is_training and rng is None and (windows is None or family == 'inception'):
    rng = np.random.default_rng()
  if windows is None:
    if family == 'reid':
      windows = [reid_train_window(h, w, side, rng, _draw(draws, k, 'selector'), _draw(draws, k, 'offset'),
                                   _draw(draws, k, 'flip')) if is_training else reid_eval_window(h, w, side)
                 for k, (h, w) in enumerate(pk.sizes)]
    elif family == 'inception':
      windows = [inception_train_window(h, w, side, side, rng, _draw(draws, k, 'box'), _draw(draws, k, 'flip'))
                 if is_training else inception_eval_window(h, w, side, side) for k, (h, w) in enumerate(pk.sizes)]
    elif is_training:
      windows = [train_window(h, w, side, side, rng, use_random_crop) for h, w in pk.sizes]
    else:
      windows = [eval_window(h, w, side, side, crop_type) for h, w in pk.sizes]
  n = len(images)
  if n != len(windows):
    raise ValueError('one window per image')
  if family != 'imagenet' and any(int(w['flip']) not in (FLIP_NONE, FLIP_BEFORE, FLIP_AFTER) for w in windows):
    raise ValueError('flip must be 0 (none), 1 (before the resize) or 2 (after resize and crop)')
  desc = np.zeros(n, dtype=_DESC_DTYPE)
  _fill_table(desc, pk.offsets, pk.sizes, windows, side, side)
  dev = torch.device(device)
  bd = _jpeg.decode_packed(pk, dev, entropy=jpeg_entropy)[0]
  td = staging.upload_table(desc, dev)
  if family == 'inception':
    if not is_training:
      return ops.preprocess_window(bd, td, n, side, side, ops.SOURCE_UNIT, ops.TAIL_NONE)
    add = np.zeros((n, 3), dtype=_F)
    for k in range(n):
      color = _draw(draws, k, 'color')
      if color is None:
        color = sample_color_draws(rng, brightness_range, cb_distortion_range, cr_distortion_range)
      add[k] = color_offsets(*color)
    add_dev = staging.upload_table(add, dev).view(torch.float32).view(n, 3)
    return ops.preprocess_window(bd, td, n, side, side, ops.SOURCE_UNIT, ops.TAIL_ADD_CLAMP, add_dev)
  if family == 'reid':
    resize = lambda sub: ops.preprocess_window(bd, td, n, side, side, ops.SOURCE_BYTES,          # noqa: E731
                                               ops.TAIL_MEANS if sub else ops.TAIL_NONE)
  else:
    resize = lambda sub: ops.resize_crop_flip(bd, td, n, side, side, sub)                        # noqa: E731
  return _augment_tail(resize, n, side, is_training, dev, rng, subtract_mean, autoaugment_type, augment)
