"""numpy float32 restatement of the reference's re-ID and Inception preprocessing (preprocessing/reid_preprocessing.py:489-540,
preprocessing/inception_preprocessing.py:117-368): the window arithmetic of each branch plus the pixel rule -- legacy TF 1.14
bilinear resize without half-pixel centres, float32 in the order top = tl + (tr - tl) * x_lerp, v = top + (bot - top) *
y_lerp.  Every operation is a float32 numpy operation in the order the reference's graph runs it, so it reproduces
tests/golden/reference_preprocessing.* with array_equal (tests/test_preprocess_types_cpu.py) and is what the GPU tests
compare the kernel with.  Nothing here imports the product."""
import numpy as np

F = np.float32
CHANNEL_MEANS = np.array([123.68, 116.78, 103.94], dtype=F)
FLIP_NONE, FLIP_BEFORE, FLIP_AFTER = 0, 1, 2
SOURCE_BYTES, SOURCE_UNIT = 0, 1
TAIL_NONE, TAIL_MEANS, TAIL_ADD_CLAMP = 0, 1, 2
REID_RESIZE = 256


def _axis(in_size, resize, first, count):
  """output indices first .. first + count - 1 of an axis resized from in_size to resize -> (lower, upper, lerp)"""
  scale = F(in_size) / F(resize)
  coord = (np.arange(count) + first).astype(F) * scale
  lower = coord.astype(np.int64)
  return lower, np.minimum(lower + 1, in_size - 1), coord - lower.astype(F)


def window_pixels(image, win, out_h, out_w, source=SOURCE_BYTES, tail=TAIL_NONE, add=None):
  """uint8 [H, W, 3] + a window (the keys of struct asm_image_desc) -> float32 [out_h, out_w, 3]"""
  w = image[win['crop_y']:win['crop_y'] + win['crop_h'], win['crop_x']:win['crop_x'] + win['crop_w']].astype(F)
  assert w.shape[:2] == (win['crop_h'], win['crop_w']) and win['flip'] in (FLIP_NONE, FLIP_BEFORE, FLIP_AFTER)
  if source == SOURCE_UNIT:
    w = w * F(1.0 / 255)
  if win['flip'] == FLIP_BEFORE:
    w = w[:, ::-1]
  ly, uy, fy = _axis(win['crop_h'], win['resize_h'], win['out_y'], out_h)
  lx, ux, fx = _axis(win['crop_w'], win['resize_w'], win['out_x'], out_w)
  fy, fx = fy[:, None, None], fx[None, :, None]
  tl, tr, bl, br = w[ly][:, lx], w[ly][:, ux], w[uy][:, lx], w[uy][:, ux]
  top = tl + (tr - tl) * fx
  bot = bl + (br - bl) * fx
  v = top + (bot - top) * fy
  if win['flip'] == FLIP_AFTER:
    v = v[:, ::-1]
  if tail == TAIL_MEANS:
    v = v - CHANNEL_MEANS
  elif tail == TAIL_ADD_CLAMP:
    if add is not None:
      v = v + np.asarray(add, dtype=F)
    v = np.minimum(np.maximum(v, F(0)), F(1))
  assert v.dtype == F
  return np.ascontiguousarray(v)


def _window(crop, resize, out, flip):
  return dict(crop_y=crop[0], crop_x=crop[1], crop_h=crop[2], crop_w=crop[3], resize_h=resize[0], resize_w=resize[1],
              out_y=out[0], out_x=out[1], flip=flip)


# ---- re-ID ------------------------------------------------------------------------------------------------------------
def reid_train_window(h, w, size, selector, offset, flip, flip_code=FLIP_AFTER):
  if selector == 0:
    assert size <= REID_RESIZE
    return _window((0, 0, h, w), (REID_RESIZE, REID_RESIZE), tuple(offset), flip_code if flip else FLIP_NONE)
  return _window((0, 0, h, w), (size, size), (0, 0), flip_code if flip else FLIP_NONE)


def reid_train(image, size, selector, offset, flip, subtract_mean=True, flip_code=FLIP_AFTER):
  win = reid_train_window(image.shape[0], image.shape[1], size, selector, offset, flip, flip_code)
  return window_pixels(image, win, size, size, SOURCE_BYTES, TAIL_MEANS if subtract_mean else TAIL_NONE)


def reid_eval_side(size, large):
  return int(size * (1.0 / 0.875)) if large else size


def reid_eval(image, size, large):
  side = reid_eval_side(size, large)
  win = _window((0, 0, image.shape[0], image.shape[1]), (side, side), (0, 0), FLIP_NONE)
  return window_pixels(image, win, side, side, SOURCE_BYTES, TAIL_MEANS)


# ---- Inception --------------------------------------------------------------------------------------------------------
def central_crop_box(h, w):
  y, x = int((h - h * 0.875) / 2), int((w - w * 0.875) / 2)
  return y, x, h - 2 * y, w - 2 * x


def inception_eval(image, out_h, out_w):
  win = _window(central_crop_box(image.shape[0], image.shape[1]), (out_h, out_w), (0, 0), FLIP_NONE)
  return window_pixels(image, win, out_h, out_w, SOURCE_UNIT, TAIL_NONE)


def color_offsets(br, cb, cr):
  br, cb, cr = F(br), F(cb), F(cr)
  return np.array([F(1.402) * cr + br, (F(-0.344136) * cb - F(0.714136) * cr) + br, F(1.772) * cb + br], dtype=F)


def inception_train(image, out_h, out_w, box, flip, color, flip_code=FLIP_AFTER):
  win = _window(tuple(box), (out_h, out_w), (0, 0), flip_code if flip else FLIP_NONE)
  return window_pixels(image, win, out_h, out_w, SOURCE_UNIT, TAIL_ADD_CLAMP, color_offsets(*color))
