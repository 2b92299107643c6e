"""CPU restatement of the reference's AutoAugment ops (test infrastructure only): plain numpy, one function per op,
written from preprocessing/autoaugment.py:316-679; float32 wherever the reference's graph computes in float32.  It is
PINNED to the reference's own source by tests/golden/reference_autoaugment.npz (tests/test_autoaugment_cpu.py) and is
what the HIP kernel is compared with (tests/test_gpu_autoaugment.py).  Nothing here calls the product package.

Images are uint8 [H, W, 3].  [TF-sem] rules: float -> uint8 casts truncate toward zero;
rgb_to_grayscale on uint8 is * (1/255), weighted sum in channel order, * 255.5, truncate; histogram_fixed_width on
integers 0..255 has bin = value; tf.contrib.image.transform is NEAREST with round-half-away-from-zero and zero outside.
"""
import math

import numpy as np

F = np.float32
CHANNEL_MEANS = np.array([123.68, 116.78, 103.94], dtype=np.float32)     # imagenet_preprocessing.py:46-49
REPLACE = 128                                                              # autoaugment.py:836


def to_uint8(image_f32):
  """imagenet_preprocessing.py:284-286: clip_by_value(image, 0, 255) then tf.cast(uint8)"""
  return np.clip(np.asarray(image_f32, dtype=F), F(0), F(255)).astype(np.int32).astype(np.uint8)


def _trunc_u8(x):
  return x.astype(np.int32).astype(np.uint8)       # int32 first: truncation toward zero, then the low 8 bits


def blend(image1, image2, factor):                 # :334-356
  factor = F(factor)
  if factor == 0.0:
    return np.array(image1, dtype=np.uint8)
  if factor == 1.0:
    return np.array(image2, dtype=np.uint8)
  a, b = image1.astype(F), image2.astype(F)
  difference = (b - a).astype(F)
  scaled = (factor * difference).astype(F)
  temp = (a + scaled).astype(F)
  if 0.0 < factor < 1.0:
    return _trunc_u8(temp)
  return _trunc_u8(np.clip(temp, F(0), F(255)))


def rgb_to_grayscale(image):
  f = image.astype(F) * F(1.0 / 255.0)
  s = f[..., 0] * F(0.2989)
  s = s + f[..., 1] * F(0.5870)
  s = s + f[..., 2] * F(0.1140)
  return _trunc_u8(s * F(255.5))


def cutout(image, pad_size, centre_y, centre_x, replace=REPLACE):      # :359-407, the centre draws handed in
  H, W = image.shape[:2]
  lower, upper = max(0, centre_y - pad_size), max(0, H - centre_y - pad_size)
  left, right = max(0, centre_x - pad_size), max(0, W - centre_x - pad_size)
  out = image.copy()
  if pad_size > 0:                                  # pad size 0: nothing is filled (this project's choice)
    out[lower:H - upper, left:W - right] = replace
  return out


def solarize(image, threshold=128):                # :410-414; compared as int, so threshold 256 keeps every pixel
  v = image.astype(np.int32)
  return np.where(v < threshold, v, 255 - v).astype(np.uint8)


def solarize_add(image, addition=0, threshold=128):    # :417-424
  v = image.astype(np.int64)
  added = np.clip(v + addition, 0, 255)
  return np.where(v < threshold, added, v).astype(np.uint8)


def color(image, factor):                          # :427-430
  gray = rgb_to_grayscale(image)
  return blend(np.repeat(gray[..., None], 3, axis=2), image, factor)


def contrast(image, factor):                       # :433-447: "mean" is the histogram's SUM over 256 = pixel count / 256
  H, W = image.shape[:2]
  mean = F(H * W) / F(256.0)
  degenerate = np.full(image.shape, np.clip(mean, F(0), F(255)), dtype=F)
  return blend(_trunc_u8(degenerate), image, factor)


def brightness(image, factor):                     # :450-453
  return blend(np.zeros_like(image), image, factor)


def posterize(image, bits):                        # :456-459; bits = 0 shifts by 8: defined as 0
  shift = 8 - bits
  v = image.astype(np.int32)
  return (((v >> shift) << shift) & 255).astype(np.uint8)


def autocontrast(image):                           # :521-557
  out = np.empty_like(image)
  for c in range(3):
    ch = image[..., c]
    lo, hi = F(ch.min()), F(ch.max())
    if hi > lo:
      scale = F(255.0) / (hi - lo)
      offset = -lo * scale
      im = (ch.astype(F) * scale).astype(F) + offset
      out[..., c] = _trunc_u8(np.clip(im, F(0), F(255)))
    else:
      out[..., c] = ch
  return out


def sharpness(image, factor):                      # :560-586
  H, W = image.shape[:2]
  result = image.copy()
  if H >= 3 and W >= 3:
    f = image.astype(F)
    w = [F(1) / F(13)] * 9
    w[4] = F(5) / F(13)
    acc = np.zeros((H - 2, W - 2, 3), dtype=F)
    for k in range(9):                             # nine taps, row-major
      dy, dx = divmod(k, 3)
      acc = (acc + (f[dy:dy + H - 2, dx:dx + W - 2] * w[k]).astype(F)).astype(F)
    result[1:-1, 1:-1] = _trunc_u8(np.clip(acc, F(0), F(255)))
  return blend(result, image, factor)


def equalize(image):                               # :589-627
  out = np.empty_like(image)
  for c in range(3):
    ch = image[..., c].astype(np.int64)
    histo = np.bincount(ch.reshape(-1), minlength=256)
    nonzero = histo[histo != 0]
    step = (nonzero.sum() - nonzero[-1]) // 255
    if step == 0:
      out[..., c] = ch
    else:
      lut = (np.cumsum(histo) + step // 2) // step
      lut = np.clip(np.concatenate([[0], lut[:-1]]), 0, 255)
      out[..., c] = lut[ch]
  return out


def invert(image):                                 # :630-633
  return (255 - image.astype(np.int32)).astype(np.uint8)


def transform(image, coeffs, replace=REPLACE):
  """wrap -> tf.contrib.image.transform (NEAREST) -> unwrap (:636-679): output (x, y) reads input
  (round(a0 x + a1 y + a2), round(b0 x + b1 y + b2)); outside the image the alpha channel reads 0 -> `replace`."""
  H, W = image.shape[:2]
  a0, a1, a2, b0, b1, b2 = [F(v) for v in coeffs]
  x = np.arange(W, dtype=F)[None, :]
  y = np.arange(H, dtype=F)[:, None]
  sx = ((a0 * x).astype(F) + (a1 * y).astype(F)).astype(F) + a2
  sy = ((b0 * x).astype(F) + (b1 * y).astype(F)).astype(F) + b2
  rx, ry = _round_half_away(sx), _round_half_away(sy)
  inside = (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
  ix = np.where(inside, rx, 0).astype(np.int64)
  iy = np.where(inside, ry, 0).astype(np.int64)
  out = image[iy, ix]
  out[~inside] = replace
  return out


def _round_half_away(v):
  # in float64, where float32 + 0.5 is exact (in float32, 0.49999997 + 0.5 would round up to 1)
  v64 = v.astype(np.float64)
  return np.where(v64 >= 0, np.floor(v64 + 0.5), np.ceil(v64 - 0.5))


def rotate_coeffs(degrees, H, W):
  """rotate (:462-484) -> angles_to_projective_transforms, float32; cos / sin taken in double and rounded"""
  radians = F(degrees) * F(math.pi / 180.0)
  c, s = F(math.cos(float(radians))), F(math.sin(float(radians)))
  w1, h1 = F(W - 1), F(H - 1)
  x_offset = (w1 - (c * w1 - s * h1)) / F(2)
  y_offset = (h1 - (s * w1 + c * h1)) / F(2)
  return [c, -s, x_offset, s, c, y_offset]


def rotate(image, degrees, replace=REPLACE):
  return transform(image, rotate_coeffs(degrees, image.shape[0], image.shape[1]), replace)


def translate_x(image, pixels, replace=REPLACE):   # :487-490: translate by [-pixels, 0] -> matrix [1, 0, pixels, 0, 1, 0]
  return transform(image, [1, 0, F(pixels), 0, 1, 0], replace)


def translate_y(image, pixels, replace=REPLACE):   # :493-496
  return transform(image, [1, 0, 0, 0, 1, F(pixels)], replace)


def shear_x(image, level, replace=REPLACE):        # :499-507
  return transform(image, [1, F(level), 0, 0, 1, 0], replace)


def shear_y(image, level, replace=REPLACE):        # :510-518
  return transform(image, [1, 0, 0, F(level), 1, 0], replace)


NAME_TO_FUNC = {'AutoContrast': autocontrast, 'Equalize': equalize, 'Invert': invert, 'Rotate': rotate,
                'Posterize': posterize, 'Solarize': solarize, 'SolarizeAdd': solarize_add, 'Color': color,
                'Contrast': contrast, 'Brightness': brightness, 'Sharpness': sharpness, 'ShearX': shear_x,
                'ShearY': shear_y, 'TranslateX': translate_x, 'TranslateY': translate_y, 'Cutout': cutout}


def apply_ops(image_u8, ops):
  """ops: list of (name, arg...) tuples or None (slot not applied), applied in order"""
  for spec in ops:
    if spec is not None:
      image_u8 = NAME_TO_FUNC[spec[0]](image_u8, *spec[1:])
  return image_u8


def augment(image_f32, ops, subtract_mean):
  """what the device computes for one image: clip / truncate, the ops, float32 out (minus the means)"""
  out = apply_ops(to_uint8(image_f32), ops).astype(F)
  return (out - CHANNEL_MEANS).astype(F) if subtract_mean else out
