"""Writes tests/golden/jpeg_fixtures.npz: small JPEG files and the pixels Pillow (libjpeg-turbo, ISLOW inverse DCT, fancy
upsampling) decodes them to.  Runs where Pillow is installed (the development machine); the tests only read the result.

  python tests/golden/make_jpeg_fixtures.py

Entries: names (in order), kind_<name> ('device' | 'progressive' | 'cmyk'), file_<name> (uint8 bytes), pix_<name> (uint8
[H, W, 3], device kinds only).  The smallest shapes that can go wrong: one pixel, one block, odd chroma widths and
heights, partial MCUs, every sampling layout, restart intervals that wrap RSTm and that give a lane a second interval,
optimised tables, a flat image whose every AC run is an immediate EOB.
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import jpeg_ref  # noqa: E402

SUB = {'444': 0, '422': 1, '420': 2}


def smooth(w, h, rng):
  y, x = np.mgrid[0:h, 0:w].astype(np.float64)
  ph = rng.uniform(0, 6.28, size=(3, 2))
  im = np.stack([127 + 110 * np.sin(x / (2.0 + c) + ph[c, 0]) * np.cos(y / (3.0 + c) + ph[c, 1]) for c in range(3)], axis=-1)
  return np.clip(im, 0, 255).astype(np.uint8)


def noise(w, h, rng):
  return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def encode(arr, mode='RGB', **kw):
  im = Image.fromarray(arr if mode != 'L' else arr[..., 0], mode)
  buf = io.BytesIO()
  im.save(buf, 'JPEG', **kw)
  return buf.getvalue()


def main():
  rng = np.random.default_rng(20261018)
  files = []      # (name, kind, bytes)
  for (w, h) in ((1, 1), (8, 8), (13, 17), (31, 9), (17, 33)):
    for sub in ('444', '422', '420'):
      files.append(('smooth_%dx%d_%s' % (w, h, sub), 'device', encode(smooth(w, h, rng), quality=75, subsampling=SUB[sub])))
      files.append(('noise_%dx%d_%s' % (w, h, sub), 'device', encode(noise(w, h, rng), quality=100, subsampling=SUB[sub])))
  # chroma planes of two columns: libjpeg replicates those, the triangle filter starts at three
  files.append(('smooth_3x5_420', 'device', encode(smooth(3, 5, rng), quality=90, subsampling=2)))
  files.append(('noise_4x3_422', 'device', encode(noise(4, 3, rng), quality=95, subsampling=1)))
  files.append(('grey_13x17', 'device', encode(smooth(13, 17, rng), 'L', quality=85)))
  files.append(('rst1_grey_40x48', 'device', encode(noise(40, 48, rng), 'L', quality=90, restart_marker_blocks=1)))
  files.append(('rst1_444_40x48', 'device', encode(smooth(40, 48, rng), quality=80, subsampling=0, restart_marker_blocks=1)))
  files.append(('rst1_444_noise_72x72', 'device', encode(noise(72, 72, rng), quality=30, subsampling=0,
                                                         restart_marker_blocks=1)))
  files.append(('rstrow_420_48x64', 'device', encode(smooth(48, 64, rng), quality=85, subsampling=2, restart_marker_rows=1)))
  files.append(('rst2_422_33x47', 'device', encode(noise(33, 47, rng), quality=70, subsampling=1, restart_marker_blocks=2)))
  files.append(('opt_420_31x29', 'device', encode(noise(31, 29, rng), quality=60, subsampling=2, optimize=True)))
  files.append(('opt_444_24x20', 'device', encode(smooth(24, 20, rng), quality=92, subsampling=0, optimize=True)))
  files.append(('flat_20x20', 'device', encode(np.full((20, 20, 3), 77, np.uint8), quality=75, subsampling=2)))
  files.append(('progressive_16x16', 'progressive', encode(smooth(16, 16, rng), quality=75, progressive=True)))
  cmyk = io.BytesIO()
  Image.fromarray(noise(16, 16, rng)).convert('CMYK').save(cmyk, 'JPEG', quality=75)
  files.append(('cmyk_16x16', 'cmyk', cmyk.getvalue()))

  out = {'names': np.array([f[0] for f in files])}
  longest, stuffed = 0, 0
  for name, kind, data in files:
    out['kind_' + name] = np.array(kind)
    out['file_' + name] = np.frombuffer(data, np.uint8)
    if kind != 'device':
      continue
    pix = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
    out['pix_' + name] = pix
    assert np.array_equal(jpeg_ref.decode(data), pix), name      # the reference reproduces Pillow bit for bit
    st = jpeg_ref.stats(data)
    longest, stuffed = max(longest, st['max_code_length']), stuffed + st['stuffed']
  assert longest == 16, 'no file uses a 16-bit Huffman code (longest %d)' % longest
  assert stuffed > 0, 'no file contains a stuffed FF 00'
  path = os.path.join(HERE, 'jpeg_fixtures.npz')
  np.savez_compressed(path, **out)
  print('%d files, %d file bytes, %d pixel bytes, longest code %d, %d stuffed bytes -> %s (%d bytes)' % (
      len(files), sum(len(f[2]) for f in files), sum(v.size for k, v in out.items() if k.startswith('pix_')), longest,
      stuffed, path, os.path.getsize(path)))


if __name__ == '__main__':
  main()
