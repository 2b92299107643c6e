"""Writes tests/golden/jpeg_progressive_fixtures.npz: small progressive (SOF2) JPEG files and the pixels Pillow
(libjpeg-turbo, ISLOW inverse DCT, fancy upsampling) decodes them to.  Runs where Pillow is installed; the tests only read
the result.

  python tests/golden/make_jpeg_progressive_fixtures.py

Entries: names (in order), file_<name> (uint8 bytes), pix_<name> (uint8 [H, W, 3]).  The smallest shapes that can go
wrong: one pixel, one block, odd chroma widths and heights, partial MCUs (where a scan of one component walks fewer
blocks than the padded grid has), every sampling layout, flat images whose end-of-band runs span many blocks, restart
intervals that wrap RSTm and give a lane a second interval in the scans of one component, a DRI that changes between
scans.  Asserted here: tests/jpeg_progressive_ref.py reproduces every file's pixels bit for bit.
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import jpeg_progressive_ref  # noqa: E402
from tests.golden.make_jpeg_fixtures import SUB, encode, noise, smooth  # noqa: E402


def main():
  rng = np.random.default_rng(20261019)
  files = []      # (name, bytes)
  for (w, h) in ((1, 1), (8, 8), (9, 7), (13, 17), (31, 9), (17, 33)):
    for sub in ('444', '422', '420'):
      files.append(('smooth_%dx%d_%s' % (w, h, sub), encode(smooth(w, h, rng), quality=75, subsampling=SUB[sub],
                                                           progressive=True)))
      files.append(('noise_%dx%d_%s' % (w, h, sub), encode(noise(w, h, rng), quality=100, subsampling=SUB[sub],
                                                         progressive=True)))
  # chroma planes of two columns
  files.append(('smooth_3x5_420', encode(smooth(3, 5, rng), quality=90, subsampling=2, progressive=True)))
  files.append(('noise_4x3_422', encode(noise(4, 3, rng), quality=95, subsampling=1, progressive=True)))
  files.append(('grey_13x17', encode(smooth(13, 17, rng), 'L', quality=85, progressive=True)))
  files.append(('grey_noise_q30_31x29', encode(noise(31, 29, rng), 'L', quality=30, progressive=True)))
  # long end-of-band runs
  files.append(('flat_20x20_420', encode(np.full((20, 20, 3), 77, np.uint8), quality=75, subsampling=2, progressive=True)))
  files.append(('flat_grey_72x72', encode(np.full((72, 72, 3), 150, np.uint8), 'L', quality=75, progressive=True)))
  files.append(('rst1_grey_40x48', encode(noise(40, 48, rng), 'L', quality=90, progressive=True, restart_marker_blocks=1)))
  files.append(('rst1_444_40x48', encode(smooth(40, 48, rng), quality=80, subsampling=0, progressive=True,
                                         restart_marker_blocks=1)))
  files.append(('rst2_422_33x47', encode(noise(33, 47, rng), quality=70, subsampling=1, progressive=True,
                                         restart_marker_blocks=2)))
  files.append(('rstrow_422_48x40', encode(smooth(48, 40, rng), quality=85, subsampling=1, progressive=True,
                                           restart_marker_rows=1)))
  files.append(('rstrow_420_noise_24x40', encode(noise(24, 40, rng), quality=50, subsampling=2, progressive=True,
                                                 restart_marker_rows=1)))
  files.append(('noopt_420_31x29', encode(noise(31, 29, rng), quality=60, subsampling=2, progressive=True, optimize=False)))

  out = {'names': np.array([f[0] for f in files])}
  kinds, dris = set(), set()
  for name, data in files:
    out['file_' + name] = np.frombuffer(data, np.uint8)
    pix = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
    out['pix_' + name] = pix
    assert np.array_equal(jpeg_progressive_ref.decode(data), pix), name      # the reference reproduces Pillow bit for bit
    scans = jpeg_progressive_ref.read_scans(data)['scans']
    kinds |= set((sc['ss'] > 0, sc['ah'] > 0) for sc in scans)
    if name.startswith('rstrow_422'):
      dris = set(sc['ri'] for sc in scans)
  assert len(kinds) == 4, 'not all four scan kinds occur'
  assert len(dris) > 1, 'DRI does not change between the scans of the restart_marker_rows file'
  path = os.path.join(HERE, 'jpeg_progressive_fixtures.npz')
  np.savez_compressed(path, **out)
  size = os.path.getsize(path)
  assert size < 256 * 1024, size
  print('%d files, %d file bytes, %d pixel bytes -> %s (%d bytes)' % (
      len(files), sum(len(f[1]) for f in files), sum(v.size for k, v in out.items() if k.startswith('pix_')), path, size))


if __name__ == '__main__':
  main()
