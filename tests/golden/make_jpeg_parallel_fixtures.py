"""Writes tests/golden/jpeg_parallel_fixtures.npz: the files the segment-parallel entropy stage (asm_jpeg_decode_parallel)
is tested on beside those of jpeg_fixtures.npz, and the pixels Pillow decodes them to.  Same layout (names, kind_<name>,
file_<name>, pix_<name>); every file is of the 'device' kind.  Runs where Pillow is installed; the tests only read the
result.

  python tests/golden/make_jpeg_parallel_fixtures.py

What the set is for: a scan with more 16-byte segments than a workgroup has lanes, every sampling layout and grey at a
size of a few dozen segments, restart intervals that are several segments long, and a scan dense in stuffed FF 00 pairs
so that segment boundaries fall between an FF and its 00.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from make_jpeg_fixtures import encode, noise, smooth  # noqa: E402
from tests import jpeg_ref  # noqa: E402


def textured(w, h, rng, amplitude=10):
  """smooth + noise: photographic-like statistics, blocks of a few dozen bits to a few hundred"""
  im = smooth(w, h, rng).astype(np.int64) + rng.integers(-amplitude, amplitude + 1, size=(h, w, 3))
  return np.clip(im, 0, 255).astype(np.uint8)


def split_pairs(data, segment_bytes=16):
  """segment boundaries of the (single-interval) scan that fall between an FF and its stuffing 00"""
  from assembled_cnn_amd import jpeg
  info = jpeg.parse(data)
  a = np.frombuffer(data, np.uint8)
  count = 0
  for begin, end in info.intervals:
    for o in range(int(begin) + segment_bytes, int(end), segment_bytes):
      count += int(a[o - 1] == 0xFF and a[o] == 0x00)
  return count


def main():
  import io
  from PIL import Image
  rng = np.random.default_rng(20261019)
  files = [
      ('tex_120x80_420', encode(textured(120, 80, rng), quality=90, subsampling=2)),
      ('tex_56x40_444', encode(textured(56, 40, rng), quality=95, subsampling=0)),
      ('tex_56x40_422', encode(textured(56, 40, rng), quality=95, subsampling=1)),
      ('tex_grey_56x40', encode(textured(56, 40, rng), 'L', quality=95)),
      ('rstrow_tex_120x80_420', encode(textured(120, 80, rng), quality=90, subsampling=2, restart_marker_rows=1)),
  ]
  while True:       # white noise at quality 100, drawn again until a 16-byte boundary splits a stuffed pair
    data = encode(noise(32, 24, rng), quality=100, subsampling=0)
    if split_pairs(data) >= 1:
      break
  files.append(('stuffed_noise_32x24_444', data))
  # several passes of a 256-lane workgroup over its segments at 16 bytes
  files.append(('tex_200x152_420', encode(textured(200, 152, rng), quality=90, subsampling=2)))
  out = {'names': np.array([f[0] for f in files])}
  for name, data in files:
    out['kind_' + name] = np.array('device')
    out['file_' + name] = np.frombuffer(data, np.uint8)
    pix = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
    out['pix_' + name] = pix
    assert np.array_equal(jpeg_ref.decode(data), pix), name
  from assembled_cnn_amd import jpeg
  big = jpeg.parse(files[6][1])
  segments = -(-(big.scan_end - big.scan_begin) // 16)
  assert segments > 2 * 256 and -(-(jpeg.parse(files[0][1]).scan_end - jpeg.parse(files[0][1]).scan_begin) // 16) > 256, 'the largest scan has %d 16-byte segments, no more than a workgroup has lanes' % segments
  rst = jpeg.parse(files[4][1])
  assert len(rst.intervals) > 1 and np.all(rst.intervals[:-1, 1] - rst.intervals[:-1, 0] > 3 * 16)
  pairs = split_pairs(files[5][1])
  assert pairs >= 1, 'no 16-byte segment boundary falls between an FF and its 00'
  path = os.path.join(HERE, 'jpeg_parallel_fixtures.npz')
  np.savez_compressed(path, **out)
  print('%d files, %d file bytes; %s: %d segments of 16 bytes; %s: %d intervals; %s: %d stuffed bytes, %d segment '
        'boundaries between an FF and its 00 -> %s (%d bytes)' % (
            len(files), sum(len(f[1]) for f in files), files[6][0], segments, files[4][0], len(rst.intervals), files[5][0],
            jpeg_ref.stats(files[5][1])['stuffed'], pairs, path, os.path.getsize(path)))


if __name__ == '__main__':
  main()
