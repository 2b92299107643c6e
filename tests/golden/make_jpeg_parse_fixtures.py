"""Writes tests/golden/jpeg_parse_fixtures.npz: the one file the device header parser (asm_jpeg_parse /
asm_jpeg_parse_fill) is tested on beside those of jpeg_fixtures.npz and jpeg_parallel_fixtures.npz, and the pixels Pillow
decodes it to.  Same layout (names, kind_<name>, file_<name>, pix_<name>).  Runs where Pillow is installed; the tests only
read the result.

  python tests/golden/make_jpeg_parse_fixtures.py

What the file is for: a restart marker behind every MCU of a grey image gives more restart intervals (420) than the
parsing workgroup has lanes (256), so its interval rows and segment entries are written in several passes.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from make_jpeg_fixtures import encode, noise  # noqa: E402
from tests import jpeg_ref  # noqa: E402


def main():
  import io
  from PIL import Image
  from assembled_cnn_amd import jpeg
  rng = np.random.default_rng(20261020)
  name, data = 'rst1_grey_168x160', encode(noise(168, 160, rng), 'L', quality=60, restart_marker_blocks=1)
  pix = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
  assert np.array_equal(jpeg_ref.decode(data), pix), name
  info = jpeg.parse(data)
  assert info.unsupported is None and len(info.intervals) == 420, len(info.intervals)
  pk = jpeg.pack([data], segment_bytes=16)
  out = {'names': np.array([name]), 'kind_' + name: np.array('device'), 'file_' + name: np.frombuffer(data, np.uint8),
         'pix_' + name: pix}
  path = os.path.join(HERE, 'jpeg_parse_fixtures.npz')
  np.savez_compressed(path, **out)
  print('%s: %d bytes, %d intervals, %d segments of 16 bytes -> %s (%d bytes)' % (
      name, len(data), len(info.intervals), pk.total_segments, path, os.path.getsize(path)))


if __name__ == '__main__':
  main()
