"""The CPU double of tests/cpu_double.py plus the one entry point the re-ID and Inception preprocessing types add,
asm_preprocess_window.  Its pixel rule is tests/preprocess_ref.window_pixels -- the restatement that
tests/golden/reference_preprocessing.* pins -- so what a test through this double checks is the host side: the dispatch, the
windows, the tables and the mode values that input_pipeline.preprocess_batch hands to the entry point."""
import numpy as np
import torch

from tests import preprocess_ref as R
from tests.cpu_double import CpuDouble, T


class PreprocessDouble(CpuDouble):
  def __init__(self):
    super().__init__()
    self.window_calls = []        # (N, out_h, out_w, source, tail, add given)

  def asm_preprocess_window(self, src, src_bytes, descs, N, out_h, out_w, source, tail, add, out, stream):
    from assembled_cnn_amd.lib import ImageDesc
    if N < 0 or out_h <= 0 or out_w <= 0 or src_bytes < 0:
      self._err = b'preprocess_window: bad sizes'
      return -1
    if source not in (0, 1) or tail not in (0, 1, 2):
      self._err = b'preprocess_window: unknown source or tail mode'
      return -1
    if add and tail != 2:
      self._err = b'preprocess_window: an add table needs the add-and-clamp tail'
      return -1
    self.window_calls.append((N, out_h, out_w, source, tail, bool(add)))
    if N == 0:
      return 0
    buf = T(src, (src_bytes,), 'u8').numpy()
    o = T(out, (N, out_h, out_w, 3), 'f32')
    adds = T(add, (N, 3), 'f32').numpy() if add else None
    table = (ImageDesc * N).from_address(descs)
    for n in range(N):
      d = table[n]
      ok = (d.src_offset >= 0 and d.src_offset + d.Hs * d.Ws * 3 <= src_bytes and d.crop_h > 0 and d.crop_w > 0 and
            d.crop_y >= 0 and d.crop_x >= 0 and d.crop_y + d.crop_h <= d.Hs and d.crop_x + d.crop_w <= d.Ws and
            d.resize_h > 0 and d.resize_w > 0 and d.out_y >= 0 and d.out_x >= 0 and
            d.out_y + out_h <= d.resize_h and d.out_x + out_w <= d.resize_w and 0 <= d.flip <= 2)
      if not ok:
        o[n].zero_()
        continue
      img = buf[d.src_offset:d.src_offset + d.Hs * d.Ws * 3].reshape(d.Hs, d.Ws, 3)
      win = {k: getattr(d, k) for k in ('crop_y', 'crop_x', 'crop_h', 'crop_w', 'resize_h', 'resize_w', 'out_y', 'out_x',
                                        'flip')}
      v = R.window_pixels(img, win, out_h, out_w, source, tail, None if adds is None else adds[n])
      o[n].copy_(torch.from_numpy(np.ascontiguousarray(v)))
    return 0
