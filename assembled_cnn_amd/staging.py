"""Host-to-device staging of the input path: the 16-byte slot layout of a packed batch, the grow-only host buffer a batch's
bytes are gathered in (pinned for a GPU) with its one asynchronous copy (Staging), and the upload of a descriptor table."""
from __future__ import annotations

import numpy as np
import torch


def slot_layout(nbytes, order=None):
  """16-byte padded slots back to back in `order` (default: as given) -> (int64 byte offset of every slot, total bytes):
  the src layout of asm_resize_crop_flip"""
  padded = (np.asarray(nbytes, dtype=np.int64).reshape(-1) + 15) // 16 * 16
  order = np.arange(padded.size) if order is None else np.asarray(order, dtype=np.int64)
  offsets = np.zeros(padded.size, np.int64)
  ends = np.cumsum(padded[order])
  offsets[order] = ends - padded[order]
  return offsets, int(padded.sum())


class Staging:
  """A grow-only host buffer per pin state and the event behind the last asynchronous copy out of the pinned one.  Two
  instances share nothing, so their users never wait for each other's copy."""

  def __init__(self):
    self._bufs = {}       # pin (bool) -> buffer
    self._event = None    # the last asynchronous copy out of the pinned buffer

  def fill(self, nbytes: int, arrays, offsets, pin: bool) -> torch.Tensor:
    """uint8 arrays -> the first `nbytes` of the staging buffer, each at its offset (one memcpy per array; copies if not
    contiguous).  The buffer is re-used across batches (a fresh 150 MB allocation costs more in page faults than the copy
    itself), so the previous batch must have been consumed; for the pinned one that is waited for here."""
    if pin and self._event is not None:
      self._event.synchronize()   # the previous batch's asynchronous H2D copy reads this buffer
    buf = self._bufs.get(pin)
    if buf is None or buf.numel() < nbytes:
      buf = self._bufs[pin] = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, pin_memory=pin)
    host = buf.numpy()
    for a, o in zip(arrays, offsets):
      host[int(o):int(o) + a.size] = a if a.ndim == 1 else a.reshape(-1)    # (a view of a mapped shard is slow to reshape)
    return buf[:nbytes]

  def stage_into(self, region: torch.Tensor, arrays, offsets):
    """Decoded uint8 arrays -> the staging buffer at `offsets` -> ONE host-to-device copy into `region` (a uint8 device view
    whose first byte is offset 0).  The copy is asynchronous: the next user of the pinned buffer waits for its event."""
    region.copy_(self.fill(region.numel(), arrays, offsets, region.is_cuda), non_blocking=True)
    if region.is_cuda:
      self._event = torch.cuda.Event()
      self._event.record()


_DEFAULT = Staging()      # the pixel path's (pack_batch, decode_packed, pack_device)
fill = _DEFAULT.fill
stage_into = _DEFAULT.stage_into


def upload_table(array: np.ndarray, device) -> torch.Tensor:
  """A numpy table (descriptor structs, or bytes) -> uint8 tensor on `device`.  A few KB: a blocking pageable copy."""
  return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1)).to(device, non_blocking=False)
