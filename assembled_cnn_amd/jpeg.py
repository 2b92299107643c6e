"""Host side of the device JPEG decoder (csrc/jpeg.hip).

``parse`` reads the marker segments of one file (ITU-T T.81 annex B): geometry, sampling, quantisation and Huffman tables,
the byte range of the scan and of each restart interval, and whether the file is one the device path decodes.  ``pack``
turns a batch of files into the tables ``asm_jpeg_decode`` reads, ``decode_batch`` runs it.  Everything a kernel could
trip over in a HEADER (truncated segments, table ids and sizes that disagree) is rejected here with ValueError; what can
go wrong in the entropy-coded bytes is the kernel's to detect (per-image status, decode_packed raises ValueError).

Replaces tf.image.decode_jpeg / decode_and_crop_jpeg (preprocessing/imagenet_preprocessing.py:81,92-93,296) for
dct_method '' / 'INTEGER_ACCURATE' (nets/hparams_config.py:223).
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import lib, ops
from .staging import slot_layout, stage_into, upload_table

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
                   14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39,
                   46, 53, 60, 61, 54, 47, 55, 62, 63], dtype=np.int64)
MAX_SIDE = 8192

# the device tables, as numpy sees the structs of lib.py (include/asm_hip.h)
DESC_DTYPE = np.dtype(lib.JpegDesc)
HUFF_DTYPE = np.dtype(lib.JpegHuff)
TABLES_DTYPE = np.dtype(lib.JpegTables)
INTERVAL_DTYPE = np.dtype(lib.JpegInterval)


def check_dct_method(dct_method: str):
  """tf.image.decode_jpeg's dct_method: '' and 'INTEGER_ACCURATE' are libjpeg's ISLOW, which is what the device computes."""
  if dct_method in ('', 'INTEGER_ACCURATE'):
    return
  if dct_method == 'INTEGER_FAST':
    raise NotImplementedError("dct_method 'INTEGER_FAST' (libjpeg's IFAST inverse DCT) is not implemented")
  raise ValueError('dct_method must be one of "", "INTEGER_FAST", "INTEGER_ACCURATE", got %r' % (dct_method,))


def is_encoded(entry) -> bool:
  """an entry of a batch that is an encoded file (bytes, bytearray or a 1-D uint8 array) and not a decoded image"""
  if isinstance(entry, (bytes, bytearray, memoryview)):
    return True
  return isinstance(entry, np.ndarray) and entry.ndim == 1 and entry.dtype == np.uint8


def _as_array(data) -> np.ndarray:
  if isinstance(data, np.ndarray):
    if data.ndim != 1 or data.dtype != np.uint8:
      raise ValueError('an encoded file must be bytes or a 1-D uint8 array')
    return np.ascontiguousarray(data)
  return np.frombuffer(bytes(data) if isinstance(data, memoryview) else data, dtype=np.uint8)


class JpegInfo:
  """What ``parse`` found.  ``unsupported`` is None for a file the device decodes, else the reason it does not."""
  __slots__ = ('width', 'height', 'ncomp', 'precision', 'sof', 'components', 'scan_components', 'qtables', 'huffman',
               'restart_interval', 'hs', 'vs', 'mcus_x', 'mcus_y', 'scan_begin', 'scan_end', 'intervals', 'rst',
               'unsupported')

  def __init__(self):
    self.width = self.height = self.ncomp = self.precision = 0
    self.sof = None                 # marker byte of the frame header
    self.components = []            # (id, h, v, quantisation table id) in frame order
    self.scan_components = []       # (component id, dc table id, ac table id) in scan order
    self.qtables = {}               # id -> uint16 [64], natural (row-major) order
    self.huffman = {}               # (class, id) -> (uint8 [16] counts, uint8 [n] symbols), class 0 = DC, 1 = AC
    self.restart_interval = 0
    self.hs = self.vs = 1
    self.mcus_x = self.mcus_y = 0
    self.scan_begin = self.scan_end = 0       # entropy-coded bytes: data[scan_begin:scan_end]
    self.intervals = np.zeros((0, 2), np.int64)    # [begin, end) of every restart interval, markers excluded
    self.rst = np.zeros(0, np.int64)          # m of the RSTm after each interval but the last
    self.unsupported = None

  @property
  def n_mcus(self) -> int:
    return self.mcus_x * self.mcus_y

  @property
  def n_blocks(self) -> int:
    """8x8 blocks of all components, each padded to whole MCUs"""
    return self.n_mcus * (self.hs * self.vs + 2 if self.ncomp == 3 else 1)


def _u16(a: np.ndarray, at: int) -> int:
  return (int(a[at]) << 8) | int(a[at + 1])


def parse(data) -> JpegInfo:
  """Marker segments of one file.  Raises ValueError for a JPEG whose headers are malformed; a file of a kind the device
  does not decode (and anything that is not JPEG at all) comes back with ``unsupported`` set."""
  a = _as_array(data)
  n = a.size
  info = JpegInfo()

  def unsupported(why):
    if info.unsupported is None:
      info.unsupported = why
    return info

  if n < 2 or a[0] != 0xFF or a[1] != 0xD8:
    return unsupported('not a JPEG file')
  adobe_transform = None
  at = 2
  seen_sos = False
  while True:
    if at >= n:
      raise ValueError('JPEG ends without an EOI marker' if seen_sos else 'JPEG ends before the scan')
    if a[at] != 0xFF:
      raise ValueError('expected a marker at byte %d' % at)
    while at < n and a[at] == 0xFF:       # fill bytes
      at += 1
    if at >= n:
      raise ValueError('truncated marker')
    m = int(a[at])
    at += 1
    if m == 0xD9:                         # EOI
      break
    if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7 or m == 0x00:
      raise ValueError('marker FF %02X outside a scan' % m)
    if at + 2 > n:
      raise ValueError('truncated segment length')
    seglen = _u16(a, at)
    if seglen < 2 or at + seglen > n:
      raise ValueError('segment FF %02X is truncated' % m)
    seg = a[at + 2:at + seglen]
    at += seglen
    if seen_sos:
      # anything but EOI after the first scan: more scans (or tables for them), DNL
      return unsupported('DNL marker' if m == 0xDC else 'several scans')
    if m == 0xDB:                         # DQT
      p = 0
      while p < seg.size:
        pq, tq = int(seg[p]) >> 4, int(seg[p]) & 15
        if tq > 3 or pq > 1:
          raise ValueError('DQT: bad table id / precision')
        size = 64 * (pq + 1)
        if p + 1 + size > seg.size:
          raise ValueError('DQT: table is truncated')
        raw = seg[p + 1:p + 1 + size]
        vals = raw.astype(np.uint16) if pq == 0 else (raw[0::2].astype(np.uint16) << 8) | raw[1::2]
        if pq == 1:
          unsupported('16-bit quantisation table')
        nat = np.zeros(64, np.uint16)
        nat[ZIGZAG] = vals
        info.qtables[tq] = nat
        p += 1 + size
    elif m == 0xC4:                       # DHT
      p = 0
      while p < seg.size:
        tc, th = int(seg[p]) >> 4, int(seg[p]) & 15
        if tc > 1 or th > 3:
          raise ValueError('DHT: bad table class / id')
        if p + 17 > seg.size:
          raise ValueError('DHT: table is truncated')
        bits = seg[p + 1:p + 17].copy()
        cnt = int(bits.sum())
        if cnt > 256 or p + 17 + cnt > seg.size:
          raise ValueError('DHT: symbol count and segment size disagree')
        code = 0
        for l in range(16):               # the counts must describe a prefix code (T.81 annex C)
          code = (code + int(bits[l])) << 1
          if code > (2 << (l + 1)):
            raise ValueError('DHT: code lengths overflow')
        info.huffman[(tc, th)] = (bits, seg[p + 17:p + 17 + cnt].copy())
        p += 17 + cnt
    elif m in (0xC0, 0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):     # SOFn
      if info.sof is not None:
        raise ValueError('two frame headers')
      if seg.size < 6:
        raise ValueError('SOF: truncated')
      info.sof = m
      info.precision, info.height, info.width, info.ncomp = int(seg[0]), _u16(seg, 1), _u16(seg, 3), int(seg[5])
      if seg.size != 6 + 3 * info.ncomp or info.ncomp == 0:
        raise ValueError('SOF: component count and segment size disagree')
      if info.width == 0:
        raise ValueError('SOF: zero width')
      for k in range(info.ncomp):
        cid, hv, tq = int(seg[6 + 3 * k]), int(seg[7 + 3 * k]), int(seg[8 + 3 * k])
        if not (1 <= hv >> 4 <= 4 and 1 <= (hv & 15) <= 4) or tq > 3:
          raise ValueError('SOF: bad sampling factors / table id')
        info.components.append((cid, hv >> 4, hv & 15, tq))
      if len(set(c[0] for c in info.components)) != info.ncomp:
        raise ValueError('SOF: duplicate component id')
      if m == 0xC2:
        unsupported('progressive (SOF2)')
      elif m not in (0xC0, 0xC1):
        unsupported('arithmetic coding' if m >= 0xC9 else 'lossless / hierarchical frame (SOF%d)' % (m - 0xC0))
      if info.precision != 8:
        unsupported('%d-bit samples' % info.precision)
    elif m == 0xCC:                       # DAC
      unsupported('arithmetic coding')
    elif m == 0xDD:                       # DRI
      if seg.size != 2:
        raise ValueError('DRI: bad length')
      info.restart_interval = _u16(seg, 0)
    elif m == 0xDC:
      unsupported('DNL marker')
    elif m == 0xEE and seg.size >= 12 and bytes(seg[:5]) == b'Adobe':
      adobe_transform = int(seg[11])
    elif m == 0xDA:                       # SOS
      if info.sof is None:
        raise ValueError('SOS before the frame header')
      if seg.size < 1 or seg.size != 4 + 2 * int(seg[0]):
        raise ValueError('SOS: component count and segment size disagree')
      ns = int(seg[0])
      ids = [c[0] for c in info.components]
      for k in range(ns):
        cs, t = int(seg[1 + 2 * k]), int(seg[2 + 2 * k])
        if cs not in ids or (t >> 4) > 3 or (t & 15) > 3:
          raise ValueError('SOS: unknown component / bad table id')
        info.scan_components.append((cs, t >> 4, t & 15))
      seen_sos = True
      info.scan_begin = at
      # the scan ends at the first FF that is followed by neither 00 (a stuffed FF), FF (fill) nor RSTm
      body = a[at:]
      ff = np.flatnonzero(body[:-1] == 0xFF) if body.size > 1 else np.zeros(0, np.int64)
      nxt = body[ff + 1]
      is_rst = (nxt >= 0xD0) & (nxt <= 0xD7)
      ends = ff[(nxt != 0) & (nxt != 0xFF) & ~is_rst]
      if ends.size == 0:
        raise ValueError('JPEG ends without an EOI marker')
      end = int(ends[0])
      while end > 0 and body[end - 1] == 0xFF:       # fill bytes in front of the marker
        end -= 1
      info.scan_end = at + end
      r = ff[is_rst & (ff < end)]
      info.rst = (body[r + 1].astype(np.int64) - 0xD0)
      begins = np.concatenate([[0], r + 2]) + at
      stops = np.concatenate([r, [end]]) + at
      info.intervals = np.stack([begins, stops], axis=1).astype(np.int64)
      at = int(ends[0]) + at
    # APPn, COM and the reserved markers carry nothing the decode needs

  if not seen_sos:
    raise ValueError('JPEG has no scan')
  # ---- classification -------------------------------------------------------------------------------
  if info.unsupported is not None:
    return info
  if info.height == 0:
    return unsupported('DNL marker')
  if info.width > MAX_SIDE or info.height > MAX_SIDE:
    return unsupported('larger than %d x %d' % (MAX_SIDE, MAX_SIDE))
  if info.ncomp == 4:
    return unsupported('4 components / CMYK')
  if info.ncomp not in (1, 3):
    return unsupported('%d components' % info.ncomp)
  if len(info.scan_components) != info.ncomp:
    return unsupported('several scans')
  if [s[0] for s in info.scan_components] != [c[0] for c in info.components]:
    return unsupported('scan components out of frame order')
  if info.ncomp == 3:
    if adobe_transform is not None and adobe_transform != 1:
      return unsupported('Adobe marker with transform %d' % adobe_transform)
    if adobe_transform is None and [c[0] for c in info.components] == [ord('R'), ord('G'), ord('B')]:
      return unsupported('RGB component ids')
    (_, h0, v0, _), (_, h1, v1, _), (_, h2, v2, _) = info.components
    if (h1, v1, h2, v2) != (1, 1, 1, 1) or (h0, v0) not in ((1, 1), (2, 1), (2, 2)):
      return unsupported('sampling %dx%d,%dx%d,%dx%d' % (h0, v0, h1, v1, h2, v2))
    info.hs, info.vs = h0, v0
  for (_, _, _, tq) in info.components:
    if tq not in info.qtables:
      raise ValueError('quantisation table %d is not defined' % tq)
  for (_, td, ta) in info.scan_components:
    if (0, td) not in info.huffman or (1, ta) not in info.huffman:
      raise ValueError('Huffman table %d/%d is not defined' % (td, ta))
  if len(set(s[1] for s in info.scan_components)) > 2 or len(set(s[2] for s in info.scan_components)) > 2:
    return unsupported('more than two DC or AC Huffman tables')
  info.mcus_x = -(-info.width // (8 * info.hs))
  info.mcus_y = -(-info.height // (8 * info.vs))
  return info


class Packed:
  """A batch ready for the device.  Entry k of the batch is either row ``dev_row[k]`` of the device tables or, when the
  file is of an unsupported kind, the decoded array ``fallback[k]``."""

  def __init__(self):
    self.files = np.zeros(16, np.uint8)
    self.descs = np.zeros(0, DESC_DTYPE)
    self.tables = np.zeros(0, TABLES_DTYPE)
    self.intervals = np.zeros(0, INTERVAL_DTYPE)
    self.sizes = []                 # (height, width) of every entry
    self.offsets = np.zeros(0, np.int64)      # byte offset of every entry's [H][W][3] pixels in the output buffer
    self.total_bytes = 16
    self.host_begin = 0             # the slots of the already decoded entries are [host_begin, total_bytes)
    self.total_blocks = self.max_blocks = self.max_pixels = 0
    self.dev_index = []             # batch index of each device row
    self.fallback = {}              # batch index -> decoded uint8 [H, W, 3]


def _check_decoded(arr, k) -> np.ndarray:
  arr = np.asarray(arr)
  if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
    raise ValueError('entry %d: a decoded image must be uint8 [height, width, 3]' % k)
  return arr


def pack(files: Sequence, fallback: Optional[Callable] = None, infos: Optional[List[JpegInfo]] = None) -> Packed:
  """Batch of entries -> the tables of asm_jpeg_decode (numpy, host).  An entry is an encoded file or an already decoded
  uint8 [H, W, 3] array (which only gets a slot in the output).  Files of an unsupported kind go through ``fallback(bytes)
  -> uint8 [H, W, 3]``; without one the call raises NotImplementedError naming the reason and the index."""
  pk = Packed()
  n = len(files)
  if infos is None:
    infos = [parse(f) if is_encoded(f) else None for f in files]
  arrays = [None] * n
  for k, (f, info) in enumerate(zip(files, infos)):
    if info is None:
      pk.fallback[k] = _check_decoded(f, k)
    elif info.unsupported is not None:
      if fallback is None:
        raise NotImplementedError('entry %d: %s is not decoded on the device and no fallback was given'
                                  % (k, info.unsupported))
      pk.fallback[k] = _check_decoded(fallback(bytes(f) if not isinstance(f, np.ndarray) else f.tobytes()), k)
    else:
      arrays[k] = _as_array(f)
      pk.dev_index.append(k)
  nd = len(pk.dev_index)
  pk.descs = np.zeros(nd, DESC_DTYPE)
  pk.tables = np.zeros(nd, TABLES_DTYPE)
  # output slots, 16-byte aligned (the src layout of asm_resize_crop_flip): the device-decoded entries first, then the
  # already decoded ones back to back, so that those travel in one host-to-device copy
  pk.sizes = [(infos[k].height, infos[k].width) if k not in pk.fallback else pk.fallback[k].shape[:2] for k in range(n)]
  hosted = sorted(pk.fallback)
  pk.offsets, total = slot_layout([h * w * 3 for h, w in pk.sizes], pk.dev_index + hosted)
  pk.host_begin = int(pk.offsets[hosted[0]]) if hosted else total
  pk.total_bytes = max(total, 16)
  scan_at, blocks_at, rows = 0, 0, []
  chunks = []
  for row, k in enumerate(pk.dev_index):
    info, a = infos[k], arrays[k]
    d = pk.descs[row]
    scan = a[info.scan_begin:info.scan_end]
    chunks.append((scan_at, scan))
    d['scan_offset'], d['scan_bytes'] = scan_at, scan.size
    d['coef_offset'] = d['plane_offset'] = blocks_at * 64
    d['dst_offset'] = pk.offsets[k]
    d['width'], d['height'], d['ncomp'] = info.width, info.height, info.ncomp
    d['hs'], d['vs'], d['mcus_x'], d['mcus_y'] = info.hs, info.vs, info.mcus_x, info.mcus_y
    d['restart_interval'] = info.restart_interval
    d['first_interval'], d['n_intervals'] = sum(r.size for r in rows), len(info.intervals)
    # Huffman slots: the (at most two) tables of each class the scan names, in order of first use
    dc_ids, ac_ids = [], []
    for c, ((_, _, _, tq), (_, td, ta)) in enumerate(zip(info.components, info.scan_components)):
      if td not in dc_ids:
        dc_ids.append(td)
      if ta not in ac_ids:
        ac_ids.append(ta)
      d['qsel'][c], d['dcsel'][c], d['acsel'][c] = tq, dc_ids.index(td), ac_ids.index(ta)
    t = pk.tables[row]
    for tq, q in info.qtables.items():
      t['quant'][tq] = q
    for cls, name, ids in ((0, 'dc', dc_ids), (1, 'ac', ac_ids)):
      for slot, th in enumerate(ids):
        bits, vals = info.huffman[(cls, th)]
        t[name][slot]['bits'] = bits
        t[name][slot]['vals'][:vals.size] = vals
    iv = np.zeros(len(info.intervals), INTERVAL_DTYPE)
    ri, total = info.restart_interval, info.n_mcus
    idx = np.arange(len(iv), dtype=np.int64)
    iv['image'] = row
    iv['first_mcu'] = np.minimum(idx * ri, 2 ** 31 - 1) if ri else 0
    iv['n_mcus'] = np.clip(total - idx * ri, -2 ** 31, ri) if ri else total
    iv['rst'] = np.concatenate([info.rst, [-1]])
    iv['byte_begin'] = info.intervals[:, 0] - info.scan_begin + scan_at
    iv['byte_end'] = info.intervals[:, 1] - info.scan_begin + scan_at
    rows.append(iv)
    scan_at += (scan.size + 15) // 16 * 16
    blocks_at += info.n_blocks
    pk.max_blocks = max(pk.max_blocks, info.n_blocks)
    pk.max_pixels = max(pk.max_pixels, info.width * info.height)
  pk.files = np.zeros(max(scan_at, 16), np.uint8)
  for o, scan in chunks:
    pk.files[o:o + scan.size] = scan
  pk.intervals = np.concatenate(rows) if rows else np.zeros(0, INTERVAL_DTYPE)
  pk.total_blocks = blocks_at
  return pk


def decode_packed(pk: Packed, device, stages: int = 3, check: bool = True, return_workspace: bool = False):
  """Run the device decode of a packed batch and copy the already decoded entries into their slots (one staged copy).
  Returns (uint8 device buffer of pk.total_bytes, int32 status per device row), plus ops.jpeg_decode's workspace
  (raw coefficients first) when return_workspace.  check: wait for the decode, return the status on the host and raise
  ValueError naming the entries whose entropy-coded data is corrupt."""
  dev = torch.device(device)
  dst = torch.empty(pk.total_bytes, dtype=torch.uint8, device=dev)
  status = ws = None
  if pk.dev_index:
    status, ws = ops.jpeg_decode(*(upload_table(t, dev) for t in (pk.files, pk.descs, pk.tables, pk.intervals)),
                                 len(pk.dev_index), len(pk.intervals), pk.total_blocks, pk.max_blocks, pk.max_pixels, dst,
                                 stages=stages)
    if check:
      status = status.cpu()
      bad = torch.nonzero(status).reshape(-1).tolist()
      if bad:
        raise ValueError('jpeg_decode: corrupt entropy-coded data in entries %s (status %s)' % (
            [pk.dev_index[b] for b in bad], [int(status[b]) for b in bad]))
  if pk.fallback:
    keys = sorted(pk.fallback)
    stage_into(dst[pk.host_begin:], [pk.fallback[k] for k in keys], [pk.offsets[k] - pk.host_begin for k in keys])
  return (dst, status, ws) if return_workspace else (dst, status)


def decode_batch(files: Sequence, device, fallback: Optional[Callable] = None, dct_method: str = ''):
  """Encoded files -> (packed uint8 device buffer, byte offsets, [(height, width)]): image k is
  buffer[offsets[k] : offsets[k] + 3 * h * w] viewed as [h, w, 3].  Raises ValueError naming the files whose
  entropy-coded data is corrupt, NotImplementedError for an unsupported kind without ``fallback``."""
  check_dct_method(dct_method)
  pk = pack(files, fallback)
  dst = decode_packed(pk, device)[0]
  return dst, pk.offsets, pk.sizes
