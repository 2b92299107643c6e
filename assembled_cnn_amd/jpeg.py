"""Host side of the device JPEG decoder (csrc/jpeg.hip).

``parse`` reads the marker segments of one file (ITU-T T.81 annex B): geometry, sampling, quantisation and Huffman tables,
the byte range of the scan and of each restart interval, and whether the file is one the device path decodes.  ``pack``
turns a batch of files into the tables ``asm_jpeg_decode`` reads, ``decode_batch`` runs it.  ``pack_device`` (opt-in)
makes the sequential rows' tables on the device instead, from files that lie there: asm_jpeg_parse, one read-back of the
head rows, ``layout_heads``, asm_jpeg_parse_fill; only the files the device does not take come back to ``parse``.
With ``progressive=True`` (opt-in) a progressive file is read scan by scan and becomes a row of a second
group of tables, the ones ``asm_jpeg_decode_progressive`` reads.  Everything a kernel could
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
MAX_SCANS = 256         # of one progressive file: the device walks them one after another
ENTROPY_MODES = ('sequential', 'parallel')
PARSE_MODES = ('host', 'device')        # who reads the headers: parse / pack here, or asm_jpeg_parse (pack_device)
# raw file bytes per segment of the segment-parallel entropy stage (entropy='parallel'); the best of the sweep in
# profiles/jpeg_decode.md
DEFAULT_SEGMENT_BYTES = 128

# the device tables, as numpy sees the structs of lib.py (include/asm_hip.h)
DESC_DTYPE = np.dtype(lib.JpegDesc)
HUFF_DTYPE = np.dtype(lib.JpegHuff)
TABLES_DTYPE = np.dtype(lib.JpegTables)
INTERVAL_DTYPE = np.dtype(lib.JpegInterval)
SCAN_DTYPE = np.dtype(lib.JpegScan)
HEAD_DTYPE = np.dtype(lib.JpegHead)
PLACE_DTYPE = np.dtype(lib.JpegPlace)
SPAN_DTYPE = np.dtype(lib.SpanDesc)


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


def mcu_grid(width, height, ncomp, hs, vs):
  """(MCUs across, MCUs down, 8x8 blocks of all components, each padded to whole MCUs) of an image with luma sampling
  hs x vs; Python ints or numpy integer arrays alike"""
  mcus_x, mcus_y = -(-width // (8 * hs)), -(-height // (8 * vs))
  return mcus_x, mcus_y, mcus_x * mcus_y * ((ncomp == 3) * (hs * vs + 1) + 1)


class ScanInfo:
  """One scan of a progressive file, as ``parse(..., progressive=True)`` found it."""
  __slots__ = ('components', 'ss', 'se', 'ah', 'al', 'huffman', 'restart_interval', 'begin', 'end', 'intervals', 'rst')

  def __init__(self):
    self.components = []            # indices in frame order
    self.ss = self.se = self.ah = self.al = 0
    self.huffman = []               # per scan component: ((bits, vals) of its DC table, of its AC table) at this SOS, or None
    self.restart_interval = 0       # DRI in force at this SOS, counting the scan's own MCUs
    self.begin = self.end = 0       # entropy-coded bytes: data[begin:end]
    self.intervals = np.zeros((0, 2), np.int64)
    self.rst = np.zeros(0, np.int64)

  def n_mcus(self, info) -> int:
    """MCUs of the scan: the image's padded MCU grid for an interleaved scan, the component's TRUE block grid for a scan
    of one component"""
    if len(self.components) > 1:
      return info.n_mcus
    _, h, v, _ = info.components[self.components[0]]
    if info.ncomp == 1:
      h = v = 1
    w, ht = -(-info.width * h // info.hs), -(-info.height * v // info.vs)
    return -(-w // 8) * -(-ht // 8)


class JpegInfo:
  """What ``parse`` found.  ``unsupported`` is None for a file the device decodes, else the reason it does not."""
  __slots__ = ('width', 'height', 'ncomp', 'precision', 'sof', 'components', 'scan_components', 'qtables', 'huffman',
               'restart_interval', 'hs', 'vs', 'mcus_x', 'mcus_y', 'scan_begin', 'scan_end', 'intervals', 'rst',
               'unsupported', 'scans')

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
    self.scans = None               # [ScanInfo] in file order: a progressive file parsed with progressive=True

  @property
  def progressive(self) -> bool:
    """a progressive file the device decodes (its row goes to asm_jpeg_decode_progressive)"""
    return self.scans is not None and self.unsupported is None

  @property
  def n_mcus(self) -> int:
    return self.mcus_x * self.mcus_y

  @property
  def n_blocks(self) -> int:
    """8x8 blocks of all components, each padded to whole MCUs"""
    return mcu_grid(self.width, self.height, self.ncomp, self.hs, self.vs)[2]


def _u16(a: np.ndarray, at: int) -> int:
  return (int(a[at]) << 8) | int(a[at + 1])


def _scan_extent(a: np.ndarray, at: int, marks):
  """The entropy-coded bytes that start at a[at]: (end, intervals [k, 2], rst [k - 1], position of the marker that ends
  them).  marks: the (FF positions followed by RSTm, by any other marker) of the whole file, found once.  The scan ends at
  the first FF that is followed by neither 00 (a stuffed FF), FF (fill) nor RSTm."""
  rst_ff, end_ff = marks
  e = int(np.searchsorted(end_ff, at))
  if e >= end_ff.size:
    raise ValueError('JPEG ends without an EOI marker')
  marker = end = int(end_ff[e])
  while end > at and a[end - 1] == 0xFF:       # fill bytes in front of the marker
    end -= 1
  r = rst_ff[np.searchsorted(rst_ff, at):np.searchsorted(rst_ff, end)]
  rst = a[r + 1].astype(np.int64) - 0xD0
  begins = np.concatenate([[at], r + 2])
  stops = np.concatenate([r, [end]])
  return end, np.stack([begins, stops], axis=1).astype(np.int64), rst, marker


def _markers(a: np.ndarray):
  ff = np.flatnonzero(a[:-1] == 0xFF) if a.size > 1 else np.zeros(0, np.int64)
  nxt = a[ff + 1]
  is_rst = (nxt >= 0xD0) & (nxt <= 0xD7)
  return ff[is_rst], ff[(nxt != 0) & (nxt != 0xFF) & ~is_rst]


def parse(data, progressive: bool = False) -> JpegInfo:
  """Marker segments of one file.  Raises ValueError for a JPEG whose headers are malformed; a file of a kind the device
  does not decode (and anything that is not JPEG at all) comes back with ``unsupported`` set.  progressive: read a
  progressive (SOF2) file scan by scan into ``info.scans`` and classify it by the rules of DESIGN.md 1.2; without the
  flag such a file is unsupported, and any other file is read the same either way."""
  a = _as_array(data)
  n = a.size
  info = JpegInfo()
  marks = None

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
    if seen_sos and (info.scans is None or info.unsupported is not None):
      # anything but EOI after the first scan: more scans (or tables for them), DNL
      return unsupported('DNL marker' if m == 0xDC else 'several scans')
    if seen_sos and m == 0xDB:
      return unsupported('quantisation tables redefined between scans')
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
        if progressive:
          info.scans = []
        else:
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
      named = []
      for k in range(ns):
        cs, t = int(seg[1 + 2 * k]), int(seg[2 + 2 * k])
        if cs not in ids or (t >> 4) > 3 or (t & 15) > 3:
          raise ValueError('SOS: unknown component / bad table id')
        named.append((cs, t >> 4, t & 15))
      if marks is None:
        marks = _markers(a)
      end, intervals, rst, marker = _scan_extent(a, at, marks)
      if not seen_sos:
        info.scan_components = named
        info.scan_begin, info.scan_end, info.intervals, info.rst = at, end, intervals, rst
      seen_sos = True
      if info.scans is not None and info.unsupported is None:
        if len(info.scans) == MAX_SCANS:
          return unsupported('more than %d scans' % MAX_SCANS)
        sc = ScanInfo()
        sc.components = [ids.index(cs) for cs, _, _ in named]
        sc.ss, sc.se, sc.ah, sc.al = int(seg[-3]), int(seg[-2]), int(seg[-1]) >> 4, int(seg[-1]) & 15
        sc.huffman = [(info.huffman.get((0, td)), info.huffman.get((1, ta))) for _, td, ta in named]
        sc.restart_interval = info.restart_interval
        sc.begin, sc.end, sc.intervals, sc.rst = at, end, intervals, rst
        info.scans.append(sc)
      at = marker
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
  if info.scans is None:
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
  info.mcus_x, info.mcus_y, _ = mcu_grid(info.width, info.height, info.ncomp, info.hs, info.vs)
  if info.scans is not None:
    why = _check_progression(info)
    return unsupported(why) if why else info
  for (_, td, ta) in info.scan_components:
    if (0, td) not in info.huffman or (1, ta) not in info.huffman:
      raise ValueError('Huffman table %d/%d is not defined' % (td, ta))
  if len(set(s[1] for s in info.scan_components)) > 2 or len(set(s[2] for s in info.scan_components)) > 2:
    return unsupported('more than two DC or AC Huffman tables')
  return info


def _check_progression(info: JpegInfo) -> Optional[str]:
  """The scan script of a progressive file (T.81 G.1.1, libjpeg's jdphuff.c start_pass): None if the device decodes it,
  else why not.  Where libjpeg warns and carries on, this refuses.  Raises ValueError for a Huffman table a scan needs
  and the file never defined."""
  coef_bits = np.full((info.ncomp, 64), -1, np.int64)
  for k, sc in enumerate(info.scans):
    nc = len(sc.components)
    if sc.ss == 0:
      if sc.se != 0:
        return 'progressive scan %d mixes DC and AC coefficients (Ss 0, Se %d)' % (k, sc.se)
      if any(b <= a for a, b in zip(sc.components, sc.components[1:])):
        return 'progressive scan %d: components out of frame order' % k
    else:
      if nc != 1:
        return 'progressive AC scan %d names %d components' % (k, nc)
      if not sc.ss <= sc.se <= 63:
        return 'progressive scan %d: bad spectral band %d..%d' % (k, sc.ss, sc.se)
    if sc.al > 13 or (sc.ah != 0 and sc.al != sc.ah - 1):
      return 'progressive scan %d: bad successive approximation Ah %d, Al %d' % (k, sc.ah, sc.al)
    for c in sc.components:
      if sc.ss > 0 and coef_bits[c, 0] < 0:
        return 'progressive AC scan %d before the DC scan of its component' % k
      band = coef_bits[c, sc.ss:sc.se + 1]
      if np.any(np.where(band < 0, 0, band) != sc.ah):
        return 'progressive scan %d: refinement out of sequence (Ah %d)' % (k, sc.ah)
      band[:] = sc.al
    for (dc, ac) in sc.huffman:
      if (sc.ss == 0 and sc.ah == 0 and dc is None) or (sc.ss > 0 and ac is None):
        raise ValueError('Huffman table of progressive scan %d is not defined' % k)
  if np.any(coef_bits != 0):
    return 'progressive file with incomplete scans'
  return None


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
    # pack(..., segment_bytes=...): asm_jpeg_decode_parallel's table, one entry per row of `intervals`
    self.segment_bytes = None
    self.segment_first = np.zeros(0, np.int32)
    self.total_segments = 0
    self.dev_index = []             # batch index of each device row
    self.fallback = {}              # batch index -> decoded uint8 [H, W, 3]
    # the progressive rows (pack(..., progressive=True)), tables of their own for asm_jpeg_decode_progressive; the fields
    # above describe the sequential rows alone
    self.prog_index = []            # batch index of each progressive row
    self.prog_files = np.zeros(16, np.uint8)
    self.prog_descs = np.zeros(0, DESC_DTYPE)
    self.prog_tables = np.zeros(0, TABLES_DTYPE)
    self.prog_scans = np.zeros(0, SCAN_DTYPE)
    self.prog_huff = np.zeros(0, HUFF_DTYPE)
    self.prog_intervals = np.zeros(0, INTERVAL_DTYPE)
    self.prog_total_blocks = self.prog_max_blocks = self.prog_max_pixels = 0
    # pack_device: the sequential rows' tables as device tensors (files, descs, tables, intervals, segment_first) in place of
    # the five numpy fields above, their interval count, and asm_jpeg_parse_fill's status word per row
    self.dev_tables = None
    self.n_intervals = 0
    self.fill_status = None


def _check_decoded(arr, k) -> np.ndarray:
  arr = np.asarray(arr)
  if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
    raise ValueError('entry %d: a decoded image must be uint8 [height, width, 3]' % k)
  return arr


def _interval_rows(image, intervals, rst, restart_interval, n_mcus, byte_shift) -> np.ndarray:
  """asm_jpeg_interval rows of one scan: interval k holds MCUs [k * restart_interval, ...) of the scan's n_mcus"""
  iv = np.zeros(len(intervals), INTERVAL_DTYPE)
  idx = np.arange(len(iv), dtype=np.int64)
  iv['image'] = image
  iv['first_mcu'] = np.minimum(idx * restart_interval, 2 ** 31 - 1) if restart_interval else 0
  iv['n_mcus'] = np.clip(n_mcus - idx * restart_interval, -2 ** 31, restart_interval) if restart_interval else n_mcus
  iv['rst'] = np.concatenate([rst, [-1]])
  iv['byte_begin'] = intervals[:, 0] + byte_shift
  iv['byte_end'] = intervals[:, 1] + byte_shift
  return iv


def _byte_pool(chunks):
  """(one zeroed uint8 array of at least 16 bytes holding the chunks at 16-byte-aligned offsets, those offsets)"""
  sizes = [(c.size + 15) // 16 * 16 for c in chunks]
  offsets = [int(o) for o in np.cumsum([0] + sizes)]
  pool = np.zeros(max(offsets[-1], 16), np.uint8)
  for o, c in zip(offsets, chunks):
    pool[o:o + c.size] = c
  return pool, offsets[:-1]


def _fill_rows(pk: Packed, group, index, infos, bodies):
  """What a sequential (group '') and a progressive group ('prog_') fill alike for its images `index` (batch indices in row
  order, their bytes in `bodies`): the byte pool and, per row, the offsets into it, into coefficients, planes and dst, the
  geometry, qsel and the quantisation tables.  Sets the group's files, descs, tables, total_blocks, max_blocks and
  max_pixels in pk and returns each body's offset in the pool."""
  descs = np.zeros(len(index), DESC_DTYPE)
  tables = np.zeros(len(index), TABLES_DTYPE)
  pool, offsets = _byte_pool(bodies)
  blocks_at = max_blocks = max_pixels = 0
  for row, k in enumerate(index):
    info, d, n_blocks = infos[k], descs[row], infos[k].n_blocks
    d['scan_offset'], d['scan_bytes'] = offsets[row], bodies[row].size
    d['coef_offset'] = d['plane_offset'] = blocks_at * 64
    d['dst_offset'] = pk.offsets[k]
    d['width'], d['height'], d['ncomp'] = info.width, info.height, info.ncomp
    d['hs'], d['vs'], d['mcus_x'], d['mcus_y'] = info.hs, info.vs, info.mcus_x, info.mcus_y
    for c, (_, _, _, tq) in enumerate(info.components):
      d['qsel'][c] = tq
    for tq, q in info.qtables.items():
      tables[row]['quant'][tq] = q
    blocks_at += n_blocks
    max_blocks = max(max_blocks, n_blocks)
    max_pixels = max(max_pixels, info.width * info.height)
  for field, value in (('files', pool), ('descs', descs), ('tables', tables), ('total_blocks', blocks_at),
                       ('max_blocks', max_blocks), ('max_pixels', max_pixels)):
    setattr(pk, group + field, value)
  return offsets


def _pack_sequential(pk: Packed, files, infos):
  """The sequential rows' tables: per image one descriptor, its (at most two per class) Huffman tables and its rows of
  the interval table; with pk.segment_bytes also the segment table of asm_jpeg_decode_parallel."""
  bodies = [_as_array(files[k])[infos[k].scan_begin:infos[k].scan_end] for k in pk.dev_index]
  offsets = _fill_rows(pk, '', pk.dev_index, infos, bodies)
  n_iv, iv_rows = 0, []
  for row, k in enumerate(pk.dev_index):
    info, d, t = infos[k], pk.descs[row], pk.tables[row]
    d['restart_interval'] = info.restart_interval
    d['first_interval'], d['n_intervals'] = n_iv, len(info.intervals)
    # Huffman slots: the (at most two) tables of each class the scan names, in order of first use
    dc_ids, ac_ids = [], []
    for c, (_, td, ta) in enumerate(info.scan_components):
      if td not in dc_ids:
        dc_ids.append(td)
      if ta not in ac_ids:
        ac_ids.append(ta)
      d['dcsel'][c], d['acsel'][c] = dc_ids.index(td), ac_ids.index(ta)
    for cls, name, ids in ((0, 'dc', dc_ids), (1, 'ac', ac_ids)):
      for slot, th in enumerate(ids):
        bits, vals = info.huffman[(cls, th)]
        t[name][slot]['bits'] = bits
        t[name][slot]['vals'][:vals.size] = vals
    iv_rows.append(_interval_rows(row, info.intervals, info.rst, info.restart_interval, info.n_mcus,
                                  offsets[row] - info.scan_begin))
    n_iv += len(info.intervals)
  pk.intervals = np.concatenate(iv_rows) if iv_rows else np.zeros(0, INTERVAL_DTYPE)
  if pk.segment_bytes is not None:
    pk.segment_first, pk.total_segments = segment_table(pk.intervals, pk.segment_bytes)


def _pack_progressive(pk: Packed, files, infos):
  """The progressive rows' tables: per image one descriptor (its first_interval / n_intervals name its rows of the scan
  table), per scan one row, one pool entry per Huffman table a scan reads, and the scans' interval rows."""
  # every scan of the image, the marker segments between them included
  bodies = [_as_array(files[k])[infos[k].scans[0].begin:infos[k].scans[-1].end] for k in pk.prog_index]
  offsets = _fill_rows(pk, 'prog_', pk.prog_index, infos, bodies)
  n_scans, n_iv = 0, 0
  scan_rows, huffs, iv_rows = [], [], []
  for row, k in enumerate(pk.prog_index):
    info = infos[k]
    shift = offsets[row] - info.scans[0].begin
    pk.prog_descs[row]['first_interval'], pk.prog_descs[row]['n_intervals'] = n_scans, len(info.scans)
    rows = np.zeros(len(info.scans), SCAN_DTYPE)
    for j, sc in enumerate(info.scans):
      r = rows[j]
      r['image'], r['ncomp'] = row, len(sc.components)
      r['comp'][:len(sc.components)] = sc.components
      r['ss'], r['se'], r['ah'], r['al'] = sc.ss, sc.se, sc.ah, sc.al
      r['huff'] = -1
      for i, (dc, ac) in enumerate(sc.huffman):
        table = ac if sc.ss > 0 else dc if sc.ah == 0 else None
        if table is not None:
          h = np.zeros((), HUFF_DTYPE)
          h['bits'] = table[0]
          h['vals'][:table[1].size] = table[1]
          r['huff'][i] = len(huffs)
          huffs.append(h)
      r['restart_interval'] = sc.restart_interval
      r['first_interval'], r['n_intervals'] = n_iv, len(sc.intervals)
      r['byte_begin'], r['byte_end'] = sc.begin + shift, sc.end + shift
      iv_rows.append(_interval_rows(row, sc.intervals, sc.rst, sc.restart_interval, sc.n_mcus(info), shift))
      n_iv += len(sc.intervals)
    scan_rows.append(rows)
    n_scans += len(rows)
  pk.prog_scans = np.concatenate(scan_rows) if scan_rows else np.zeros(0, SCAN_DTYPE)
  pk.prog_huff = np.array(huffs, HUFF_DTYPE) if huffs else np.zeros(0, HUFF_DTYPE)
  pk.prog_intervals = np.concatenate(iv_rows) if iv_rows else np.zeros(0, INTERVAL_DTYPE)


def check_segment_bytes(segment_bytes: int) -> int:
  if int(segment_bytes) != segment_bytes or not 16 <= segment_bytes <= 65536 or segment_bytes % 16:
    raise ValueError('segment_bytes must be a multiple of 16 in 16..65536, got %r' % (segment_bytes,))
  return int(segment_bytes)


def check_modes(entropy: str, segment_bytes, parse: str, resident, prefix: str = '') -> Optional[int]:
  """The mode arguments of decode_batch (prefix '') and preprocess_batch (prefix 'jpeg_', as its arguments are called):
  ValueError for a bad one, else the segment_bytes to pack with -- DEFAULT_SEGMENT_BYTES for entropy='parallel' when none
  was given.  Its range is pack's to check."""
  if entropy not in ENTROPY_MODES:
    raise ValueError('%sentropy must be one of %s, got %r' % (prefix, ENTROPY_MODES, entropy))
  if parse not in PARSE_MODES:
    raise ValueError('%sparse must be one of %s, got %r' % (prefix, PARSE_MODES, parse))
  if resident is not None and parse != 'device':
    raise ValueError("resident needs parse='device'")
  if segment_bytes is not None and entropy != 'parallel':
    raise ValueError("segment_bytes needs entropy='parallel'")
  return DEFAULT_SEGMENT_BYTES if segment_bytes is None and entropy == 'parallel' else segment_bytes


def segment_table(intervals: np.ndarray, segment_bytes: int):
  """(int32 first segment of every interval row, total segments): an interval of b bytes has max(1, ceil(b /
  segment_bytes)) segments and the rows follow each other without a gap (include/asm_hip.h, asm_jpeg_decode_parallel)"""
  size = intervals['byte_end'].astype(np.int64) - intervals['byte_begin']
  counts = np.maximum(-(-size // segment_bytes), 1)
  ends = np.cumsum(counts)
  total = int(ends[-1]) if len(ends) else 0
  if total >= 2 ** 30:
    raise ValueError('segment_bytes = %d gives %d segments, more than one call takes' % (segment_bytes, total))
  return (ends - counts).astype(np.int32), total


def _route(pk: Packed, files, infos, fallback):
  """Where every entry of a batch goes by what the header reader found (`infos`; None for a decoded array): a sequential
  row (pk.dev_index), a progressive row (pk.prog_index) or a decoded array in pk.fallback -- given, or made by
  ``fallback`` from a file of an unsupported kind (NotImplementedError without one)."""
  for k, (f, info) in enumerate(zip(files, infos)):
    if info is None:
      pk.fallback[k] = _check_decoded(f, k)
    elif info.unsupported is not None:
      if fallback is None:
        raise NotImplementedError('entry %d: %s is not decoded on the device and no fallback was given'
                                  % (k, info.unsupported))
      pk.fallback[k] = _check_decoded(fallback(bytes(f) if not isinstance(f, np.ndarray) else f.tobytes()), k)
    else:
      (pk.prog_index if info.progressive else pk.dev_index).append(k)


class _HostHeaders:
  """The header reader of ``pack``: parse, slot_layout, _pack_sequential."""

  def __init__(self, infos):
    self.infos = infos

  def read(self, files, progressive, segment_bytes):
    if self.infos is not None:
      return self.infos
    return [parse(f, progressive) if is_encoded(f) else None for f in files]

  def layout(self, pk, tail):
    return slot_layout([h * w * 3 for h, w in pk.sizes], pk.dev_index + tail)

  sequential = staticmethod(_pack_sequential)


def _pack(reader, files, fallback, progressive, segment_bytes) -> Packed:
  """What pack and pack_device share.  `reader` reads the headers (-> per entry a JpegInfo, the _HeadInfo of a file whose
  headers stay on the device, or None for a decoded array), lays out the output slots (-> offsets, total bytes) and makes
  the sequential rows' tables."""
  pk = Packed()
  if segment_bytes is not None:
    pk.segment_bytes = check_segment_bytes(segment_bytes)
  infos = reader.read(files, progressive, pk.segment_bytes)
  _route(pk, files, infos, fallback)
  # output slots, 16-byte aligned (the src layout of asm_resize_crop_flip): the device-decoded entries first (sequential
  # rows, then progressive rows), then the already decoded ones back to back, so that those travel in one host-to-device
  # copy
  pk.sizes = [(infos[k].height, infos[k].width) if k not in pk.fallback else pk.fallback[k].shape[:2]
              for k in range(len(files))]
  hosted = sorted(pk.fallback)
  pk.offsets, total = reader.layout(pk, pk.prog_index + hosted)
  pk.host_begin = int(pk.offsets[hosted[0]]) if hosted else total
  pk.total_bytes = max(total, 16)
  reader.sequential(pk, files, infos)
  if pk.prog_index:
    _pack_progressive(pk, files, infos)
  return pk


def pack(files: Sequence, fallback: Optional[Callable] = None, infos: Optional[List[JpegInfo]] = None,
         progressive: bool = False, segment_bytes: Optional[int] = None) -> Packed:
  """Batch of entries -> the tables of asm_jpeg_decode (numpy, host).  An entry is an encoded file or an already decoded
  uint8 [H, W, 3] array (which only gets a slot in the output).  Files of an unsupported kind go through ``fallback(bytes)
  -> uint8 [H, W, 3]``; without one the call raises NotImplementedError naming the reason and the index.
  progressive: progressive files the device decodes become rows of a second group (the prog_* fields, the tables of
  asm_jpeg_decode_progressive); `infos`, when given, must then have been parsed with the flag too.
  segment_bytes: also fill the segment table of asm_jpeg_decode_parallel for the sequential rows (entropy='parallel')."""
  return _pack(_HostHeaders(infos), files, fallback, progressive, segment_bytes)


def layout_heads(heads: np.ndarray, sizes=None, tail=(), segment_bytes: Optional[int] = None):
  """The host's part between asm_jpeg_parse and asm_jpeg_parse_fill, pure numpy.  heads: HEAD_DTYPE [n], row k the head row
  of batch entry k; the entries of class 0 become the sequential rows, in batch order.  sizes: (height, width) of every
  entry (those of the class-0 entries are taken from their head rows); tail: the other entries in the order of their
  output slots (progressive rows, then the hosted ones).  Returns (PLACE_DTYPE [rows] placement table, batch index of each
  row, int64 slot offset of every entry, bytes of all slots, totals): pack's slot layout, block offsets, first_interval
  and first segment, with totals = dict(total_blocks, max_blocks, max_pixels, n_intervals, total_segments)."""
  heads = np.asarray(heads).view(HEAD_DTYPE).reshape(-1)
  n = len(heads)
  rows = np.flatnonzero(heads['cls'] == 0)
  h = heads[rows]
  hw = np.zeros((n, 2), np.int64)
  if sizes is not None and n:
    hw[:] = np.asarray(sizes, dtype=np.int64).reshape(n, 2)
  hw[rows, 0], hw[rows, 1] = h['height'], h['width']
  order = [int(k) for k in rows] + [int(k) for k in tail]
  if sorted(order) != list(range(n)):
    raise ValueError('layout_heads: the class-0 rows and `tail` must name every entry once')
  offsets, total = slot_layout(hw[:, 0] * hw[:, 1] * 3, order)
  width, height, ncomp, hs, vs = (h[f].astype(np.int64) for f in ('width', 'height', 'ncomp', 'hs', 'vs'))
  blocks = mcu_grid(width, height, ncomp, hs, vs)[2]
  n_iv = h['n_intervals'].astype(np.int64)
  n_seg = h['n_segments'].astype(np.int64) if segment_bytes is not None else np.zeros(len(h), np.int64)
  totals = dict(total_blocks=int(blocks.sum()), max_blocks=int(blocks.max(initial=0)),
                max_pixels=int((width * height).max(initial=0)), n_intervals=int(n_iv.sum()),
                total_segments=int(n_seg.sum()))
  if totals['total_segments'] >= 2 ** 30:
    raise ValueError('segment_bytes = %d gives %d segments, more than one call takes' % (segment_bytes,
                                                                                        totals['total_segments']))
  if totals['n_intervals'] >= 2 ** 31:
    raise ValueError('%d restart intervals, more than one call takes' % totals['n_intervals'])
  place = np.zeros(len(rows), PLACE_DTYPE)
  place['span'] = rows
  place['first_interval'] = np.cumsum(n_iv) - n_iv
  place['first_segment'] = np.cumsum(n_seg) - n_seg
  place['coef_offset'] = (np.cumsum(blocks) - blocks) * 64
  place['dst_offset'] = offsets[rows]
  return place, order[:len(rows)], offsets, total, totals


class _HeadInfo:
  """What the host keeps of a file asm_jpeg_parse gave class 0: its size.  Routed as the JpegInfo of a sequential file;
  the rest of its headers stays on the device."""
  __slots__ = ('height', 'width')
  unsupported, progressive = None, False

  def __init__(self, height, width):
    self.height, self.width = height, width


class _DeviceHeaders:
  """The header reader of ``pack_device``: asm_jpeg_parse and the one read-back, layout_heads, asm_jpeg_parse_fill."""

  def __init__(self, device, resident):
    self.dev, self.resident = device, resident

  def read(self, files, progressive, segment_bytes):
    n, dev = len(files), torch.device(self.dev)
    encoded = [is_encoded(f) for f in files]
    spans = np.zeros(n, SPAN_DTYPE)
    if self.resident is not None:
      buf, where = self.resident
      where = np.asarray(where.cpu() if isinstance(where, torch.Tensor) else where, dtype=np.int64)
      if (not isinstance(buf, torch.Tensor) or buf.dim() != 1 or buf.dtype != torch.uint8 or buf.device.type != dev.type or
          (dev.index is not None and buf.device.index != dev.index)):
        raise ValueError('resident: the buffer must be a 1-D uint8 tensor on %s' % dev)
      if where.shape != (n, 2):
        raise ValueError('resident: one (offset, length) per entry, got shape %s for %d entries' % (where.shape, n))
      for k, e in enumerate(encoded):
        if not e:
          raise ValueError('entry %d: a decoded image cannot be resident' % k)
      spans['offset'], spans['length'] = where[:, 0], where[:, 1]
    else:
      whole = [_as_array(f) for f, e in zip(files, encoded) if e]
      spans['length'][encoded] = [a.size for a in whole]
      spans['offset'], total = slot_layout(spans['length'])
      buf = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
      stage_into(buf, whole, spans['offset'][encoded])
    self.buf, self.spans_dev = buf, upload_table(spans, dev)
    self.heads_dev, self.tables_dev = ops.jpeg_parse(buf, self.spans_dev, n, segment_bytes)
    self.heads = heads = self.heads_dev.cpu().numpy().view(HEAD_DTYPE)        # the path's one synchronisation
    infos = [None] * n
    for k, (cls, height, width) in enumerate(zip(heads['cls'].tolist(), heads['height'].tolist(), heads['width'].tolist())):
      if cls == 0:
        infos[k] = _HeadInfo(height, width)
      elif encoded[k]:
        infos[k] = parse(files[k], progressive)
        if infos[k].unsupported is None and not infos[k].progressive:
          raise lib.AsmError('entry %d: asm_jpeg_parse refused (class %d) a file the host parser accepts' % (k, cls))
    return infos

  def layout(self, pk, tail):
    self.place, rows, offsets, total, totals = layout_heads(self.heads, pk.sizes, tail, pk.segment_bytes)
    assert rows == pk.dev_index
    pk.total_blocks, pk.max_blocks, pk.max_pixels = totals['total_blocks'], totals['max_blocks'], totals['max_pixels']
    pk.n_intervals, pk.total_segments = totals['n_intervals'], totals['total_segments']
    return offsets, total

  def sequential(self, pk, files, infos):
    descs, tables, intervals, first, pk.fill_status = ops.jpeg_parse_fill(
        self.buf, self.spans_dev, len(files), self.heads_dev, self.tables_dev, upload_table(self.place, self.dev),
        len(self.place), pk.n_intervals, pk.total_segments, pk.segment_bytes)
    pk.dev_tables = (self.buf, descs, tables, intervals, first)


def pack_device(files: Sequence, device, resident=None, fallback: Optional[Callable] = None, progressive: bool = False,
                segment_bytes: Optional[int] = None) -> Packed:
  """``pack`` with the headers read on the device: the sequential rows' tables come back as device tensors
  (``dev_tables``) that ``decode_packed`` hands to the same kernels, with `files` = the buffer the whole files lie in.
  resident = (1-D uint8 device buffer, int64 [n, 2] offset and length of every entry's bytes in it): the files are there
  already (records.RecordDataset(keep_payloads=True)); files[k] is then read only for an entry the device hands back.
  Without it the whole files travel up in one staged copy, at 16-byte slots; a decoded array is then allowed as in pack,
  with `resident` it raises ValueError.  Two launches around ONE synchronisation (the head rows, 72 bytes a file).
  A file the device does not give class 0 goes through ``parse`` here exactly as in ``pack``: the same progressive rows,
  fallback calls, NotImplementedError and ValueError.  Slots, offsets and every decoded byte equal pack's."""
  return _pack(_DeviceHeaders(device, resident), files, fallback, progressive, segment_bytes)


def _raise_corrupt(status_rows):
  """status_rows: (batch index, status word) of every device row, on the host"""
  bad = sorted((k, st) for k, st in status_rows if st)
  if bad:
    raise ValueError('jpeg_decode: corrupt entropy-coded data in entries %s (status %s)' % (
        [k for k, _ in bad], [st for _, st in bad]))


def decode_packed(pk: Packed, device, stages: int = 3, check: bool = True, return_workspace: bool = False,
                  entropy: str = 'sequential', return_info: bool = False):
  """Run the device decode of a packed batch and copy the already decoded entries into their slots (one staged copy).
  Returns (uint8 device buffer of pk.total_bytes, int32 status per device row: the sequential rows, then the progressive
  ones), plus ops.jpeg_decode's workspace (raw coefficients first) when return_workspace -- and, for a batch with
  progressive rows, ops.jpeg_decode_progressive's as a fourth value.  check: wait for the decode, return the status on
  the host and raise ValueError naming the entries whose entropy-coded data is corrupt.
  The two groups are launched one after the other (three launches each) and write disjoint slots of the buffer.
  entropy: 'parallel' decodes the sequential rows with asm_jpeg_decode_parallel (the pack must have been made with
  segment_bytes); every result is the same.  return_info (parallel only): append the int32 [rows, 2] device tensor of
  segments and rounds per sequential row."""
  if entropy not in ENTROPY_MODES:
    raise ValueError('entropy must be one of %s, got %r' % (ENTROPY_MODES, entropy))
  if entropy == 'parallel' and pk.segment_bytes is None:
    raise ValueError("entropy='parallel' needs a batch packed with segment_bytes")
  if return_info and entropy != 'parallel':
    raise ValueError("return_info needs entropy='parallel'")
  dev = torch.device(device)
  dst = torch.empty(pk.total_bytes, dtype=torch.uint8, device=dev)
  status = ws = prog_status = prog_ws = info = None
  if pk.dev_tables is not None:           # pack_device: the tables are on the device already
    tabs, n_iv = pk.dev_tables, pk.n_intervals
  else:
    host = (pk.files, pk.descs, pk.tables, pk.intervals) + ((pk.segment_first,) if entropy == 'parallel' else ())
    tabs, n_iv = tuple(upload_table(t, dev) for t in host) if pk.dev_index else (), len(pk.intervals)
  if pk.dev_index and entropy == 'parallel':
    status, ws, info = ops.jpeg_decode_parallel(*tabs[:5], len(pk.dev_index), n_iv, pk.total_segments, pk.segment_bytes,
                                                pk.total_blocks, pk.max_blocks, pk.max_pixels, dst, stages=stages,
                                                info=True)
  elif pk.dev_index:
    status, ws = ops.jpeg_decode(*tabs[:4], len(pk.dev_index), n_iv, pk.total_blocks, pk.max_blocks, pk.max_pixels, dst,
                                 stages=stages)
  if status is not None and pk.fill_status is not None:
    status = status | pk.fill_status       # a row asm_jpeg_parse_fill refused (ASM_JPEG_EDESC)
  if pk.prog_index:
    if return_workspace and ws is not None:
      ws = ws.clone()       # both calls use the stream's one scratch buffer
    tabs = (pk.prog_files, pk.prog_descs, pk.prog_tables, pk.prog_scans, pk.prog_huff, pk.prog_intervals)
    prog_status, prog_ws = ops.jpeg_decode_progressive(
        *(upload_table(t, dev) for t in tabs), len(pk.prog_index), len(pk.prog_scans), len(pk.prog_huff),
        len(pk.prog_intervals), pk.prog_total_blocks, pk.prog_max_blocks, pk.prog_max_pixels, dst, stages=stages)
    status = prog_status if status is None else torch.cat([status, prog_status])
  if check and status is not None:
    status = status.cpu()
    _raise_corrupt(zip(pk.dev_index + pk.prog_index, status.tolist()))
  if pk.fallback:
    keys = sorted(pk.fallback)
    stage_into(dst[pk.host_begin:], [pk.fallback[k] for k in keys], [pk.offsets[k] - pk.host_begin for k in keys])
  out = (dst, status)
  if return_workspace:
    out += (ws, prog_ws) if pk.prog_index else (ws,)
  return out + (info,) if return_info else out


def decode_batch(files: Sequence, device, fallback: Optional[Callable] = None, dct_method: str = '',
                 progressive: bool = False, entropy: str = 'sequential', segment_bytes: Optional[int] = None,
                 parse: str = 'host', resident=None):
  """Encoded files -> (packed uint8 device buffer, byte offsets, [(height, width)]): image k is
  buffer[offsets[k] : offsets[k] + 3 * h * w] viewed as [h, w, 3].  Raises ValueError naming the files whose
  entropy-coded data is corrupt, NotImplementedError for an unsupported kind without ``fallback``.
  progressive: decode progressive files on the device too (they need no fallback then).
  entropy: 'parallel' decodes each sequential file's scan on all lanes of a workgroup, in segments of segment_bytes
  (default DEFAULT_SEGMENT_BYTES); the pixels are the same.
  parse: 'device' reads the headers on the device too (pack_device; opt-in, every result is the same); resident: the
  (buffer, spans) of files that lie on the device already (parse='device' only)."""
  check_dct_method(dct_method)
  segment_bytes = check_modes(entropy, segment_bytes, parse, resident)
  if parse == 'device':
    pk = pack_device(files, device, resident, fallback, progressive=progressive, segment_bytes=segment_bytes)
  else:
    pk = pack(files, fallback, progressive=progressive, segment_bytes=segment_bytes)
  dst = decode_packed(pk, device, entropy=entropy)[0]
  return dst, pk.offsets, pk.sizes
