"""numpy reference of the device JPEG decoder, written from the rules of DESIGN.md 1.2 and from nothing in the package:
its own marker reader, its own Huffman decode, libjpeg's integer ISLOW inverse DCT, "fancy" chroma upsampling and
16-bit fixed-point YCbCr -> RGB.  It decodes what the device path decodes (baseline / extended-sequential Huffman, one
interleaved scan, grey or YCbCr with luma sampling 1x1 / 2x1 / 2x2) and nothing else.

  decode(data)        -> uint8 [H, W, 3]
  coefficients(data)  -> (list of int16 [blocks_high, blocks_wide, 64] per component, natural order, raw) , header dict
  stats(data)         -> dict(max_code_length=..., stuffed=...)    (what the fixture generator asserts about the set)
"""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47,
          55, 62, 63]


def read_header(data):
  b = bytes(data)
  assert b[:2] == b'\xff\xd8', 'not a JPEG file'
  h = dict(q={}, huff={}, ri=0)
  at = 2
  while True:
    assert b[at] == 0xFF
    while b[at] == 0xFF:
      at += 1
    m = b[at]
    at += 1
    n = (b[at] << 8) | b[at + 1]
    seg = b[at + 2:at + n]
    at += n
    if m == 0xDB:
      p = 0
      while p < len(seg):
        assert seg[p] >> 4 == 0, '8-bit quantisation tables only'
        t = np.zeros(64, np.int64)
        t[ZIGZAG] = list(seg[p + 1:p + 65])
        h['q'][seg[p] & 15] = t
        p += 65
    elif m == 0xC4:
      p = 0
      while p < len(seg):
        counts = list(seg[p + 1:p + 17])
        k = sum(counts)
        h['huff'][(seg[p] >> 4, seg[p] & 15)] = (counts, list(seg[p + 17:p + 17 + k]))
        p += 17 + k
    elif m in (0xC0, 0xC1):
      assert seg[0] == 8
      h['H'], h['W'] = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
      h['comps'] = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])]
    elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
      raise AssertionError('frame type SOF%d is outside the reference decoder' % (m - 0xC0))
    elif m == 0xDD:
      h['ri'] = (seg[0] << 8) | seg[1]
    elif m == 0xDA:
      ns = seg[0]
      assert ns == len(h['comps']), 'one interleaved scan'
      h['scan'] = [(seg[1 + 2 * i], seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)]
      h['scan_begin'] = at
      return h


class _Bits:
  """bit reader over the entropy-coded bytes starting at `at`; stops at a marker"""

  def __init__(self, b, at):
    self.b, self.at, self.acc, self.n = b, at, 0, 0
    self.stuffed = 0

  def bit(self):
    if self.n == 0:
      v = self.b[self.at]
      self.at += 1
      if v == 0xFF:
        nxt = self.b[self.at]
        assert nxt == 0, 'marker FF %02X inside an interval' % nxt
        self.at += 1
        self.stuffed += 1
      self.acc, self.n = v, 8
    self.n -= 1
    return (self.acc >> self.n) & 1

  def bits(self, k):
    v = 0
    for _ in range(k):
      v = (v << 1) | self.bit()
    return v

  def restart(self, m):
    self.n = 0                                      # pad bits
    while self.b[self.at] == 0xFF and self.b[self.at + 1] == 0xFF:
      self.at += 1
    assert self.b[self.at] == 0xFF and self.b[self.at + 1] == 0xD0 + m, 'expected RST%d' % m
    self.at += 2


def _code_table(counts, vals):
  """(length, code) -> symbol, canonical codes (T.81 annex C)"""
  table, code, k = {}, 0, 0
  for length in range(1, 17):
    for _ in range(counts[length - 1]):
      table[(length, code)] = vals[k]
      code += 1
      k += 1
    code <<= 1
  return table


def _symbol(bits, table, seen):
  code = 0
  for length in range(1, 17):
    code = (code << 1) | bits.bit()
    s = table.get((length, code))
    if s is not None:
      seen[0] = max(seen[0], length)
      return s
  raise AssertionError('no Huffman code matches')


def _extend(v, s):
  return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _geometry(h):
  comps = h['comps']
  if len(comps) == 1:
    fac = [(1, 1)]
  else:
    fac = [(c[1], c[2]) for c in comps]
    assert fac[1:] == [(1, 1), (1, 1)] and fac[0] in ((1, 1), (2, 1), (2, 2)), 'sampling outside the reference decoder'
  hmax, vmax = fac[0]
  mx, my = -(-h['W'] // (8 * hmax)), -(-h['H'] // (8 * vmax))
  return fac, hmax, vmax, mx, my


def coefficients(data, _stats=None):
  h = read_header(data)
  fac, hmax, vmax, mx, my = _geometry(h)
  coefs = [np.zeros((my * v, mx * hh, 64), np.int16) for hh, v in fac]
  tables = {k: _code_table(*v) for k, v in h['huff'].items()}
  bits = _Bits(bytes(data), h['scan_begin'])
  seen = [0]
  pred = [0] * len(fac)
  ri, m = h['ri'], 0
  for mcu in range(mx * my):
    if ri and mcu and mcu % ri == 0:
      bits.restart(m)
      m = (m + 1) & 7
      pred = [0] * len(fac)
    row, col = divmod(mcu, mx)
    for c, (hh, v) in enumerate(fac):
      _, td, ta = h['scan'][c]
      for by in range(v):
        for bx in range(hh):
          blk = coefs[c][row * v + by, col * hh + bx]
          s = _symbol(bits, tables[(0, td)], seen)
          pred[c] += _extend(bits.bits(s), s)
          blk[0] = pred[c]
          k = 1
          while k < 64:
            rs = _symbol(bits, tables[(1, ta)], seen)
            r, s = rs >> 4, rs & 15
            if s == 0:
              if r != 15:
                break
              k += 16
              continue
            k += r
            blk[ZIGZAG[k]] = _extend(bits.bits(s), s)
            k += 1
  if _stats is not None:
    _stats.update(max_code_length=seen[0], stuffed=bits.stuffed)
  return coefs, h


def stats(data):
  st = {}
  coefficients(data, st)
  return st


_C = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137,
          f1_961=16069, f2_053=16819, f2_562=20995, f3_072=25172)


def _islow_1d(x, shift):
  """jidctint.c jpeg_idct_islow, one pass over the last axis (eight values), int64"""
  x = [x[..., i] for i in range(8)]
  z1 = (x[2] + x[6]) * _C['f0_541']
  tmp2 = z1 - x[6] * _C['f1_847']
  tmp3 = z1 + x[2] * _C['f0_765']
  tmp0 = (x[0] + x[4]) << 13
  tmp1 = (x[0] - x[4]) << 13
  tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
  tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
  z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
  z5 = (z3 + z4) * _C['f1_175']
  tmp0, tmp1, tmp2, tmp3 = tmp0 * _C['f0_298'], tmp1 * _C['f2_053'], tmp2 * _C['f3_072'], tmp3 * _C['f1_501']
  z1, z2 = -z1 * _C['f0_899'], -z2 * _C['f2_562']
  z3, z4 = -z3 * _C['f1_961'] + z5, -z4 * _C['f0_390'] + z5
  tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
  r = 1 << (shift - 1)
  out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
  return np.stack([(o + r) >> shift for o in out], axis=-1)


def idct_plane(coefs, q):
  """int16 [bh, bw, 64] raw coefficients, quantisation table [64] -> uint8 [bh * 8, bw * 8]"""
  bh, bw, _ = coefs.shape
  x = (coefs.astype(np.int64) * q.astype(np.int64)).reshape(bh, bw, 8, 8)
  ws = _islow_1d(x.transpose(0, 1, 3, 2), 11)              # pass 1: down the columns ([.., column, row])
  out = _islow_1d(ws.transpose(0, 1, 3, 2), 18)            # pass 2: along the rows
  out = np.clip(out + 128, 0, 255).astype(np.uint8)
  return out.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample_h2v1(p):
  """libjpeg h2v1 fancy (triangle) upsampling of a plane of its TRUE size; planes of one or two columns are replicated"""
  p = p.astype(np.int64)
  h, w = p.shape
  if w <= 2:
    return np.repeat(p, 2, axis=1)
  left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
  right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
  out = np.empty((h, 2 * w), np.int64)
  out[:, 0::2] = (3 * p + left + 1) >> 2
  out[:, 1::2] = (3 * p + right + 2) >> 2
  out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
  return out


def upsample_h2v2(p):
  p = p.astype(np.int64)
  h, w = p.shape
  if w <= 2:
    return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
  above = np.concatenate([p[:1], p[:-1]], axis=0)
  below = np.concatenate([p[1:], p[-1:]], axis=0)
  out = np.empty((2 * h, 2 * w), np.int64)
  for parity, other in ((0, above), (1, below)):
    s = 3 * p + other
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    row = np.empty((h, 2 * w), np.int64)
    row[:, 0::2] = (3 * s + left + 8) >> 4
    row[:, 1::2] = (3 * s + right + 7) >> 4
    row[:, 0] = (4 * s[:, 0] + 8) >> 4
    row[:, -1] = (4 * s[:, -1] + 7) >> 4
    out[parity::2] = row
  return out


def ycc_to_rgb(y, cb, cr):
  y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
  r = y + ((91881 * cr + 32768) >> 16)
  g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
  b = y + ((116130 * cb + 32768) >> 16)
  return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data):
  coefs, h = coefficients(data)
  fac, hmax, vmax, _, _ = _geometry(h)
  H, W = h['H'], h['W']
  planes = [idct_plane(c, h['q'][comp[3]]) for c, comp in zip(coefs, h['comps'])]
  if len(planes) == 1:
    y = planes[0][:H, :W]
    return np.stack([y, y, y], axis=-1)
  y = planes[0][:H, :W]
  ch, cw = -(-H // vmax), -(-W // hmax)
  chroma = []
  for p in planes[1:]:
    p = p[:ch, :cw]                                        # the true size first: the edges replicate at THIS size
    if (hmax, vmax) == (2, 1):
      p = upsample_h2v1(p)
    elif (hmax, vmax) == (2, 2):
      p = upsample_h2v2(p)
    chroma.append(p[:H, :W])
  return ycc_to_rgb(y, chroma[0], chroma[1])
