"""A small writer of spectral-selection-only progressive files (Ah = Al = 0, with end-of-band runs) from the coefficients
of a baseline file: scan scripts no common encoder writes, whose pixels are the baseline file's own.

  recode(baseline_bytes, script) -> bytes        script: a key of SCRIPTS

The DC code has 12 symbols of 4 bits, the AC code 176 symbols of 8 bits (sizes 1..10 for every run, EOB0..EOB14, ZRL); a
DHT segment precedes every scan and reuses table id 0, as libjpeg's does.  Scans of one component walk its TRUE block
grid, so the blocks a baseline encoder adds to fill whole MCUs are not carried over.
"""
import numpy as np

from tests import jpeg_ref
from tests.jpeg_progressive_ref import true_grid
from tests.jpeg_ref import ZIGZAG, _geometry

# (DC interleaved?, AC bands)
SCRIPTS = {
    'dc_each_ac_1_63': (False, [(1, 63)]),
    'dc_all_ac_1_2_3_63': (True, [(1, 2), (3, 63)]),
    'dc_each_ac_1_5_6_20_21_63': (False, [(1, 5), (6, 20), (21, 63)]),
}

DC_SYMBOLS = list(range(12))
AC_SYMBOLS = [(r << 4) | s for r in range(16) for s in range(1, 11)] + [r << 4 for r in range(16)]
assert len(AC_SYMBOLS) == 176


def _segment(marker, payload):
  return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + bytes(payload)


def _dht(cls, symbols, length):
  counts = [0] * 16
  counts[length - 1] = len(symbols)
  return _segment(0xC4, bytes([cls << 4]) + bytes(counts) + bytes(symbols))


class _Out:
  def __init__(self):
    self.acc, self.n, self.out = 0, 0, bytearray()

  def put(self, value, nbits):
    self.acc = (self.acc << nbits) | (value & ((1 << nbits) - 1))
    self.n += nbits
    while self.n >= 8:
      byte = (self.acc >> (self.n - 8)) & 255
      self.out.append(byte)
      if byte == 0xFF:
        self.out.append(0)
      self.n -= 8
    self.acc &= (1 << self.n) - 1

  def finish(self):
    if self.n:
      self.put((1 << (8 - self.n)) - 1, 8 - self.n)      # pad with ones
    return bytes(self.out)


def _magnitude(out, v, nbits):
  out.put(v if v >= 0 else v - 1, nbits)


def _dc_scan(blocks):
  """blocks: per MCU a list of (predictor slot, DC value)"""
  out = _Out()
  pred = {}
  for mcu in blocks:
    for slot, dc in mcu:
      diff = int(dc) - pred.get(slot, 0)
      pred[slot] = int(dc)
      nbits = abs(diff).bit_length()
      out.put(DC_SYMBOLS.index(nbits), 4)
      if nbits:
        _magnitude(out, diff, nbits)
  return out.finish()


def _ac_scan(blocks, ss, se):
  """blocks: int16 [n, 64] in natural order"""
  out = _Out()
  eobrun = 0

  def flush():
    nonlocal eobrun
    if eobrun:
      nbits = eobrun.bit_length() - 1
      out.put(AC_SYMBOLS.index(nbits << 4), 8)
      if nbits:
        out.put(eobrun, nbits)
      eobrun = 0

  for blk in blocks:
    r = 0
    for k in range(ss, se + 1):
      v = int(blk[ZIGZAG[k]])
      if v == 0:
        r += 1
        continue
      flush()
      while r > 15:
        out.put(AC_SYMBOLS.index(0xF0), 8)
        r -= 16
      nbits = abs(v).bit_length()
      out.put(AC_SYMBOLS.index((r << 4) | nbits), 8)
      _magnitude(out, v, nbits)
      r = 0
    if r:
      eobrun += 1
      if eobrun == 0x7FFF:
        flush()
  flush()
  return out.finish()


def recode(data, script):
  dc_together, bands = SCRIPTS[script]
  coefs, h = jpeg_ref.coefficients(data)
  fac, hmax, vmax, mx, my = _geometry(h)
  comps = h['comps']
  out = bytearray(b'\xff\xd8')
  for tq, q in sorted(h['q'].items()):
    out += _segment(0xDB, bytes([tq]) + bytes(int(q[ZIGZAG[k]]) for k in range(64)))
  out += _segment(0xC2, bytes([8]) + h['H'].to_bytes(2, 'big') + h['W'].to_bytes(2, 'big') + bytes([len(comps)]) +
                  b''.join(bytes([cid, (hh << 4) | v, tq]) for cid, hh, v, tq in comps))

  def sos(cs, ss, se):
    return _segment(0xDA, bytes([len(cs)]) + b''.join(bytes([comps[c][0], 0]) for c in cs) + bytes([ss, se, 0]))

  grids = [true_grid(h, c) for c in range(len(comps))]
  if dc_together and len(comps) > 1:
    mcus = [[(c, coefs[c][row * fac[c][1] + by, col * fac[c][0] + bx, 0]) for c in range(len(comps))
             for by in range(fac[c][1]) for bx in range(fac[c][0])] for row in range(my) for col in range(mx)]
    out += _dht(0, DC_SYMBOLS, 4) + sos(list(range(len(comps))), 0, 0) + _dc_scan(mcus)
  else:
    for c, (th, tw) in enumerate(grids):
      out += _dht(0, DC_SYMBOLS, 4) + sos([c], 0, 0) + _dc_scan([[(0, coefs[c][y, x, 0])] for y in range(th) for x in range(tw)])
  for c, (th, tw) in enumerate(grids):
    blocks = coefs[c][:th, :tw].reshape(-1, 64)
    for ss, se in bands:
      out += _dht(1, AC_SYMBOLS, 8) + sos([c], ss, se) + _ac_scan(blocks, ss, se)
  return bytes(out + b'\xff\xd9')
