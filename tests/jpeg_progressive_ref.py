"""numpy reference of the device decoder for progressive (SOF2) files, written from the rules of DESIGN.md 1.2 (T.81 annex
G) and from nothing in the package: its own marker reader and its own four scan kinds, then tests/jpeg_ref.py's pixel
stages (ISLOW inverse DCT, fancy upsampling, YCbCr -> RGB).

  read_scans(data)    -> header dict: H, W, comps, q, scans = [dict(comps, ss, se, ah, al, huff, ri, begin)]
  coefficients(data)  -> (list of int16 [blocks_high, blocks_wide, 64] per component on the PADDED grid, natural order, raw;
                          header dict).  Blocks of the padded grid that no scan visits stay zero.
  true_grid(h, c)     -> (blocks high, blocks wide) of component c's true block grid
  decode(data)        -> uint8 [H, W, 3]
"""
import numpy as np

from tests import jpeg_ref
from tests.jpeg_ref import ZIGZAG, _Bits, _code_table, _extend, _geometry, _symbol


def read_scans(data):
  b = bytes(data)
  assert b[:2] == b'\xff\xd8', 'not a JPEG file'
  h = dict(q={}, scans=[])
  huff, ri = {}, 0
  at = 2
  while True:
    assert b[at] == 0xFF, 'expected a marker at byte %d' % at
    while b[at] == 0xFF:
      at += 1
    m = b[at]
    at += 1
    if m == 0xD9:
      return h
    n = (b[at] << 8) | b[at + 1]
    seg = b[at + 2:at + n]
    at += n
    if m == 0xDB:
      assert not h['scans'], 'DQT between scans'
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
        huff[(seg[p] >> 4, seg[p] & 15)] = (counts, list(seg[p + 17:p + 17 + k]))
        p += 17 + k
    elif m == 0xC2:
      assert seg[0] == 8
      h['H'], h['W'] = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
      h['comps'] = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])]
    elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
      raise AssertionError('frame type SOF%d is not progressive' % (m - 0xC0))
    elif m == 0xDD:
      ri = (seg[0] << 8) | seg[1]
    elif m == 0xDA:
      ns = seg[0]
      ids = [c[0] for c in h['comps']]
      named = [(seg[1 + 2 * i], seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)]
      sc = dict(comps=[ids.index(cs) for cs, _, _ in named], ss=seg[1 + 2 * ns], se=seg[2 + 2 * ns],
                ah=seg[3 + 2 * ns] >> 4, al=seg[3 + 2 * ns] & 15, ri=ri, begin=at,
                huff=[(huff.get((0, td)), huff.get((1, ta))) for _, td, ta in named])      # as defined at THIS SOS
      h['scans'].append(sc)
      # the entropy-coded bytes end at the first FF followed by neither 00, FF nor RSTm
      while not (b[at] == 0xFF and b[at + 1] != 0 and b[at + 1] != 0xFF and not 0xD0 <= b[at + 1] <= 0xD7):
        at += 1
      sc['end'] = at


def true_grid(h, c):
  fac, hmax, vmax, _, _ = _geometry(h)
  hh, v = fac[c]
  return -(-(-(-h['H'] * v // vmax)) // 8), -(-(-(-h['W'] * hh // hmax)) // 8)


def _correct(bits, blk, z, p1):
  if bits.bit() and (int(blk[z]) & p1) == 0:
    blk[z] += p1 if blk[z] >= 0 else -p1


def _block(bits, sc, i, blk, st, seen):
  """one block of scan component i; st: dict(pred=[..], eobrun=int) of the restart interval"""
  ss, se, ah, al = sc['ss'], sc['se'], sc['ah'], sc['al']
  if ss == 0 and ah == 0:                       # DC first
    s = _symbol(bits, sc['dc'][i], seen)
    st['pred'][i] += _extend(bits.bits(s), s)
    blk[0] = st['pred'][i] * (1 << al)
  elif ss == 0:                                 # DC refinement
    if bits.bit():
      blk[0] |= 1 << al
  elif ah == 0:                                 # AC first
    if st['eobrun'] > 0:
      st['eobrun'] -= 1
      return
    k = ss
    while k <= se:
      rs = _symbol(bits, sc['ac'][i], seen)
      r, s = rs >> 4, rs & 15
      if s:
        k += r
        assert k <= se
        blk[ZIGZAG[k]] = _extend(bits.bits(s), s) * (1 << al)
        k += 1
      elif r == 15:
        k += 16
      else:
        st['eobrun'] = (1 << r) - 1 + (bits.bits(r) if r else 0)
        break
  else:                                         # AC refinement
    p1 = 1 << al
    k = ss
    if st['eobrun'] == 0:
      while k <= se:
        rs = _symbol(bits, sc['ac'][i], seen)
        r, s = rs >> 4, rs & 15
        value = 0
        if s:
          assert s == 1
          value = p1 if bits.bit() else -p1
        elif r < 15:
          st['eobrun'] = (1 << r) + (bits.bits(r) if r else 0)
          break
        while k <= se:
          z = ZIGZAG[k]
          if blk[z] != 0:
            _correct(bits, blk, z, p1)
          else:
            r -= 1
            if r < 0:
              break
          k += 1
        if value:
          assert k <= se
          blk[ZIGZAG[k]] = value
        k += 1
    if st['eobrun'] > 0:
      while k <= se:
        z = ZIGZAG[k]
        if blk[z] != 0:
          _correct(bits, blk, z, p1)
        k += 1
      st['eobrun'] -= 1


def coefficients(data):
  h = read_scans(data)
  fac, hmax, vmax, mx, my = _geometry(h)
  coefs = [np.zeros((my * v, mx * hh, 64), np.int16) for hh, v in fac]
  b = bytes(data)
  seen = [0]
  for sc in h['scans']:
    sc['dc'] = [_code_table(*d) if d and sc['ss'] == 0 and sc['ah'] == 0 else None for d, _ in sc['huff']]
    sc['ac'] = [_code_table(*a) if a and sc['ss'] > 0 else None for _, a in sc['huff']]
    bits = _Bits(b, sc['begin'])
    comps = sc['comps']
    if len(comps) > 1:                          # interleaved: the padded MCU grid
      order = [[(i, c, row * fac[c][1] + by, col * fac[c][0] + bx) for i, c in enumerate(comps)
                for by in range(fac[c][1]) for bx in range(fac[c][0])] for row in range(my) for col in range(mx)]
    else:                                       # one component: its TRUE block grid, one block per MCU
      th, tw = true_grid(h, comps[0])
      order = [[(0, comps[0], y, x)] for y in range(th) for x in range(tw)]
    st = dict(pred=[0] * len(comps), eobrun=0)
    m = 0
    for n, mcu in enumerate(order):
      if sc['ri'] and n and n % sc['ri'] == 0:
        bits.restart(m)
        m = (m + 1) & 7
        st = dict(pred=[0] * len(comps), eobrun=0)
      for i, c, y, x in mcu:
        _block(bits, sc, i, coefs[c][y, x], st, seen)
  return coefs, h


def decode(data):
  coefs, h = coefficients(data)
  fac, hmax, vmax, _, _ = _geometry(h)
  H, W = h['H'], h['W']
  planes = [jpeg_ref.idct_plane(c, h['q'][comp[3]]) for c, comp in zip(coefs, h['comps'])]
  y = planes[0][:H, :W]
  if len(planes) == 1:
    return np.stack([y, y, y], axis=-1)
  ch, cw = -(-H // vmax), -(-W // hmax)
  chroma = []
  for p in planes[1:]:
    p = p[:ch, :cw]
    if (hmax, vmax) == (2, 1):
      p = jpeg_ref.upsample_h2v1(p)
    elif (hmax, vmax) == (2, 2):
      p = jpeg_ref.upsample_h2v2(p)
    chroma.append(p[:H, :W])
  return jpeg_ref.ycc_to_rgb(y, chroma[0], chroma[1])
