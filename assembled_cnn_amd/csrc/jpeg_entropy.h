// Baseline JPEG entropy decode (ITU-T T.81 F.2.2) of one restart interval, as plain functions shared by the device
// kernel (jpeg.hip) and a host program (tools/probes/jpeg_entropy_host.cpp, built with the address and undefined-behaviour
// sanitizers): the same text is compiled for both, so what the host program proves about bounds holds for the kernel.
// The second half of the file does the same for progressive files (T.81 annex G; jpeg_progressive_kernel and
// tools/probes/jpeg_progressive_host.cpp).
// What the sequential, the segment-parallel (jpeg_parallel.h) and the progressive decoder decide alike is one function
// each: jpeg_check_interval (a row of the interval table) and jpeg_decode_dc_diff / jpeg_decode_ac_step (a baseline symbol).
//
// Rules: canonical codes of 1..16 bits; a 9-bit lookup, longer codes through maxcode / valoff; EXTEND;
// one DC predictor per component, zero at the start of the interval; EOB and ZRL; FF 00 -> FF; pad bits ignored.
// Safety: every byte read lies in [begin, end); every coefficient index is <= 63; every block index lies inside the
// component's block grid; a violation returns a non-zero ASM_JPEG_E* and stops.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/asm_hip.h"

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ inline
#else
#define JPEG_HD inline
#endif

#define JPEG_LOOK_BITS 9

// decode form of one Huffman table: look[prefix] = length << 8 | symbol for codes of <= 9 bits (0: longer, or none)
struct jpeg_dtab {
  uint16_t look[1 << JPEG_LOOK_BITS];
  int32_t maxcode[17];       // [l] largest code of length l, -1 if there is none
  int32_t valoff[17];        // [l] index in vals of the first code of length l, minus that code
  uint8_t vals[256];
};

// geometry of one image as the entropy decoder needs it
struct jpeg_geom {
  int ncomp;
  int mcus_x, n_mcus;        // MCUs per row, MCUs in the image
  int ch[3], cv[3];          // blocks per MCU of each component, horizontally and vertically
  int bw[3];                 // blocks per row of each component's (padded) grid
  int64_t base[3];           // first coefficient of each component, relative to the image's first
  int64_t n_coefs;           // all components
};

// T.81 figure A.6, index -> position in the 8x8 block
#define JPEG_ZIGZAG_INIT                                                                                            \
  {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// false: the descriptor's geometry is not one this decoder handles
JPEG_HD bool jpeg_make_geom(const asm_jpeg_desc& d, jpeg_geom* g) {
  if (d.width < 1 || d.height < 1 || d.width > 8192 || d.height > 8192) return false;
  if (d.ncomp != 1 && d.ncomp != 3) return false;
  const int hs = d.ncomp == 1 ? 1 : d.hs, vs = d.ncomp == 1 ? 1 : d.vs;
  if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
  if (d.hs != hs || d.vs != vs) return false;
  if (d.mcus_x != (d.width + 8 * hs - 1) / (8 * hs) || d.mcus_y != (d.height + 8 * vs - 1) / (8 * vs)) return false;
  g->ncomp = d.ncomp;
  g->mcus_x = d.mcus_x;
  g->n_mcus = d.mcus_x * d.mcus_y;
  int64_t at = 0;
  for (int c = 0; c < 3; ++c) {
    g->ch[c] = c == 0 ? hs : 1;
    g->cv[c] = c == 0 ? vs : 1;
    g->bw[c] = d.mcus_x * g->ch[c];
    g->base[c] = at;
    if (c < d.ncomp) at += (int64_t)g->bw[c] * (d.mcus_y * g->cv[c]) * 64;
  }
  g->n_coefs = at;
  return true;
}

// maxcode / valoff / vals of a table (T.81 F.2.2.3, figure F.15); any bits[] is safe: indices into vals are masked
JPEG_HD void jpeg_dtab_prepare(const asm_jpeg_huff& h, jpeg_dtab* t) {
  int code = 0, k = 0;
  t->maxcode[0] = -1;
  t->valoff[0] = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = h.bits[l - 1];
    t->valoff[l] = k - code;
    t->maxcode[l] = n ? code + n - 1 : -1;
    code = (code + n) << 1;
    k += n;
  }
  for (int i = 0; i < 256; ++i) t->vals[i] = h.vals[i];
}

// the code that starts the 16 bits `peek` (first bit = bit 15), lengths lo..hi: length << 8 | symbol, 0 if none
JPEG_HD unsigned jpeg_code_lookup(const jpeg_dtab* t, unsigned peek, int lo, int hi) {
  for (int l = lo; l <= hi; ++l) {
    const int code = (int)(peek >> (16 - l));
    if (code <= t->maxcode[l]) return ((unsigned)l << 8) | t->vals[(t->valoff[l] + code) & 255];
  }
  return 0;
}

JPEG_HD void jpeg_dtab_fill_look(jpeg_dtab* t, int first, int step) {
  for (int i = first; i < (1 << JPEG_LOOK_BITS); i += step)
    t->look[i] = (uint16_t)jpeg_code_lookup(t, (unsigned)i << (16 - JPEG_LOOK_BITS), 1, JPEG_LOOK_BITS);
}

// bit reader over [p, end): `n` bits are held in the low end of buf, the last `pad` of them are zeros invented after the
// end of the data (or after a marker); consuming one of those is the overrun error
struct jpeg_bits {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t buf, word;
  int n, pad, wn;
  bool done;
};

JPEG_HD void jpeg_bits_init(jpeg_bits* b, const uint8_t* p, const uint8_t* end) {
  b->p = p;
  b->end = end;
  b->buf = b->word = 0;
  b->n = b->pad = b->wn = 0;
  b->done = false;
}

// next byte of the interval, -1 at its end; reads eight bytes at a time while eight remain
JPEG_HD int jpeg_next_byte(jpeg_bits* b) {
  if (b->wn == 0) {
    const int64_t left = b->end - b->p;
    if (left >= 8) {
      memcpy(&b->word, b->p, 8);
      b->p += 8;
      b->wn = 8;
    } else if (left > 0) {
      b->word = *b->p++;
      b->wn = 1;
    } else {
      return -1;
    }
  }
  const int v = (int)(b->word & 255u);
  b->word >>= 8;
  --b->wn;
  return v;
}

JPEG_HD void jpeg_bits_fill(jpeg_bits* b) {
  while (b->n <= 56) {
    int v = b->done ? -1 : jpeg_next_byte(b);
    if (v == 0xFF) {
      const int s = jpeg_next_byte(b);       // FF 00 is the data byte FF; FF + anything else (or nothing) ends the data
      if (s != 0) v = -1;
    }
    if (v < 0) {
      b->done = true;
      b->pad += 8;
      v = 0;
    }
    b->buf = (b->buf << 8) | (uint64_t)v;
    b->n += 8;
  }
}

JPEG_HD unsigned jpeg_bits_peek16(const jpeg_bits* b) { return (unsigned)(b->buf >> (b->n - 16)) & 0xFFFFu; }

// one Huffman symbol; -1 and *err set if no code matches or the data ran out
JPEG_HD int jpeg_decode_symbol(jpeg_bits* b, const jpeg_dtab* t, int* err) {
  if (b->n < 32) jpeg_bits_fill(b);
  const unsigned peek = jpeg_bits_peek16(b);
  unsigned e = t->look[peek >> (16 - JPEG_LOOK_BITS)];
  if (e == 0) e = jpeg_code_lookup(t, peek, JPEG_LOOK_BITS + 1, 16);
  if (e == 0) {
    *err |= ASM_JPEG_EBADCODE;
    return -1;
  }
  b->n -= (int)(e >> 8);
  if (b->n < b->pad) {
    *err |= ASM_JPEG_EOVERRUN;
    return -1;
  }
  return (int)(e & 255u);
}

// k raw bits (0..16) of those already in buf, first bit first; 0 and *err set if one of them is a pad bit
JPEG_HD int jpeg_take_bits(jpeg_bits* b, int k, int* err) {
  b->n -= k;
  if (b->n < b->pad) {
    *err |= ASM_JPEG_EOVERRUN;
    return 0;
  }
  return (int)((b->buf >> b->n) & ((1u << k) - 1u));
}

// s bits (1..15; the caller filled at least 32 before the symbol) -> EXTEND(value, s) (T.81 F.2.2.1); with *err set the
// value means nothing and every caller drops it
JPEG_HD int jpeg_receive_extend(jpeg_bits* b, int s, int* err) {
  const int v = jpeg_take_bits(b, s, err);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// The baseline symbol step of the sequential, the segment-parallel and (DC half) the progressive decoder: a DC symbol and
// its EXTEND -> *diff (0 for the symbol 0).  Returns 0 or ASM_JPEG_E*.  What becomes of the predictor is the caller's business.
JPEG_HD int jpeg_decode_dc_diff(jpeg_bits* b, const jpeg_dtab* t, int* diff) {
  int err = 0;
  *diff = 0;
  const int s = jpeg_decode_symbol(b, t, &err);
  if (s < 0) return err;
  if (s > 15) return ASM_JPEG_EBADCODE;
  if (s) *diff = jpeg_receive_extend(b, s, &err);
  return err;
}

// One AC symbol at zig-zag index *k (1..63) of a block: ZRL moves *k on by sixteen, EOB sets it to 64, anything else skips
// its run, stores EXTEND at the index it reaches (through `out` unless that is null: symbols only) and moves one past it.
// Returns 0 or ASM_JPEG_E*; an index past 63 is ASM_JPEG_EBADCODE.
JPEG_HD int jpeg_decode_ac_step(jpeg_bits* b, const jpeg_dtab* t, const uint8_t* zigzag, int* k, int16_t* out) {
  int err = 0;
  const int rs = jpeg_decode_symbol(b, t, &err);
  if (rs < 0) return err;
  const int run = rs >> 4, s = rs & 15;
  if (s == 0) {
    *k = run == 15 ? *k + 16 : 64;
    return 0;
  }
  *k += run;
  if (*k > 63) return ASM_JPEG_EBADCODE;
  const int val = jpeg_receive_extend(b, s, &err);
  if (err) return err;
  if (out) out[zigzag[*k]] = (int16_t)val;
  ++*k;
  return 0;
}

// Row k of the n_intervals rows of one scan, before a byte of it is read: it must belong to image `img`, lie inside the
// bytes [range_begin, range_end) (ASM_JPEG_EDESC), name the MCUs and the RSTm that k, restart_interval and the scan's
// n_mcus_scan MCUs give it (ASM_JPEG_ERESTART), and those MCUs must exist (ASM_JPEG_EDESC) -- in this order.  0: the
// interval decodes *n_mcus MCUs from *first_mcu.  The one check of the sequential, parallel and progressive decoders.
JPEG_HD int jpeg_check_interval(const asm_jpeg_interval& iv, int k, int n_intervals, int img, int restart_interval,
                                int n_mcus_scan, int64_t range_begin, int64_t range_end, int* first_mcu, int* n_mcus) {
  const int64_t first = restart_interval > 0 ? (int64_t)k * restart_interval : 0;
  const int64_t left = n_mcus_scan - first;
  const int64_t count = restart_interval > 0 ? (restart_interval < left ? restart_interval : left) : n_mcus_scan;
  const bool last = k == n_intervals - 1;
  *first_mcu = *n_mcus = 0;
  if (iv.image != img || iv.byte_begin < range_begin || iv.byte_end < iv.byte_begin || iv.byte_end > range_end)
    return ASM_JPEG_EDESC;
  if (iv.first_mcu != first || iv.n_mcus != count || iv.rst != (last ? -1 : (k & 7))) return ASM_JPEG_ERESTART;
  if (first < 0 || count < 1 || first > n_mcus_scan - count) return ASM_JPEG_EDESC;
  *first_mcu = (int)first;
  *n_mcus = (int)count;
  return 0;
}

// Decode MCUs [first_mcu, first_mcu + n_mcus) (jpeg_check_interval passed them) of one image from the bytes [begin, end)
// into coefs (the image's own region of g.n_coefs int16, already zero).  dc[c] / ac[c]: component c's.  Returns 0 or ASM_JPEG_E*.
JPEG_HD int jpeg_decode_interval(const uint8_t* begin, const uint8_t* end, const jpeg_geom& g, const jpeg_dtab* const* dc,
                                 const jpeg_dtab* const* ac, const uint8_t* zigzag, int first_mcu, int n_mcus,
                                 int16_t* coefs) {
  jpeg_bits b;
  jpeg_bits_init(&b, begin, end);
  int pred[3] = {0, 0, 0};
  int my = first_mcu / g.mcus_x, mx = first_mcu - my * g.mcus_x;
  for (int m = 0; m < n_mcus; ++m) {
    for (int c = 0; c < g.ncomp; ++c) {
      for (int v = 0; v < g.cv[c]; ++v) {
        for (int h = 0; h < g.ch[c]; ++h) {
          const int64_t blk = (int64_t)(my * g.cv[c] + v) * g.bw[c] + (mx * g.ch[c] + h);
          const int64_t at = g.base[c] + blk * 64;
          if (at < 0 || at + 64 > g.n_coefs) return ASM_JPEG_EDESC;
          int16_t* out = coefs + at;
          int diff;
          int err = jpeg_decode_dc_diff(&b, dc[c], &diff);
          if (err) return err;
          pred[c] = (int16_t)(pred[c] + diff);      // a running predictor, stored when it is not the zero already there
          if (pred[c]) out[0] = (int16_t)pred[c];
          for (int k = 1; k < 64;) {
            err = jpeg_decode_ac_step(&b, ac[c], zigzag, &k, out);
            if (err) return err;
          }
        }
      }
    }
    if (++mx == g.mcus_x) {
      mx = 0;
      ++my;
    }
  }
  return 0;
}

// intervals a workgroup expects for a scan of n_mcus MCUs: one without DRI, else one per restart_interval MCUs
JPEG_HD int jpeg_expected_intervals(int restart_interval, int n_mcus) {
  return restart_interval > 0 ? (int)(((int64_t)n_mcus + restart_interval - 1) / restart_interval) : 1;
}

// What lane `lane` of `lanes` does for image `img`: its share (k = lane, lane + lanes, ...) of the image's rows of the
// interval table, each checked against the descriptor before a byte of it is read.  tab: dc 0, dc 1, ac 0, ac 1.
// The caller has checked the descriptor itself (geometry, offsets, selectors < 2, first_interval + n_intervals in range).
JPEG_HD int jpeg_decode_lane(const uint8_t* files, const asm_jpeg_desc& d, const jpeg_geom& g,
                             const asm_jpeg_interval* intervals, int img, const jpeg_dtab* tab, const uint8_t* zigzag,
                             int lane, int lanes, int16_t* coefs) {
  const jpeg_dtab* dc[3] = {&tab[d.dcsel[0] & 1], &tab[d.dcsel[1] & 1], &tab[d.dcsel[2] & 1]};
  const jpeg_dtab* ac[3] = {&tab[2 + (d.acsel[0] & 1)], &tab[2 + (d.acsel[1] & 1)], &tab[2 + (d.acsel[2] & 1)]};
  int err = 0;
  for (int k = lane; k < d.n_intervals; k += lanes) {
    const asm_jpeg_interval iv = intervals[d.first_interval + k];
    int first, count;
    // the row must lie in the descriptor's scan; a refused row is ORed in and the lane goes on to its next interval
    const int row_err = jpeg_check_interval(iv, k, d.n_intervals, img, d.restart_interval, g.n_mcus, d.scan_offset,
                                            d.scan_offset + d.scan_bytes, &first, &count);
    err |= row_err ? row_err
                   : jpeg_decode_interval(files + iv.byte_begin, files + iv.byte_end, g, dc, ac, zigzag, first, count, coefs);
  }
  return err;
}

// one scan on many lanes: the segment-parallel form of jpeg_decode_lane (asm_jpeg_decode_parallel)
#include "jpeg_parallel.h"

// ---------------------------------------------------------------------------------------------------------------------
// Progressive files (T.81 annex G, libjpeg's jdphuff.c): one scan carries a spectral band ss..se of some components at
// successive-approximation position al.  The four kinds -- DC first, DC refinement, AC first, AC refinement -- below,
// block by block; jpeg_prog_decode_interval walks one restart interval of one scan, jpeg_prog_decode_lane a lane's share
// of a scan's intervals.  Same safety rules as above; the arithmetic is done in int and narrowed on store, negative
// values are multiplied, never shifted.
// ---------------------------------------------------------------------------------------------------------------------

// k raw bits (0..16), first bit first
JPEG_HD int jpeg_receive_bits(jpeg_bits* b, int k, int* err) {
  if (b->n < 32) jpeg_bits_fill(b);
  return jpeg_take_bits(b, k, err);
}

// a scan row as the decoder walks it: its MCU grid and what one MCU holds
struct jpeg_scan_geom {
  int ncomp;                 // components in the scan
  int comp[3];               // their indices in the frame
  int ch[3], cv[3];          // blocks per MCU of each, horizontally and vertically (1 x 1 for a scan of one component)
  int mcus_x, n_mcus;        // MCUs per row, MCUs in the scan
  int ss, se, ah, al;
};

// false: the scan row is not one this decoder handles (ASM_JPEG_EDESC)
JPEG_HD bool jpeg_make_scan_geom(const asm_jpeg_desc& d, const jpeg_geom& g, const asm_jpeg_scan& sc, jpeg_scan_geom* s) {
  if (sc.ncomp < 1 || sc.ncomp > g.ncomp) return false;
  for (int i = 0; i < sc.ncomp; ++i) {
    if (sc.comp[i] >= g.ncomp || (i > 0 && sc.comp[i] <= sc.comp[i - 1])) return false;
  }
  if (sc.ss == 0 ? sc.se != 0 : (sc.ncomp != 1 || sc.se < sc.ss || sc.se > 63)) return false;
  if (sc.al > 13 || (sc.ah != 0 && sc.al != sc.ah - 1)) return false;
  s->ncomp = sc.ncomp;
  s->ss = sc.ss;
  s->se = sc.se;
  s->ah = sc.ah;
  s->al = sc.al;
  for (int i = 0; i < 3; ++i) {
    const int c = i < sc.ncomp ? sc.comp[i] : 0;
    s->comp[i] = c;
    s->ch[i] = sc.ncomp > 1 ? g.ch[c] : 1;
    s->cv[i] = sc.ncomp > 1 ? g.cv[c] : 1;
  }
  if (sc.ncomp > 1) {
    s->mcus_x = g.mcus_x;
    s->n_mcus = g.n_mcus;
  } else {
    // not interleaved: the component's true block grid, not the padded one
    const int c = sc.comp[0];
    const int hmax = g.ch[0], vmax = g.cv[0];
    const int w = (d.width * g.ch[c] + hmax - 1) / hmax, h = (d.height * g.cv[c] + vmax - 1) / vmax;
    s->mcus_x = (w + 7) / 8;
    s->n_mcus = s->mcus_x * ((h + 7) / 8);
  }
  return true;
}

// Huffman tables the scan needs: one DC table per component for a DC-first scan, one AC table for an AC scan
JPEG_HD int jpeg_scan_tables(const asm_jpeg_scan& sc) {
  if (sc.ss > 0) return 1;
  return sc.ah != 0 ? 0 : sc.ncomp < 1 ? 0 : sc.ncomp > 3 ? 3 : sc.ncomp;
}

// A scan row of image `img` against the image's descriptor and the table sizes of the call, before anything it points to
// is read: 0 and *s filled, or ASM_JPEG_EDESC / ASM_JPEG_ERESTART.
JPEG_HD int jpeg_check_scan(const asm_jpeg_desc& d, const jpeg_geom& g, const asm_jpeg_scan& sc, int img, int n_huff,
                            int n_intervals_total, jpeg_scan_geom* s) {
  if (sc.image != img || !jpeg_make_scan_geom(d, g, sc, s)) return ASM_JPEG_EDESC;
  if (sc.restart_interval < 0 || sc.first_interval < 0 || sc.n_intervals < 1 ||
      sc.first_interval > n_intervals_total - sc.n_intervals)
    return ASM_JPEG_EDESC;
  if (sc.byte_begin < d.scan_offset || sc.byte_end < sc.byte_begin || sc.byte_end > d.scan_offset + d.scan_bytes)
    return ASM_JPEG_EDESC;
  const int n_tab = jpeg_scan_tables(sc);
  for (int i = 0; i < n_tab; ++i) {
    if (sc.huff[i] < 0 || sc.huff[i] >= n_huff) return ASM_JPEG_EDESC;
  }
  return sc.n_intervals == jpeg_expected_intervals(sc.restart_interval, s->n_mcus) ? 0 : ASM_JPEG_ERESTART;
}

// DC first: pred += EXTEND; coef[0] = pred * 2^al
JPEG_HD int jpeg_prog_dc_first(jpeg_bits* b, const jpeg_dtab* t, int al, int* pred, int16_t* out) {
  int diff;
  const int err = jpeg_decode_dc_diff(b, t, &diff);
  if (err) return err;
  *pred = (int16_t)(*pred + diff);
  out[0] = (int16_t)(*pred * (1 << al));
  return 0;
}

// DC refinement: one raw bit per block
JPEG_HD int jpeg_prog_dc_refine(jpeg_bits* b, int al, int16_t* out) {
  int err = 0;
  const int bit = jpeg_receive_bits(b, 1, &err);
  if (err) return err;
  if (bit) out[0] = (int16_t)(out[0] | (1 << al));
  return 0;
}

// AC first: band ss..se of one block, with end-of-band runs over blocks
JPEG_HD int jpeg_prog_ac_first(jpeg_bits* b, const jpeg_dtab* t, const uint8_t* zigzag, int ss, int se, int al, int* eobrun,
                               int16_t* out) {
  if (*eobrun > 0) {
    --*eobrun;
    return 0;
  }
  int err = 0;
  for (int k = ss; k <= se;) {
    const int rs = jpeg_decode_symbol(b, t, &err);
    if (rs < 0) return err;
    const int r = rs >> 4, s = rs & 15;
    if (s != 0) {
      k += r;
      if (k > se) return ASM_JPEG_EBADCODE;
      const int val = jpeg_receive_extend(b, s, &err);
      if (err) return err;
      out[zigzag[k]] = (int16_t)(val * (1 << al));
      ++k;
    } else if (r == 15) {
      k += 16;
    } else {
      *eobrun = (1 << r) - 1;
      if (r) *eobrun += jpeg_receive_bits(b, r, &err);
      return err;
    }
  }
  return 0;
}

// one correction bit for an already non-zero coefficient (T.81 G.1.2.3)
JPEG_HD void jpeg_prog_correct(jpeg_bits* b, int p1, int16_t* cp, int* err) {
  const int bit = jpeg_receive_bits(b, 1, err);
  const int v = *cp;
  if (bit && (v & p1) == 0) *cp = (int16_t)(v >= 0 ? v + p1 : v - p1);
}

// AC refinement: new coefficients of magnitude 2^al between correction bits for the ones already known
JPEG_HD int jpeg_prog_ac_refine(jpeg_bits* b, const jpeg_dtab* t, const uint8_t* zigzag, int ss, int se, int al,
                                int* eobrun, int16_t* out) {
  const int p1 = 1 << al;
  int err = 0;
  int k = ss;
  if (*eobrun == 0) {
    while (k <= se) {
      const int rs = jpeg_decode_symbol(b, t, &err);
      if (rs < 0) return err;
      int r = rs >> 4;
      const int s = rs & 15;
      int value = 0;
      if (s != 0) {
        if (s != 1) return ASM_JPEG_EBADCODE;
        value = jpeg_receive_bits(b, 1, &err) ? p1 : -p1;
        if (err) return err;
      } else if (r != 15) {
        *eobrun = 1 << r;
        if (r) *eobrun += jpeg_receive_bits(b, r, &err);
        if (err) return err;
        break;
      }
      // past r still-zero coefficients, correcting the non-zero ones on the way
      while (k <= se) {
        int16_t* cp = out + zigzag[k];
        if (*cp != 0) {
          jpeg_prog_correct(b, p1, cp, &err);
          if (err) return err;
        } else if (--r < 0) {
          break;
        }
        ++k;
      }
      if (value != 0) {
        if (k > se) return ASM_JPEG_EBADCODE;
        out[zigzag[k]] = (int16_t)value;
      }
      ++k;
    }
  }
  if (*eobrun > 0) {
    for (; k <= se; ++k) {
      int16_t* cp = out + zigzag[k];
      if (*cp != 0) {
        jpeg_prog_correct(b, p1, cp, &err);
        if (err) return err;
      }
    }
    --*eobrun;
  }
  return 0;
}

// Decode MCUs [first_mcu, first_mcu + n_mcus) (jpeg_check_interval passed them) of one scan from the bytes [begin, end)
// into coefs (the image's g.n_coefs int16).  tab[i]: scan component i's table (DC-first) or tab[0] (AC); none for a DC refinement.
JPEG_HD int jpeg_prog_decode_interval(const uint8_t* begin, const uint8_t* end, const jpeg_geom& g, const jpeg_scan_geom& s,
                                      const jpeg_dtab* tab, const uint8_t* zigzag, int first_mcu, int n_mcus,
                                      int16_t* coefs) {
  jpeg_bits b;
  jpeg_bits_init(&b, begin, end);
  int pred[3] = {0, 0, 0};
  int eobrun = 0;
  int my = first_mcu / s.mcus_x, mx = first_mcu - my * s.mcus_x;
  for (int m = 0; m < n_mcus; ++m) {
    for (int i = 0; i < s.ncomp; ++i) {
      const int c = s.comp[i];
      for (int v = 0; v < s.cv[i]; ++v) {
        for (int h = 0; h < s.ch[i]; ++h) {
          const int bx = mx * s.ch[i] + h;
          if (bx >= g.bw[c]) return ASM_JPEG_EDESC;
          const int64_t blk = (int64_t)(my * s.cv[i] + v) * g.bw[c] + bx;
          const int64_t at = g.base[c] + blk * 64;
          const int64_t stop = c + 1 < g.ncomp ? g.base[c + 1] : g.n_coefs;
          if (at < g.base[c] || at + 64 > stop) return ASM_JPEG_EDESC;
          int16_t* out = coefs + at;
          int err;
          if (s.ss == 0)
            err = s.ah == 0 ? jpeg_prog_dc_first(&b, &tab[i], s.al, &pred[i], out) : jpeg_prog_dc_refine(&b, s.al, out);
          else
            err = s.ah == 0 ? jpeg_prog_ac_first(&b, &tab[0], zigzag, s.ss, s.se, s.al, &eobrun, out)
                            : jpeg_prog_ac_refine(&b, &tab[0], zigzag, s.ss, s.se, s.al, &eobrun, out);
          if (err) return err;
        }
      }
    }
    if (++mx == s.mcus_x) {
      mx = 0;
      ++my;
    }
  }
  return 0;
}

// What lane `lane` of `lanes` does for scan row `sc` of image `img`: its share (k = lane, lane + lanes, ...) of the scan's
// rows of the interval table, each checked before a byte of it is read.  The caller has checked the scan row itself
// (jpeg_make_scan_geom, byte range inside the image's, first_interval + n_intervals in range, interval count).
JPEG_HD int jpeg_prog_decode_lane(const uint8_t* files, const jpeg_geom& g, const asm_jpeg_scan& sc, const jpeg_scan_geom& s,
                                  const asm_jpeg_interval* intervals, int img, const jpeg_dtab* tab, const uint8_t* zigzag,
                                  int lane, int lanes, int16_t* coefs) {
  int err = 0;
  for (int k = lane; k < sc.n_intervals && !err; k += lanes) {
    const asm_jpeg_interval iv = intervals[sc.first_interval + k];
    int first, count;
    // the row must lie in its scan row's bytes; the lane stops at its first error (the loop's condition)
    err = jpeg_check_interval(iv, k, sc.n_intervals, img, sc.restart_interval, s.n_mcus, sc.byte_begin, sc.byte_end, &first,
                              &count);
    if (!err) err = jpeg_prog_decode_interval(files + iv.byte_begin, files + iv.byte_end, g, s, tab, zigzag, first, count, coefs);
  }
  return err;
}
