// JPEG marker segments read on the device (ITU-T T.81 annex B): what jpeg.parse (progressive=False), _pack_sequential,
// _interval_rows and segment_table of assembled_cnn_amd/jpeg.py do for ONE file at buf[offset, offset + length), as plain
// functions shared by the kernels of jpeg_parse.hip and a host program (tools/probes/jpeg_parse_host.cpp, built with the
// address and undefined-behaviour sanitizers): the same text is compiled for both.  A function that takes `lane` is run by
// every lane of the 256-lane workgroup (a loop on the host); one that does not is lane 0's; between two of them the kernel
// has a barrier (the end of the loop on the host).
//
// Rules ("Headers on the device"):
//   header walk   SOI, fill bytes, marker segments with their length checks; DQT (8 bit, through the zig-zag, several per
//                 segment, a later table replaces an earlier one), DHT (count check, prefix-code check), SOF0 / SOF1, DRI,
//                 APP14 "Adobe", SOS; other APPn, COM and the reserved markers are skipped by length alone.
//   class         0 exactly where jpeg.parse neither raises nor sets `unsupported`; everything else is a non-zero set of
//                 ASM_JPEG_P* bits (diagnostics: the host parses such a file again and reports it in its own words), so
//                 the walk stops at the first thing that cannot be part of a class-0 file.
//   scan extent   ends at the first FF followed by none of 00, FF, D0..D7; fill FFs in front of that marker are trimmed; an
//                 FF as the last byte of the span is no marker; the marker must lead to EOI (possibly behind fill) and
//                 nothing behind EOI is read; a restart interval ends at every FF D0..D7.
// Safety: every read lies inside the span (never only inside the buffer), every table index inside its table, and every
// loop consumes a byte or ends.
//
// The walk reads through a window of JPP_WINDOW bytes that all lanes load with one 16-byte vector each; a step that needs
// bytes the window does not hold asks for a refill at its own position, and no step needs more than JPP_NEED bytes, so a
// refilled window always serves it.  The entropy-coded bytes are scanned 16 per lane per pass: each lane leaves a bit mask
// of the markers in its vector, lane 0 takes the marked lanes in order and carries the interval's first byte across lanes
// and passes.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/asm_hip.h"
#include "jpeg_entropy.h"      // JPEG_ZIGZAG_INIT

#if defined(__HIPCC__)
#define JPP_HD __host__ __device__ inline
#else
#define JPP_HD inline
#endif

#define JPP_LANES 256
#define JPP_WINDOW (16 * JPP_LANES)
#define JPP_NEED 320                              // marker + length + the largest item read at once (a DHT table: 273)
#define JPP_MAX_BYTES (((int64_t)1 << 40) - 1)
#define JPP_MAX_SIDE 8192                         // jpeg.MAX_SIDE

enum { JPP_REFILL = 0, JPP_SCAN = 1, JPP_END = 2 };                      // what jpp_walk returns
enum { JPP_M_SOI = 0, JPP_M_MARKER, JPP_M_FILL, JPP_M_CODE, JPP_M_DQT, JPP_M_DHT };  // where the walk stands

struct jpp_state {
  alignas(16) uint8_t win[JPP_WINDOW];     // span bytes [win_base, win_base + JPP_WINDOW), valid in [win_from, win_to)
  int64_t win_base, win_from, win_to, want;
  int64_t at, seg_end;                     // the walk: next byte, end of the DQT / DHT segment whose tables are being read
  int32_t mode, after_scan, ret, cls;
  // what the header defined
  uint16_t quant[4][64];                   // natural order
  asm_jpeg_huff huff[2][4];                // [class][id]
  uint32_t qdef, hdef[2];                  // bit id: defined
  int32_t sof, width, height, ncomp, hs, vs, dri, adobe;
  uint8_t cid[4], ch[4], cv[4], ctq[4], std[4], sta[4];
  uint8_t dcsel[4], acsel[4], dc_ids[2], ac_ids[2];
  int32_t n_dc, n_ac;
  // the scan
  int64_t scan_begin, scan_end, marker, iv_begin, n_iv, n_seg;
  int32_t scan_done, bad_rows;
  uint32_t word[JPP_LANES];                // bit j: RSTm at byte j of the lane's vector; bit 16 + j: another marker
  uint32_t rstv[JPP_LANES];                // the m of those RSTm, 3 bits each, in order
  uint64_t any[JPP_LANES / 64];            // bit l of [w]: word[64 w + l] != 0
};

// where the rows of one file go (asm_jpeg_parse_fill); null in asm_jpeg_parse, which only counts
struct jpp_rows {
  asm_jpeg_interval* intervals;            // the file's first row
  int32_t* segment_first;                  // its first entry; null when segment_bytes == 0
  int64_t n_intervals, n_segments;         // what the head row counted: nothing is written past them
  int64_t byte_shift;                      // position of the span in buf
  int32_t image, restart_interval;
  int64_t n_mcus, first_segment;
};

JPP_HD void jpp_init(jpp_state* s) {
  s->win_base = s->win_from = s->win_to = s->want = 0;
  s->at = s->seg_end = 0;
  s->mode = JPP_M_SOI;
  s->after_scan = s->ret = s->cls = 0;
  s->qdef = s->hdef[0] = s->hdef[1] = 0;
  s->sof = s->width = s->height = s->ncomp = s->dri = 0;
  s->hs = s->vs = 1;
  s->adobe = -1;
  s->n_dc = s->n_ac = 0;
  for (int c = 0; c < 4; ++c) s->cid[c] = s->ch[c] = s->cv[c] = s->ctq[c] = s->std[c] = s->sta[c] = s->dcsel[c] = s->acsel[c] = 0;
  s->scan_begin = s->scan_end = s->marker = s->iv_begin = s->n_iv = s->n_seg = 0;
  s->scan_done = s->bad_rows = 0;
}

// descriptor check without int64 overflow: [offset, offset + length) lies inside [0, buf_bytes)
JPP_HD bool jpp_span_ok(int64_t offset, int64_t length, int64_t buf_bytes) {
  return offset >= 0 && length >= 0 && offset <= buf_bytes && length <= buf_bytes - offset;
}

// One 16-byte vector of the address space, the bytes [vb, vb + 16) of the span, into dst: one aligned load where the whole
// vector lies in [from, to), single bytes (zero outside) where it does not.  `span + vb` is 16-byte aligned.
JPP_HD void jpp_load16(const uint8_t* span, int64_t vb, int64_t from, int64_t to, uint8_t* dst) {
  if (vb >= from && vb + 16 <= to) {
    memcpy(dst, __builtin_assume_aligned(span + vb, 16), 16);
    return;
  }
  for (int j = 0; j < 16; ++j) dst[j] = (vb + j >= from && vb + j < to) ? span[vb + j] : 0;
}

// every lane: the window at s->want (span bytes [0, n))
JPP_HD void jpp_load_window(jpp_state* s, const uint8_t* span, int64_t n, int lane) {
  const int64_t want = s->want;
  const int64_t base = want - (int64_t)((uintptr_t)(span + want) & 15u);
  jpp_load16(span, base + 16 * lane, 0, n, s->win + 16 * lane);
  if (lane == JPP_LANES - 1) {             // nobody reads these before the barrier
    s->win_base = base;
    s->win_from = base < 0 ? 0 : base;
    s->win_to = base + JPP_WINDOW < n ? base + JPP_WINDOW : n;
  }
}

JPP_HD int jpp_b(const jpp_state* s, int64_t pos) { return s->win[pos - s->win_base]; }
JPP_HD int jpp_u16(const jpp_state* s, int64_t pos) { return (jpp_b(s, pos) << 8) | jpp_b(s, pos + 1); }
JPP_HD int jpp_stop(jpp_state* s, int why) {
  s->cls |= why;
  return JPP_END;
}

// the classification of jpeg.parse behind its loop, made at SOS (nothing but EOI may follow the scan of a class-0 file, so
// every table is final there); also the Huffman slots of _pack_sequential.  false: not class 0.
JPP_HD bool jpp_classify(jpp_state* s) {
  if (s->height == 0 || s->width > JPP_MAX_SIDE || s->height > JPP_MAX_SIDE) return false;
  if (s->ncomp == 3) {
    if (s->adobe >= 0 && s->adobe != 1) return false;
    if (s->adobe < 0 && s->cid[0] == 'R' && s->cid[1] == 'G' && s->cid[2] == 'B') return false;
    if (s->ch[1] != 1 || s->cv[1] != 1 || s->ch[2] != 1 || s->cv[2] != 1) return false;
    const int h0 = s->ch[0], v0 = s->cv[0];
    if (!((h0 == 1 && v0 == 1) || (h0 == 2 && v0 == 1) || (h0 == 2 && v0 == 2))) return false;
    s->hs = h0;
    s->vs = v0;
  }
  s->n_dc = s->n_ac = 0;
  for (int c = 0; c < s->ncomp; ++c) {
    if (!((s->qdef >> s->ctq[c]) & 1u) || !((s->hdef[0] >> s->std[c]) & 1u) || !((s->hdef[1] >> s->sta[c]) & 1u)) return false;
    int d = 0, a = 0;
    while (d < s->n_dc && s->dc_ids[d] != s->std[c]) ++d;
    while (a < s->n_ac && s->ac_ids[a] != s->sta[c]) ++a;
    if (d == 2 || a == 2) return false;        // more than two DC or AC tables
    if (d == s->n_dc) s->dc_ids[s->n_dc++] = s->std[c];
    if (a == s->n_ac) s->ac_ids[s->n_ac++] = s->sta[c];
    s->dcsel[c] = (uint8_t)d;
    s->acsel[c] = (uint8_t)a;
  }
  return true;
}

// Lane 0: walk the marker segments from s->at for as long as the window serves.  JPP_REFILL: load the window at s->want
// and call again; JPP_SCAN: the SOS header is read and accepted, the entropy-coded bytes start at s->scan_begin; JPP_END:
// s->cls says what the file is (0 only behind the EOI that follows the scan).
JPP_HD int jpp_walk(jpp_state* s, int64_t n) {
  constexpr uint8_t zigzag[64] = JPEG_ZIGZAG_INIT;
  for (;;) {
    const int64_t at = s->at;
    if (at < n) {
      const int64_t need_to = n - at < JPP_NEED ? n : at + JPP_NEED;
      if (at < s->win_from || need_to > s->win_to) {
        s->want = at;
        return JPP_REFILL;
      }
    }
    switch (s->mode) {
      case JPP_M_SOI:
        if (n < 2 || jpp_b(s, 0) != 0xFF || jpp_b(s, 1) != 0xD8) return jpp_stop(s, ASM_JPEG_PNOTJPEG);
        s->at = 2;
        s->mode = JPP_M_MARKER;
        break;
      case JPP_M_MARKER:
        if (at >= n) return jpp_stop(s, s->after_scan ? ASM_JPEG_PNOEOI : ASM_JPEG_PHEADER);
        if (jpp_b(s, at) != 0xFF) return jpp_stop(s, ASM_JPEG_PHEADER);
        s->mode = JPP_M_FILL;
        break;
      case JPP_M_FILL: {
        int64_t p = at;
        while (p < s->win_to && jpp_b(s, p) == 0xFF) ++p;
        s->at = p;
        if (p >= n) return jpp_stop(s, ASM_JPEG_PHEADER);          // truncated marker
        if (p < s->win_to) s->mode = JPP_M_CODE;                   // else: more fill may follow, behind a refill
        break;
      }
      case JPP_M_CODE: {
        const int m = jpp_b(s, at);
        const int64_t pos = at + 1;
        if (s->after_scan) return m == 0xD9 ? JPP_END : jpp_stop(s, ASM_JPEG_PKIND);   // more scans, tables, DNL
        if (m == 0xD9 || m == 0xD8 || m == 0x01 || m == 0x00 || (m >= 0xD0 && m <= 0xD7)) return jpp_stop(s, ASM_JPEG_PHEADER);
        if (pos + 2 > n) return jpp_stop(s, ASM_JPEG_PHEADER);
        const int seglen = jpp_u16(s, pos);
        if (seglen < 2 || seglen > n - pos) return jpp_stop(s, ASM_JPEG_PHEADER);
        const int64_t body = pos + 2, end = pos + seglen;
        const int size = seglen - 2;
        s->at = end;
        s->mode = JPP_M_MARKER;
        if (m == 0xDB || m == 0xC4) {
          s->at = body;
          s->seg_end = end;
          s->mode = m == 0xDB ? JPP_M_DQT : JPP_M_DHT;
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8 && m != 0xCC) {      // SOFn
          if (s->sof || size < 6) return jpp_stop(s, ASM_JPEG_PHEADER);
          const int precision = jpp_b(s, body), ncomp = jpp_b(s, body + 5);
          s->sof = m;
          s->height = jpp_u16(s, body + 1);
          s->width = jpp_u16(s, body + 3);
          if (size != 6 + 3 * ncomp || ncomp == 0 || s->width == 0) return jpp_stop(s, ASM_JPEG_PHEADER);
          if (ncomp != 1 && ncomp != 3) return jpp_stop(s, ASM_JPEG_PKIND);   // or a header the host refuses: not class 0
          s->ncomp = ncomp;
          for (int c = 0; c < ncomp; ++c) {
            const int hv = jpp_b(s, body + 7 + 3 * c), tq = jpp_b(s, body + 8 + 3 * c);
            if ((hv >> 4) < 1 || (hv >> 4) > 4 || (hv & 15) < 1 || (hv & 15) > 4 || tq > 3) return jpp_stop(s, ASM_JPEG_PHEADER);
            s->cid[c] = (uint8_t)jpp_b(s, body + 6 + 3 * c);
            s->ch[c] = (uint8_t)(hv >> 4);
            s->cv[c] = (uint8_t)(hv & 15);
            s->ctq[c] = (uint8_t)tq;
            for (int o = 0; o < c; ++o)
              if (s->cid[o] == s->cid[c]) return jpp_stop(s, ASM_JPEG_PHEADER);
          }
          if ((m != 0xC0 && m != 0xC1) || precision != 8) return jpp_stop(s, ASM_JPEG_PKIND);
        } else if (m == 0xCC || m == 0xDC) {                                 // DAC, DNL
          return jpp_stop(s, ASM_JPEG_PKIND);
        } else if (m == 0xDD) {                                              // DRI
          if (size != 2) return jpp_stop(s, ASM_JPEG_PHEADER);
          s->dri = jpp_u16(s, body);
        } else if (m == 0xEE) {                                              // APP14
          if (size >= 12 && jpp_b(s, body) == 'A' && jpp_b(s, body + 1) == 'd' && jpp_b(s, body + 2) == 'o' &&
              jpp_b(s, body + 3) == 'b' && jpp_b(s, body + 4) == 'e')
            s->adobe = jpp_b(s, body + 11);
        } else if (m == 0xDA) {                                              // SOS
          if (!s->sof || size < 1 || size != 4 + 2 * jpp_b(s, body)) return jpp_stop(s, ASM_JPEG_PHEADER);
          if (jpp_b(s, body) != s->ncomp) return jpp_stop(s, ASM_JPEG_PKIND);   // several scans, or an unknown component
          for (int c = 0; c < s->ncomp; ++c) {
            const int cs = jpp_b(s, body + 1 + 2 * c), t = jpp_b(s, body + 2 + 2 * c);
            if ((t >> 4) > 3 || (t & 15) > 3) return jpp_stop(s, ASM_JPEG_PHEADER);
            if (cs != s->cid[c]) return jpp_stop(s, ASM_JPEG_PKIND);         // out of frame order, or unknown
            s->std[c] = (uint8_t)(t >> 4);
            s->sta[c] = (uint8_t)(t & 15);
          }
          if (!jpp_classify(s)) return jpp_stop(s, ASM_JPEG_PKIND);
          s->scan_begin = s->iv_begin = end;
          return JPP_SCAN;
        }
        break;
      }
      case JPP_M_DQT: {
        if (at >= s->seg_end) {
          s->at = s->seg_end;
          s->mode = JPP_M_MARKER;
          break;
        }
        const int pq = jpp_b(s, at) >> 4, tq = jpp_b(s, at) & 15;
        if (tq > 3 || pq > 1 || at + 1 + 64 * (pq + 1) > s->seg_end) return jpp_stop(s, ASM_JPEG_PHEADER);
        if (pq == 1) return jpp_stop(s, ASM_JPEG_PKIND);                     // 16-bit quantisation table
        for (int k = 0; k < 64; ++k) s->quant[tq][zigzag[k]] = (uint16_t)jpp_b(s, at + 1 + k);
        s->qdef |= 1u << tq;
        s->at = at + 65;
        break;
      }
      case JPP_M_DHT: {
        if (at >= s->seg_end) {
          s->at = s->seg_end;
          s->mode = JPP_M_MARKER;
          break;
        }
        const int tc = jpp_b(s, at) >> 4, th = jpp_b(s, at) & 15;
        if (tc > 1 || th > 3 || at + 17 > s->seg_end) return jpp_stop(s, ASM_JPEG_PHEADER);
        int cnt = 0, code = 0;
        bool prefix = true;
        for (int l = 0; l < 16; ++l) {
          const int b = jpp_b(s, at + 1 + l);
          cnt += b;
          code = (code + b) << 1;                                            // < 2^25: 16 counts of at most 255
          prefix = prefix && code <= (2 << (l + 1));
        }
        if (cnt > 256 || at + 17 + cnt > s->seg_end || !prefix) return jpp_stop(s, ASM_JPEG_PHEADER);
        asm_jpeg_huff* h = &s->huff[tc][th];
        for (int l = 0; l < 16; ++l) h->bits[l] = (uint8_t)jpp_b(s, at + 1 + l);
        for (int k = 0; k < 256; ++k) h->vals[k] = k < cnt ? (uint8_t)jpp_b(s, at + 17 + k) : 0;
        s->hdef[tc] |= 1u << th;
        s->at = at + 17 + cnt;
        break;
      }
      default:
        return jpp_stop(s, ASM_JPEG_PHEADER);
    }
  }
}

// segments of an interval of `size` bytes (segment_table of jpeg.py); 0 without a segment table
JPP_HD int64_t jpp_segments(int64_t size, int segment_bytes) {
  if (segment_bytes <= 0) return 0;
  const int64_t k = (size + segment_bytes - 1) / segment_bytes;
  return k < 1 ? 1 : k;
}

// Lane 0: the interval [s->iv_begin, end) is complete and `rst` (-1: none) ends it.  Counts it and, with `out`, writes its
// row and its segment entry by _interval_rows' arithmetic -- unless the head row counted fewer: then nothing is written.
JPP_HD void jpp_close_interval(jpp_state* s, int64_t end, int rst, int segment_bytes, const jpp_rows* out) {
  const int64_t segs = jpp_segments(end - s->iv_begin, segment_bytes);
  if (out) {
    if (s->n_iv < out->n_intervals && segs <= out->n_segments - s->n_seg && end >= s->iv_begin) {
      asm_jpeg_interval row;
      const int64_t ri = out->restart_interval, first = s->n_iv * ri, left = out->n_mcus - first;
      row.image = out->image;
      row.first_mcu = ri ? (int32_t)(first < 2147483647 ? first : 2147483647) : 0;
      row.n_mcus = ri ? (int32_t)(left > ri ? ri : left < -2147483647 - 1 ? -2147483647 - 1 : left) : (int32_t)out->n_mcus;
      row.rst = rst;
      row.byte_begin = s->iv_begin + out->byte_shift;
      row.byte_end = end + out->byte_shift;
      out->intervals[s->n_iv] = row;
      if (out->segment_first) out->segment_first[s->n_iv] = (int32_t)(out->first_segment + s->n_seg);
    } else {
      s->bad_rows = 1;
    }
  }
  ++s->n_iv;
  s->n_seg += segs;
}

// The pass that holds span byte `pos`: passes are JPP_WINDOW bytes of the address space, 16-byte aligned.
JPP_HD int64_t jpp_pass_base(const uint8_t* span, int64_t pos) { return pos - (int64_t)((uintptr_t)(span + pos) & 15u); }

// Every lane: the markers among the 16 bytes [pass_base + 16 lane, + 16) of the entropy-coded bytes [s->scan_begin, limit):
// a pair FF xx counts where both bytes lie below `limit`.  Returns whether the lane found any (the kernel makes s->any of
// it with a ballot, the host program with jpp_mark).
JPP_HD bool jpp_scan_lane(jpp_state* s, const uint8_t* span, int64_t limit, int64_t pass_base, int lane) {
  const int64_t vb = pass_base + 16 * lane;
  const int64_t lo = vb > s->scan_begin ? vb : s->scan_begin, hi = vb + 16 < limit - 1 ? vb + 16 : limit - 1;
  uint32_t word = 0, vals = 0;
  if (lo < hi) {
    uint8_t b[17];
    jpp_load16(span, vb, s->scan_begin, limit, b);
    b[16] = vb + 16 < limit ? span[vb + 16] : 0;
    int k = 0;
    for (int j = 0; j < 16; ++j) {
      if (vb + j < lo || vb + j >= hi || b[j] != 0xFF) continue;
      const int c = b[j + 1];
      if (c >= 0xD0 && c <= 0xD7) {
        word |= 1u << j;
        vals |= (uint32_t)(c - 0xD0) << (3 * k++);
      } else if (c != 0x00 && c != 0xFF) {
        word |= 1u << (16 + j);
      }
    }
  }
  s->word[lane] = word;
  s->rstv[lane] = vals;
  return word != 0;
}

// host form of the ballot: the lanes run in order, the first of each group of 64 clears the group's word
JPP_HD void jpp_mark(jpp_state* s, int lane, bool any) {
  if ((lane & 63) == 0) s->any[lane >> 6] = 0;
  if (any) s->any[lane >> 6] |= (uint64_t)1 << (lane & 63);
}

JPP_HD int jpp_ctz64(uint64_t v) {
  int k = 0;
  while (!(v & 1u)) {
    v >>= 1;
    ++k;
  }
  return k;
}

// Lane 0: the marked lanes of one pass in order.  An RSTm closes the interval that s->iv_begin opened; another marker ends
// the scan (s->marker; s->scan_end in front of its fill bytes), closes the last interval and sets s->scan_done.
JPP_HD void jpp_scan_combine(jpp_state* s, const uint8_t* span, int64_t pass_base, int segment_bytes, const jpp_rows* out) {
  for (int w = 0; w < JPP_LANES / 64 && !s->scan_done; ++w) {
    uint64_t lanes = s->any[w];
    while (lanes && !s->scan_done) {
      const int lane = 64 * w + jpp_ctz64(lanes);
      lanes &= lanes - 1;
      const uint32_t word = s->word[lane], vals = s->rstv[lane];
      uint32_t bits = (word | (word >> 16)) & 0xFFFFu;
      int k = 0;
      while (bits) {
        const int j = jpp_ctz64(bits);
        bits &= bits - 1;
        const int64_t q = pass_base + 16 * lane + j;
        if ((word >> 16) & (1u << j)) {
          int64_t e = q;
          while (e > s->iv_begin && span[e - 1] == 0xFF) --e;     // fill bytes in front of the marker
          s->marker = q;
          s->scan_end = e;
          jpp_close_interval(s, e, -1, segment_bytes, out);
          s->scan_done = 1;
          break;
        }
        jpp_close_interval(s, q, (int)((vals >> (3 * k++)) & 7u), segment_bytes, out);
        s->iv_begin = q + 2;
      }
    }
  }
}

// Lane 0, behind a scan that found its end: the walk goes on at the marker, which must lead to EOI
JPP_HD void jpp_after_scan(jpp_state* s) {
  s->at = s->marker;
  s->mode = JPP_M_MARKER;
  s->after_scan = 1;
}

// Lane 0: the head row
JPP_HD void jpp_head(const jpp_state* s, asm_jpeg_head* h) {
  asm_jpeg_head r;
  memset(&r, 0, sizeof r);
  r.cls = s->cls;
  if (s->cls == 0) {
    r.width = s->width;
    r.height = s->height;
    r.ncomp = s->ncomp;
    r.hs = s->hs;
    r.vs = s->vs;
    r.restart_interval = s->dri;
    r.n_intervals = (int32_t)s->n_iv;
    r.scan_begin = s->scan_begin;
    r.scan_bytes = s->scan_end - s->scan_begin;
    r.n_segments = s->n_seg;
    for (int c = 0; c < s->ncomp; ++c) {
      r.qsel[c] = s->ctq[c];
      r.dcsel[c] = s->dcsel[c];
      r.acsel[c] = s->acsel[c];
    }
  }
  *h = r;
}

// Every lane: the table block as _pack_sequential fills it -- every defined quantisation table, the Huffman tables the
// scan names in slots of first use, zero elsewhere and all zero for a file of another class -- as 32-bit words.
JPP_HD void jpp_tables(const jpp_state* s, uint32_t* out, int lane) {
  for (int i = lane; i < (int)(sizeof(asm_jpeg_tables) / 4); i += JPP_LANES) {
    uint32_t v = 0;
    if (s->cls == 0) {
      if (i < 128) {
        const int tq = i / 32;
        if ((s->qdef >> tq) & 1u) v = (uint32_t)s->quant[tq][2 * (i % 32)] | ((uint32_t)s->quant[tq][2 * (i % 32) + 1] << 16);
      } else {
        const int t = (i - 128) / 68, r = 4 * ((i - 128) % 68), cls = t >> 1, slot = t & 1;   // 272 bytes a table
        if (slot < (cls ? s->n_ac : s->n_dc)) {
          const asm_jpeg_huff* h = &s->huff[cls][cls ? s->ac_ids[slot] : s->dc_ids[slot]];
          const uint8_t* p = r < 16 ? h->bits + r : h->vals + (r - 16);
          v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        }
      }
    }
    out[i] = v;
  }
}

// Lane 0 of asm_jpeg_parse_fill: the descriptor row of a class-0 head row (geometry as jpeg.parse derives it)
JPP_HD void jpp_desc(const asm_jpeg_head& h, int64_t span_offset, const asm_jpeg_place& p, asm_jpeg_desc* d) {
  asm_jpeg_desc r;
  memset(&r, 0, sizeof r);
  r.scan_offset = span_offset + h.scan_begin;
  r.scan_bytes = h.scan_bytes;
  r.coef_offset = r.plane_offset = p.coef_offset;
  r.dst_offset = p.dst_offset;
  r.width = h.width;
  r.height = h.height;
  r.ncomp = h.ncomp;
  r.hs = h.hs;
  r.vs = h.vs;
  r.mcus_x = (h.width + 8 * h.hs - 1) / (8 * h.hs);
  r.mcus_y = (h.height + 8 * h.vs - 1) / (8 * h.vs);
  r.restart_interval = h.restart_interval;
  r.first_interval = p.first_interval;
  r.n_intervals = h.n_intervals;
  for (int c = 0; c < 4; ++c) {
    r.qsel[c] = h.qsel[c];
    r.dcsel[c] = h.dcsel[c];
    r.acsel[c] = h.acsel[c];
  }
  *d = r;
}

// a head row asm_jpeg_parse_fill can trust to describe bytes of its span: what asm_jpeg_parse writes for class 0
JPP_HD bool jpp_head_ok(const asm_jpeg_head& h, int64_t span_length) {
  return h.cls == 0 && h.width >= 1 && h.width <= JPP_MAX_SIDE && h.height >= 1 && h.height <= JPP_MAX_SIDE &&
         (h.ncomp == 1 || h.ncomp == 3) && h.hs >= 1 && h.hs <= 2 && h.vs >= 1 && h.vs <= 2 && h.restart_interval >= 0 &&
         h.n_intervals >= 1 && h.n_segments >= 0 && h.scan_begin >= 0 && h.scan_bytes >= 0 && h.scan_begin <= span_length &&
         h.scan_bytes <= span_length - h.scan_begin;
}
