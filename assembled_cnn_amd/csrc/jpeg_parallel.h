// Segment-parallel entropy decode of sequential (SOF0 / SOF1) scans ("one scan on many lanes"): every
// restart interval is cut into segments of `segment_bytes` raw file bytes, all lanes of a workgroup decode segments at
// once from guessed states, and because Huffman codes resynchronise by themselves (Klein & Wiseman 2003; Weissenberger &
// Schmidt 2018, 2021) the guesses fall onto the true decoder's states after a few rounds.  Included by jpeg_entropy.h;
// the functions below take (lane, lanes) so that the kernel (jpeg.hip, one call per lane between barriers) and the host
// program (tools/probes/jpeg_parallel_host.cpp, lanes simulated by a loop, address + undefined-behaviour sanitizers)
// compile the same text.
//
// State of a decoder between two symbols: (raw bit position, k, block-in-MCU).  The position counts the file's own
// stuffed bytes from the start of `files` and is normalised: it never names a stuffing 00.  k is the zig-zag index of the
// next AC coefficient, 0 when a DC symbol comes next.  The DC predictor is NOT part of the state: the write phase stores
// differences and a prefix sum per component turns them into values.
//
// Phases of one image (every lane-function is followed by a workgroup barrier):
//   jpeg_par_check_table   the image's rows of the segment table against the sizes of the call
//   jpeg_par_init          one state row per segment: the true entry for the first of an interval, a guess for the others;
//                          the interval's row is judged by jpeg_check_interval, the sequential decoder's own check
//   jpeg_par_decode /      a round: every segment whose entry changed is decoded from it, symbols only, up to the first
//   jpeg_par_publish       symbol that starts at or after its end (exit state + blocks started); then every exit that is
//                          no error and differs from the next entry replaces it.  Repeat until nothing was published.
//   jpeg_par_chain_sum /   per interval: segment j + 1 is valid when j is valid, ended without error and its exit equals
//   jpeg_par_chain_apply   j + 1's entry; the ordinal of a valid segment's first block is the sum of the counts before it
//   jpeg_par_write         every valid segment once more, storing AC coefficients and DC differences; only this ORs errors
//   jpeg_par_dc_sum /      DC values: per-component prefix sums over contiguous MCU runs, restarted at interval starts
//   jpeg_par_dc_apply
// Symbols are decoded by jpeg_decode_dc_diff / jpeg_decode_ac_step, the sequential decoder's own step: the status words agree.
// Safety: the rules of jpeg_entropy.h.  Bytes are read inside the interval's range only, every block ordinal becomes an
// address through jpeg_par_block_at (checked against the geometry), every loop consumes a bit per iteration or ends.
// The state rows are untrusted (jpeg_par_segment_range): whatever they hold, every table index is bounded by the
// image's own interval count, every byte range is a checked interval row's, and every state by that range.
#pragma once

#define JPEG_SEG_DIRTY 1       // the entry changed since the segment's last decode
#define JPEG_SEG_FIRST 2       // first segment of its interval: the entry is the truth
#define JPEG_SEG_LAST 4        // last segment of its interval: no end bound, nothing to publish
#define JPEG_SEG_DEAD 8        // its interval's row was refused (ASM_JPEG_EDESC / ASM_JPEG_ERESTART): never decoded
#define JPEG_SEG_NOEXIT (~0ull)
#define JPEG_SEG_COUNT_CAP (1 << 30)

// one row of the state region (asm_jpeg_decode_parallel's workspace, after coefficients and planes)
struct jpeg_seg {
  uint64_t entry, exit;        // packed states; exit of the last decode from `entry`, JPEG_SEG_NOEXIT after an error
  int32_t interval;            // index among the image's intervals
  int32_t count;               // blocks that started in the segment, last decode
  int32_t ordinal;             // scan-order index inside the interval of its first block, -1: not valid
  int32_t flags;
};

JPEG_HD uint64_t jpeg_seg_pack(int64_t pos, int k, int blk) {
  return ((uint64_t)pos << 16) | ((uint64_t)k << 8) | (uint64_t)blk;
}

// what a lane needs to know about the image; segs points at the image's first state row
struct jpeg_par_ctx {
  const uint8_t* files;
  asm_jpeg_desc d;
  jpeg_geom g;
  int bpm;                     // blocks per MCU
  const asm_jpeg_interval* intervals;      // the image's first row
  const int32_t* seg_first;    // the image's first row of the segment table
  int img;
  int segment_bytes;
  jpeg_seg* segs;
  int n_segs;
  const jpeg_dtab* tab;        // dc 0, dc 1, ac 0, ac 1
  const uint8_t* zigzag;
  int16_t* coefs;
};

// everything of the context but the descriptor and the geometry (filled first: bpm reads them) and the state rows, which
// are set once jpeg_par_check_table has passed
JPEG_HD void jpeg_par_ctx_fill(jpeg_par_ctx* c, const uint8_t* files, const asm_jpeg_interval* intervals, const int32_t* seg_first,
                               int img, int segment_bytes, const jpeg_dtab* tab, const uint8_t* zigzag, int16_t* coefs) {
  c->files = files;
  c->bpm = c->d.ncomp == 1 ? 1 : c->d.hs * c->d.vs + 2;
  c->intervals = intervals;
  c->seg_first = seg_first;
  c->img = img;
  c->segment_bytes = segment_bytes;
  c->tab = tab;
  c->zigzag = zigzag;
  c->coefs = coefs;
  c->segs = nullptr;
  c->n_segs = 0;
}

// segments of an interval row: ceil(bytes / segment_bytes), at least one
JPEG_HD int64_t jpeg_par_interval_segments(const asm_jpeg_interval& iv, int segment_bytes) {
  const int64_t bytes = iv.byte_end - iv.byte_begin;
  return bytes > segment_bytes ? (bytes + segment_bytes - 1) / segment_bytes : 1;
}

// The image's rows of the segment table: row k names the first state row of interval k, the rows of one image follow
// each other without a gap, and all of them lie inside [0, total_segments).  true: this lane saw a violation.
JPEG_HD bool jpeg_par_check_table(const jpeg_par_ctx& c, int64_t total_segments, int lane, int lanes) {
  bool bad = false;
  for (int k = lane; k < c.d.n_intervals; k += lanes) {
    const int64_t at = c.seg_first[k], n = jpeg_par_interval_segments(c.intervals[k], c.segment_bytes);
    if (at < 0 || n > total_segments - at) bad = true;
    else if (k + 1 < c.d.n_intervals && c.seg_first[k + 1] != at + n) bad = true;
  }
  return bad;
}

// state rows of the image once jpeg_par_check_table has passed on every lane
JPEG_HD int jpeg_par_segments(const jpeg_par_ctx& c) {
  const int last = c.d.n_intervals - 1;
  return (int)(c.seg_first[last] + jpeg_par_interval_segments(c.intervals[last], c.segment_bytes) - c.seg_first[0]);
}

// State row `row` (a copy) of segment s, judged before anything it names is used.  The state region is NOT trusted: a
// segment table in which two images share rows lets another workgroup write into this image's rows at any time, so a
// row's interval index, flags and states are data like the file's bytes.  false: the row names no interval of this
// image, its interval's row of the interval table is refused (jpeg_check_interval), or s is no segment of that
// interval.  Else *iv is the checked interval row, [iv->byte_begin, *end) what the segment may cover (*end is the
// segment's end, the interval's for its last segment, *last), *first_mcu / *n_mcus the interval's MCUs.
JPEG_HD bool jpeg_par_segment_range(const jpeg_par_ctx& c, int s, const jpeg_seg& row, asm_jpeg_interval* iv, int64_t* end,
                                    bool* last, int* first_mcu, int* n_mcus) {
  if (row.interval < 0 || row.interval >= c.d.n_intervals) return false;
  *iv = c.intervals[row.interval];
  if (jpeg_check_interval(*iv, row.interval, c.d.n_intervals, c.img, c.d.restart_interval, c.g.n_mcus, c.d.scan_offset,
                          c.d.scan_offset + c.d.scan_bytes, first_mcu, n_mcus))
    return false;
  const int64_t j = s - (int64_t)(c.seg_first[row.interval] - c.seg_first[0]);
  const int64_t n = jpeg_par_interval_segments(*iv, c.segment_bytes);
  if (j < 0 || j >= n) return false;
  *last = j == n - 1;
  *end = *last ? iv->byte_end : iv->byte_begin + (j + 1) * c.segment_bytes;
  return true;
}

// the image's state rows lane, lane + lanes, ...; returns the ASM_JPEG_E* of the interval rows it refused
JPEG_HD int jpeg_par_init(const jpeg_par_ctx& c, int lane, int lanes) {
  int err = 0;
  for (int s = lane; s < c.n_segs; s += lanes) {
    // the interval of segment s: the last row whose first segment is <= s (the rows increase: jpeg_par_check_table)
    int lo = 0, hi = c.d.n_intervals - 1;
    const int64_t want = (int64_t)c.seg_first[0] + s;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (c.seg_first[mid] <= want) lo = mid;
      else hi = mid - 1;
    }
    const asm_jpeg_interval iv = c.intervals[lo];
    const int64_t j = want - c.seg_first[lo], n = jpeg_par_interval_segments(iv, c.segment_bytes);
    int first_mcu, n_mcus;
    // the row against the descriptor's scan, as jpeg_decode_lane judges it
    const int row_err = jpeg_check_interval(iv, lo, c.d.n_intervals, c.img, c.d.restart_interval, c.g.n_mcus, c.d.scan_offset,
                                            c.d.scan_offset + c.d.scan_bytes, &first_mcu, &n_mcus);
    jpeg_seg row;
    row.interval = lo;
    row.count = 0;
    row.ordinal = -1;
    row.exit = JPEG_SEG_NOEXIT;
    row.flags = (j == 0 ? JPEG_SEG_FIRST : 0) | (j == n - 1 ? JPEG_SEG_LAST : 0);
    row.entry = 0;
    if (row_err) {      // a refused row is ORed in and its segments are marked dead: never decoded
      err |= row_err;
      row.flags |= JPEG_SEG_DEAD;
    } else {
      int64_t o = iv.byte_begin + j * c.segment_bytes;
      // a segment that starts behind an FF on a 00 starts on stuffing
      if (j > 0 && c.files[o - 1] == 0xFF && c.files[o] == 0x00) ++o;
      row.entry = jpeg_seg_pack(o * 8, 0, 0);
      if (!(row.flags & JPEG_SEG_LAST)) row.flags |= JPEG_SEG_DIRTY;
    }
    c.segs[s] = row;
  }
  return err;
}

// Bit reader that knows the raw position of its next unread bit: jpeg_bits plus, for each of the (at most eight) bytes in
// buf, whether a stuffing 00 followed it in the file (sm, newest byte in bit 0), and where the data ended.
struct jpeg_pbits {
  jpeg_bits b;
  const uint8_t* stop;         // once b.done: the FF of the marker that ended the data, or the end of the interval
  uint32_t sm;
};

JPEG_HD void jpeg_pbits_fill(jpeg_pbits* r) {
  jpeg_bits* b = &r->b;
  while (b->n <= 56) {
    int v = -1;
    uint32_t stuffed = 0;
    if (!b->done) {
      v = jpeg_next_byte(b);
      if (v < 0) {
        r->stop = b->end;
      } else if (v == 0xFF) {
        const uint8_t* ff = b->p - b->wn - 1;
        if (jpeg_next_byte(b) == 0) {
          stuffed = 1;
        } else {
          v = -1;
          r->stop = ff;
        }
      }
    }
    if (v < 0) {
      b->done = true;
      b->pad += 8;
      v = 0;
    }
    b->buf = (b->buf << 8) | (uint64_t)v;
    r->sm = (r->sm << 1) | stuffed;
    b->n += 8;
  }
}

// first raw byte the reader has not taken into buf
JPEG_HD const uint8_t* jpeg_pbits_next(const jpeg_pbits* r) { return r->b.done ? r->stop : r->b.p - r->b.wn; }

// raw position of the next unread bit (bits from `files`); meaningful while no pad bit has been consumed
JPEG_HD int64_t jpeg_pbits_pos(const jpeg_pbits* r, const uint8_t* files) {
  const int real = r->b.n - r->b.pad;
  const int held = (r->b.n + 7) >> 3;
  const int raw = ((real + 7) >> 3) + __builtin_popcount(r->sm & ((1u << held) - 1u));
  return (int64_t)(jpeg_pbits_next(r) - files - raw) * 8 + ((-real) & 7);
}

// address (in the image's coefficients) of block `ordinal` of the interval that starts at first_mcu; -1: outside the
// geometry.  *comp: its component.
JPEG_HD int64_t jpeg_par_block_at(const jpeg_geom& g, int bpm, int first_mcu, int64_t ordinal, int* comp) {
  if (ordinal < 0) return -1;
  const int64_t m = first_mcu + ordinal / bpm;
  const int rem = (int)(ordinal % bpm);
  if (m >= g.n_mcus) return -1;
  const int n0 = g.ch[0] * g.cv[0];
  const int c = rem < n0 ? 0 : rem - n0 + 1;
  const int v = c == 0 ? rem / g.ch[0] : 0, h = c == 0 ? rem - v * g.ch[0] : 0;
  const int my = (int)(m / g.mcus_x), mx = (int)(m - (int64_t)my * g.mcus_x);
  const int64_t blk = (int64_t)(my * g.cv[c] + v) * g.bw[c] + (mx * g.ch[c] + h);
  const int64_t at = g.base[c] + blk * 64;
  if (c >= g.ncomp || at < 0 || at + 64 > g.n_coefs) return -1;
  *comp = c;
  return at;
}

// Decode from `entry` up to the first symbol that starts at or after raw byte seg_end (bounded = false: no end bound),
// reading no byte outside [iv_begin, iv_end).  coefs == nullptr: symbols only.  Else AC coefficients and DC differences are
// stored, `ordinal` is the interval-relative index of the first block that STARTS here (a block in progress at the entry
// is ordinal - 1) and the decode stops in front of block `total`.  *exit: the state it stopped in; *started: blocks
// whose DC symbol was decoded.  Returns 0 or ASM_JPEG_E*, the word jpeg_decode_interval returns for the same bits.
JPEG_HD int jpeg_par_decode_segment(const jpeg_par_ctx& c, int64_t iv_begin, int64_t iv_end, int64_t seg_end, bool bounded,
                                    uint64_t entry, int16_t* coefs, int first_mcu, int64_t ordinal, int64_t total, uint64_t* exit,
                                    int* started) {
  const jpeg_dtab* dc[3] = {&c.tab[c.d.dcsel[0] & 1], &c.tab[c.d.dcsel[1] & 1], &c.tab[c.d.dcsel[2] & 1]};
  const jpeg_dtab* ac[3] = {&c.tab[2 + (c.d.acsel[0] & 1)], &c.tab[2 + (c.d.acsel[1] & 1)], &c.tab[2 + (c.d.acsel[2] & 1)]};
  int64_t pos = (int64_t)(entry >> 16);
  int k = (int)(entry >> 8) & 255, blk = (int)entry & 255;
  *exit = JPEG_SEG_NOEXIT;
  *started = 0;
  if (k > 63 || blk >= c.bpm || pos < iv_begin * 8 || (pos >> 3) > iv_end) return ASM_JPEG_EDESC;
  // bytes behind the interval's last block: the sequential decoder never looks at them
  if (coefs && ordinal - (k != 0 ? 1 : 0) >= total) return 0;
  jpeg_pbits r;
  jpeg_bits_init(&r.b, c.files + (pos >> 3), c.files + iv_end);
  r.stop = c.files + iv_end;
  r.sm = 0;
  jpeg_pbits_fill(&r);
  r.b.n -= (int)(pos & 7);
  if (r.b.n < r.b.pad) return ASM_JPEG_EOVERRUN;       // a guess inside a marker: no true decoder stands there
  const int n0 = c.g.ch[0] * c.g.cv[0];
  int comp = blk < n0 ? 0 : blk - n0 + 1;
  int16_t* out = nullptr;
  if (coefs && k != 0) {
    const int64_t at = jpeg_par_block_at(c.g, c.bpm, first_mcu, ordinal - 1, &comp);
    if (at < 0) return ASM_JPEG_EDESC;
    out = coefs + at;
  }
  const uint8_t* seg_stop = c.files + seg_end;
  int n = 0;
  for (;;) {
    if (r.b.n < 32) jpeg_pbits_fill(&r);
    if (bounded && jpeg_pbits_next(&r) >= seg_stop && jpeg_pbits_pos(&r, c.files) >= seg_end * 8) break;
    if (k == 0) {
      if (coefs) {
        if (ordinal + n >= total) break;
        const int64_t at = jpeg_par_block_at(c.g, c.bpm, first_mcu, ordinal + n, &comp);
        if (at < 0) return ASM_JPEG_EDESC;
        out = coefs + at;
      } else {
        comp = blk < n0 ? 0 : blk - n0 + 1;
      }
      int diff;
      const int err = jpeg_decode_dc_diff(&r.b, dc[comp], &diff);
      if (err) return err;
      if (out) out[0] = (int16_t)diff;      // the difference: jpeg_par_dc_* turn it into the value
      ++n;
      k = 1;
    } else {
      const int err = jpeg_decode_ac_step(&r.b, ac[comp], c.zigzag, &k, out);
      if (err) return err;
    }
    if (k >= 64) {
      k = 0;
      blk = blk + 1 == c.bpm ? 0 : blk + 1;
    }
  }
  *exit = jpeg_seg_pack(jpeg_pbits_pos(&r, c.files), k, blk);
  *started = n;
  return 0;
}

// first half of a round: the lane's segments whose entry changed are decoded, symbols only
JPEG_HD void jpeg_par_decode(const jpeg_par_ctx& c, int lane, int lanes) {
  for (int s = lane; s < c.n_segs; s += lanes) {
    jpeg_seg row = c.segs[s];
    if (!(row.flags & JPEG_SEG_DIRTY)) continue;
    asm_jpeg_interval iv;
    int64_t end;
    bool last;
    int first_mcu, n_mcus, started = 0;
    // a row that is not this image's own (shared state rows) or names the last segment of an interval is not decoded
    int err = ASM_JPEG_EDESC;
    if (jpeg_par_segment_range(c, s, row, &iv, &end, &last, &first_mcu, &n_mcus) && !last)
      err = jpeg_par_decode_segment(c, iv.byte_begin, iv.byte_end, end, true, row.entry, nullptr, 0, 0, 0, &row.exit, &started);
    if (err) row.exit = JPEG_SEG_NOEXIT;
    row.count = started;
    row.flags &= ~JPEG_SEG_DIRTY;
    c.segs[s] = row;
  }
}

// second half: an exit that is no error and differs from the next segment's entry replaces it.  true: this lane published
JPEG_HD bool jpeg_par_publish(const jpeg_par_ctx& c, int lane, int lanes) {
  bool changed = false;
  for (int s = lane; s < c.n_segs; s += lanes) {
    const int flags = c.segs[s].flags;
    if (s == 0 || (flags & (JPEG_SEG_FIRST | JPEG_SEG_DEAD))) continue;
    const uint64_t from = c.segs[s - 1].exit;
    if (from == JPEG_SEG_NOEXIT || from == c.segs[s].entry) continue;
    c.segs[s].entry = from;
    // the last segment of an interval is decoded by the write phase alone
    if (!(flags & JPEG_SEG_LAST)) c.segs[s].flags = flags | JPEG_SEG_DIRTY;
    changed = true;
  }
  return changed;
}

// Validity and first-block ordinals: a segmented scan over the image's segments, restarted at the first segment of
// every interval.  Lane `lane` owns the contiguous run [lane * per, (lane + 1) * per); jpeg_par_chain_sum leaves the
// run's (sum, valid, saw a restart) in sum[lane] / flags[lane] (bit 0 valid, bit 1 restart), jpeg_par_chain_apply
// (after a barrier) folds the lanes in front of it into a carry and writes the ordinals.
JPEG_HD void jpeg_par_chain_walk(const jpeg_par_ctx& c, int lane, int lanes, int* sum, int* valid, bool* restart, bool store) {
  const int per = (c.n_segs + lanes - 1) / lanes;
  const int64_t from = (int64_t)lane * per;
  const int to = (int)(from + per < c.n_segs ? from + per : c.n_segs);
  for (int s = (int)from; s < to; ++s) {
    const jpeg_seg row = c.segs[s];
    if (row.flags & JPEG_SEG_FIRST) {
      *sum = 0;
      *valid = !(row.flags & JPEG_SEG_DEAD);
      *restart = true;
    }
    if (store) c.segs[s].ordinal = *valid ? *sum : -1;
    const bool follows = (row.flags & JPEG_SEG_LAST) || (s + 1 < c.n_segs && row.exit == c.segs[s + 1].entry);
    *valid = *valid && !(row.flags & JPEG_SEG_DIRTY) && row.exit != JPEG_SEG_NOEXIT && follows;
    const int64_t next = (int64_t)*sum + (row.count > 0 ? row.count : 0);       // a row's count is data, not a promise
    *sum = (int)(next < JPEG_SEG_COUNT_CAP ? next : JPEG_SEG_COUNT_CAP);
  }
}

JPEG_HD void jpeg_par_chain_sum(const jpeg_par_ctx& c, int lane, int lanes, int32_t* sum, uint8_t* flags) {
  int s = 0, valid = 1;
  bool restart = false;
  jpeg_par_chain_walk(c, lane, lanes, &s, &valid, &restart, false);
  sum[lane] = s;
  flags[lane] = (uint8_t)((valid ? 1 : 0) | (restart ? 2 : 0));
}

JPEG_HD void jpeg_par_chain_apply(const jpeg_par_ctx& c, int lane, int lanes, const int32_t* sum, const uint8_t* flags) {
  int64_t carry = 0;
  int valid = 1;
  for (int l = lane - 1; l >= 0; --l) {
    carry += sum[l];
    valid = valid && (flags[l] & 1);
    if (flags[l] & 2) break;
  }
  int s = (int)(carry < JPEG_SEG_COUNT_CAP ? carry : JPEG_SEG_COUNT_CAP);
  bool restart = false;
  jpeg_par_chain_walk(c, lane, lanes, &s, &valid, &restart, true);
}

// the write phase: the lane's valid segments once more, storing; returns the errors of the image's true decode
JPEG_HD int jpeg_par_write(const jpeg_par_ctx& c, int lane, int lanes) {
  int err = 0;
  for (int s = lane; s < c.n_segs; s += lanes) {
    const jpeg_seg row = c.segs[s];
    if (row.ordinal < 0 || (row.flags & JPEG_SEG_DEAD)) continue;
    asm_jpeg_interval iv;
    int64_t end;
    bool last;
    int first_mcu, n_mcus;
    if (!jpeg_par_segment_range(c, s, row, &iv, &end, &last, &first_mcu, &n_mcus)) continue;
    uint64_t exit;
    int started;
    err |= jpeg_par_decode_segment(c, iv.byte_begin, iv.byte_end, end, !last, row.entry, c.coefs, first_mcu, row.ordinal,
                                   (int64_t)n_mcus * c.bpm, &exit, &started);
  }
  return err;
}

// DC values from the stored differences: predictor = sum of the differences since the interval's first block, per
// component, in unsigned 32-bit arithmetic narrowed on store (addition mod 2^16 is associative, so this is the
// sequential (int16_t)(pred + diff) chain).  Lane `lane` owns the MCUs [lane * per, (lane + 1) * per) of the image; a
// predictor restarts at MCU 0 and at every multiple of restart_interval.
JPEG_HD void jpeg_par_dc_walk(const jpeg_par_ctx& c, int lane, int lanes, uint32_t* pred, bool* restart, bool store) {
  const jpeg_geom& g = c.g;
  const int per = (g.n_mcus + lanes - 1) / lanes;
  const int64_t from = (int64_t)lane * per;
  const int to = (int)(from + per < g.n_mcus ? from + per : g.n_mcus);
  const int ri = c.d.restart_interval;
  for (int m = (int)from; m < to; ++m) {
    if (m == 0 || (ri > 0 && m % ri == 0)) {
      pred[0] = pred[1] = pred[2] = 0;
      *restart = true;
    }
    const int my = m / g.mcus_x, mx = m - my * g.mcus_x;
    for (int comp = 0; comp < g.ncomp; ++comp) {
      for (int v = 0; v < g.cv[comp]; ++v) {
        for (int h = 0; h < g.ch[comp]; ++h) {
          const int64_t at = g.base[comp] + ((int64_t)(my * g.cv[comp] + v) * g.bw[comp] + (mx * g.ch[comp] + h)) * 64;
          if (at < 0 || at + 64 > g.n_coefs) continue;
          pred[comp] += (uint32_t)(int32_t)c.coefs[at];
          if (store) c.coefs[at] = (int16_t)(uint16_t)(pred[comp] & 0xFFFFu);
        }
      }
    }
  }
}

// sums: [3][lanes], flags: [lanes] (1: the run saw a restart)
JPEG_HD void jpeg_par_dc_sum(const jpeg_par_ctx& c, int lane, int lanes, uint32_t* sums, uint8_t* flags) {
  uint32_t pred[3] = {0, 0, 0};
  bool restart = false;
  jpeg_par_dc_walk(c, lane, lanes, pred, &restart, false);
  for (int comp = 0; comp < 3; ++comp) sums[comp * lanes + lane] = pred[comp];
  flags[lane] = restart ? 1 : 0;
}

JPEG_HD void jpeg_par_dc_apply(const jpeg_par_ctx& c, int lane, int lanes, const uint32_t* sums, const uint8_t* flags) {
  uint32_t pred[3] = {0, 0, 0};
  for (int l = lane - 1; l >= 0; --l) {
    for (int comp = 0; comp < 3; ++comp) pred[comp] += sums[comp * lanes + l];
    if (flags[l]) break;
  }
  bool restart = false;
  jpeg_par_dc_walk(c, lane, lanes, pred, &restart, true);
}
