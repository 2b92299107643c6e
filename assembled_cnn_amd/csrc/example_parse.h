// tf.train.Example protos read on the device: what records._fields / _feature / _example / _proto do for ONE payload at
// buf[offset, offset + length), and the KD label row of records._kd_label, as plain functions shared by the kernels of
// records.hip and a host program (tools/probes/example_parse_host.cpp, built with the address and undefined-behaviour
// sanitizers): the same text is compiled for both.  A function that takes `lane` is run by every lane of the workgroup (a
// loop on the host); one that does not is lane 0's; between two of them the kernel has a barrier.
//
// Rules ("Examples on the device"):
//   varints     at most ten bytes, the tenth at most 1; truncation, an overlong varint and overflow are errors.
//   fields      wire types 0, 1, 2, 5; 3, 4, 6, 7 are errors; every length is checked against the enclosing message; unknown
//               fields are skipped by their wire type at every level.
//   structure   Example{1: Features}, Features{1: entry{1: key, 2: Feature}}, Feature{1: BytesList, 2: FloatList, 3:
//               Int64List}; every Feature of every name is validated in full (the host's _example does).
//   class       0 only where _proto does not raise, and then the row holds what it returns.  Everything else is a non-zero set
//               of ASM_EXAMPLE_P* bits (diagnostics: the host parses such a record again), so the walk stops at the first
//               thing that cannot be part of a class-0 record.  ASM_EXAMPLE_PFORM stands for the legal forms the walk leaves
//               to the host -- TensorFlow writes none of them.
// Safety: every read lies inside the span (never only inside the buffer) and every loop consumes a byte or ends.
//
// The walk is a stack of message ends (Example, Features, entry, Feature, list, packed varints) and reads through a window
// of ASM_EXAMPLE_WINDOW bytes that all lanes load with one 16-byte vector each.  A step -- one field header, with the key's
// bytes where the field is a short feature name -- needs at most EXP_NEED bytes; one that the window does not serve asks
// for a refill at its own position.  Blobs are skipped by their length and never loaded; a feature name longer than every
// name that is read is only scanned for bytes >= 0x80, window after window.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/asm_hip.h"
#include "jpeg_parse.h"        // jpp_load16, jpp_span_ok

#if defined(__HIPCC__)
#define EXP_HD __host__ __device__ inline
#else
#define EXP_HD inline
#endif

#define EXP_LANES (ASM_EXAMPLE_WINDOW / 16)
#define EXP_MAX_KEY 22                            // strlen("image/object/bbox/ymin"), the longest name that is read
#define EXP_NEED 48                               // two varints (20) and such a name
#define EXP_MAX_BYTES (((int64_t)1 << 40) - 1)
static_assert(ASM_EXAMPLE_WINDOW % 16 == 0 && EXP_NEED >= 20 + EXP_MAX_KEY && EXP_NEED + 15 <= ASM_EXAMPLE_WINDOW,
              "a refilled window serves every step");
static_assert(sizeof(asm_example_row) == 48, "ABI");

enum { EXP_REFILL = 0, EXP_END = 1 };                                     // what exp_walk returns
enum { EXP_L_EXAMPLE = 0, EXP_L_FEATURES, EXP_L_ENTRY, EXP_L_FEATURE, EXP_L_LIST, EXP_L_PACKED, EXP_LEVELS };
enum { EXP_ENCODED = 0, EXP_FILENAME, EXP_LABEL, EXP_LOGIT, EXP_YMIN, EXP_XMIN, EXP_YMAX, EXP_XMAX, EXP_NAMES };
enum { EXP_K_NONE = 0, EXP_K_BYTES = 1, EXP_K_FLOAT = 2, EXP_K_INT64 = 3 };   // the Feature's field numbers

struct exp_feat {
  int32_t kind, count;                     // values: BytesList entries, floats, integers
  int32_t parts, packed;                   // FloatList: fields that hold values, and those of them that are packed runs
  int64_t begin;                           // the first bytes entry / the first float part, relative to the span
  int32_t length;                          // of that bytes entry
  uint32_t value;                          // low 32 bits of the first integer
};

struct exp_state {
  alignas(16) uint8_t win[ASM_EXAMPLE_WINDOW];   // span bytes [win_base, win_base + WINDOW), valid in [win_from, win_to)
  int64_t win_base, win_from, win_to, want;
  int64_t at, end[EXP_LEVELS], scan_end;   // next byte, the open messages' ends, the end of the long key being scanned
  int32_t depth, scanning, ret, cls;
  int32_t n_key, n_val, n_kind, name;      // of the open map entry / Feature; name: EXP_NAMES for one that is not read
  uint32_t seen;                           // bit k: name k had an entry
  exp_feat cur, got[EXP_NAMES];
};

EXP_HD void exp_clear(exp_feat* f) {
  f->kind = f->count = f->parts = f->packed = f->length = 0;
  f->begin = 0;
  f->value = 0;
}

// lane 0: the state in front of the span's first byte; PSPAN / PFORM are decided here, before anything is read
EXP_HD void exp_init(exp_state* s, int64_t offset, int64_t length, int64_t buf_bytes) {
  s->win_base = s->win_from = s->win_to = s->want = 0;
  s->at = s->scan_end = 0;
  for (int l = 0; l < EXP_LEVELS; ++l) s->end[l] = 0;
  s->depth = s->scanning = s->ret = s->cls = 0;
  s->n_key = s->n_val = s->n_kind = 0;
  s->name = EXP_NAMES;
  s->seen = 0;
  exp_clear(&s->cur);
  for (int k = 0; k < EXP_NAMES; ++k) exp_clear(&s->got[k]);
  if (!jpp_span_ok(offset, length, buf_bytes)) s->cls = ASM_EXAMPLE_PSPAN;
  else if (length > 2147483647) s->cls = ASM_EXAMPLE_PFORM;
  else s->end[0] = length;
}

// every lane: the window at s->want (span bytes [0, n))
EXP_HD void exp_load_window(exp_state* s, const uint8_t* span, int64_t n, int lane) {
  const int64_t want = s->want;
  const int64_t base = want - (int64_t)((uintptr_t)(span + want) & 15u);
  jpp_load16(span, base + 16 * lane, 0, n, s->win + 16 * lane);
  if (lane == EXP_LANES - 1) {             // nobody reads these before the barrier
    s->win_base = base;
    s->win_from = base < 0 ? 0 : base;
    s->win_to = base + ASM_EXAMPLE_WINDOW < n ? base + ASM_EXAMPLE_WINDOW : n;
  }
}

EXP_HD uint32_t exp_b(const exp_state* s, int64_t pos) { return s->win[pos - s->win_base]; }
EXP_HD int exp_stop(exp_state* s, int why) {
  s->cls |= why;
  return EXP_END;
}

// records._varint at *pos, bounded by lim (<= the window's end): false for a truncated, overlong or overflowing one
EXP_HD bool exp_varint(const exp_state* s, int64_t* pos, int64_t lim, uint64_t* value) {
  uint64_t v = 0;
  int64_t p = *pos;
  for (int k = 0; k < 10; ++k) {
    if (p >= lim) return false;
    const uint32_t b = exp_b(s, p++);
    v |= (uint64_t)(b & 0x7fu) << (7 * k);
    if (!(b & 0x80u)) {
      if (k == 9 && b > 1) return false;
      *pos = p;
      *value = v;
      return true;
    }
  }
  return false;
}

// which of the names that are read the key [at, at + len) is (len <= EXP_MAX_KEY, inside the window); EXP_NAMES: none
EXP_HD int exp_name(const exp_state* s, int64_t at, int len) {
  constexpr char names[EXP_NAMES][EXP_MAX_KEY + 1] = {"image/encoded",          "image/filename",         "image/class/label",
                                                      "image/logit",            "image/object/bbox/ymin", "image/object/bbox/xmin",
                                                      "image/object/bbox/ymax", "image/object/bbox/xmax"};
  for (int k = 0; k < EXP_NAMES; ++k) {
    int j = 0;
    while (j < len && names[k][j] != 0 && exp_b(s, at + j) == (uint32_t)(uint8_t)names[k][j]) ++j;
    if (j == len && names[k][j] == 0) return k;
  }
  return EXP_NAMES;
}

EXP_HD void exp_push(exp_state* s, int level, int64_t begin, int64_t end) {
  s->depth = level;
  s->end[level] = end;
  s->at = begin;
}

// Lane 0: walk from s->at for as long as the window serves.  EXP_REFILL: load the window at s->want and call again;
// EXP_END: s->cls is 0 behind the last byte of a well-formed Example, or says why the walk stopped.
EXP_HD int exp_walk(exp_state* s, int64_t n) {
  for (;;) {
    const int64_t at = s->at;
    if (at < n) {
      const int64_t need_to = n - at < EXP_NEED ? n : at + EXP_NEED;
      if (at < s->win_from || need_to > s->win_to) {
        s->want = at;
        return EXP_REFILL;
      }
    }
    if (s->scanning) {                       // a long feature name: at < scan_end <= n, so the window holds byte `at`
      const int64_t lim = s->scan_end < s->win_to ? s->scan_end : s->win_to;
      int64_t p = at;
      while (p < lim && !(exp_b(s, p) & 0x80u)) ++p;
      if (p < lim) return exp_stop(s, ASM_EXAMPLE_PFORM);
      s->at = p;
      s->scanning = p < s->scan_end;         // more of it behind a refill
      continue;
    }
    const int depth = s->depth;
    const int64_t end = s->end[depth];
    if (at >= end) {                         // the open message is complete
      if (depth == EXP_L_EXAMPLE) return EXP_END;
      if (depth == EXP_L_ENTRY && s->name < EXP_NAMES) {
        if ((s->seen >> s->name) & 1u) return exp_stop(s, ASM_EXAMPLE_PFORM);      // the last of two would win
        s->seen |= 1u << s->name;
        s->got[s->name] = s->cur;
      }
      s->depth = depth - 1;
      continue;
    }
    int64_t p = at;
    uint64_t v = 0;
    if (depth == EXP_L_PACKED) {             // one integer of a packed run
      if (!exp_varint(s, &p, end, &v)) return exp_stop(s, ASM_EXAMPLE_PMALFORMED);
      if (s->cur.count++ == 0) s->cur.value = (uint32_t)v;
      s->at = p;
      continue;
    }
    // one field: records._fields
    uint64_t key = 0;
    if (!exp_varint(s, &p, end, &key)) return exp_stop(s, ASM_EXAMPLE_PMALFORMED);
    const uint64_t fn = key >> 3;
    const int wt = (int)(key & 7u);
    int64_t body = p, next;
    if (wt == 0) {
      if (!exp_varint(s, &p, end, &v)) return exp_stop(s, ASM_EXAMPLE_PMALFORMED);
      next = p;
    } else if (wt == 1 || wt == 5) {
      if ((wt == 1 ? 8 : 4) > end - p) return exp_stop(s, ASM_EXAMPLE_PMALFORMED);
      next = p + (wt == 1 ? 8 : 4);
    } else if (wt == 2) {
      uint64_t len = 0;
      if (!exp_varint(s, &p, end, &len) || len > (uint64_t)(end - p)) return exp_stop(s, ASM_EXAMPLE_PMALFORMED);
      body = p;
      next = p + (int64_t)len;
    } else {
      return exp_stop(s, ASM_EXAMPLE_PMALFORMED);
    }
    s->at = next;                            // skipped, unless a case below opens it
    const bool sub = wt == 2;                // a length-delimited field
    switch (depth) {
      case EXP_L_EXAMPLE:
        if (fn == 1 && sub) exp_push(s, EXP_L_FEATURES, body, next);
        break;
      case EXP_L_FEATURES:
        if (fn == 1 && sub) {
          exp_push(s, EXP_L_ENTRY, body, next);
          s->n_key = s->n_val = 0;
          s->name = EXP_NAMES;               // no key: the name ''
          exp_clear(&s->cur);                // no value: a Feature with no kind
        }
        break;
      case EXP_L_ENTRY:
        if (fn == 1 && sub) {
          if (++s->n_key > 1) return exp_stop(s, ASM_EXAMPLE_PFORM);
          if (next - body > EXP_MAX_KEY) {
            s->at = body;
            s->scan_end = next;
            s->scanning = 1;
          } else {                           // body + length <= at + EXP_NEED: in the window
            for (int64_t q = body; q < next; ++q)
              if (exp_b(s, q) & 0x80u) return exp_stop(s, ASM_EXAMPLE_PFORM);
            s->name = exp_name(s, body, (int)(next - body));
          }
        } else if (fn == 2 && sub) {
          if (++s->n_val > 1) return exp_stop(s, ASM_EXAMPLE_PFORM);
          exp_push(s, EXP_L_FEATURE, body, next);
          s->n_kind = 0;
        }
        break;
      case EXP_L_FEATURE:
        if (fn >= 1 && fn <= 3 && sub) {
          if (++s->n_kind > 1) return exp_stop(s, ASM_EXAMPLE_PFORM);
          exp_clear(&s->cur);
          s->cur.kind = (int32_t)fn;
          exp_push(s, EXP_L_LIST, body, next);
        }
        break;
      case EXP_L_LIST:
        if (fn != 1) break;
        if (s->cur.kind == EXP_K_BYTES) {
          if (sub && s->cur.count++ == 0) {
            s->cur.begin = body;
            s->cur.length = (int32_t)(next - body);
          }
        } else if (s->cur.kind == EXP_K_FLOAT) {
          if (sub) {
            if ((next - body) & 3) return exp_stop(s, ASM_EXAMPLE_PMALFORMED);
            if (s->cur.parts++ == 0) s->cur.begin = body;
            ++s->cur.packed;
            s->cur.count += (int32_t)((next - body) >> 2);
          } else if (wt == 5) {
            ++s->cur.parts;
            ++s->cur.count;
          }
        } else {
          if (wt == 0) {
            if (s->cur.count++ == 0) s->cur.value = (uint32_t)v;
          } else if (sub) {
            exp_push(s, EXP_L_PACKED, body, next);
          }
        }
        break;
      default:
        return exp_stop(s, ASM_EXAMPLE_PMALFORMED);
    }
  }
}

// records._fixed for a feature of one value: false where _proto refuses it
EXP_HD bool exp_fixed(const exp_feat& f, int kind) { return f.kind == EXP_K_NONE || (f.kind == kind && f.count == 1); }

// Lane 0: the row -- records._proto's checks on what the walk collected; `offset` is the span's position in buf
EXP_HD void exp_row(exp_state* s, int64_t offset, asm_example_row* out) {
  asm_example_row r;
  memset(&r, 0, sizeof r);
  if (s->cls == 0) {
    const exp_feat &enc = s->got[EXP_ENCODED], &name = s->got[EXP_FILENAME], &label = s->got[EXP_LABEL], &logit = s->got[EXP_LOGIT];
    if (!exp_fixed(enc, EXP_K_BYTES) || !exp_fixed(name, EXP_K_BYTES) || !exp_fixed(label, EXP_K_INT64)) s->cls |= ASM_EXAMPLE_PSCHEMA;
    if (logit.kind != EXP_K_NONE && logit.kind != EXP_K_FLOAT) s->cls |= ASM_EXAMPLE_PSCHEMA;
    else if (logit.parts > 1 || logit.parts != logit.packed) s->cls |= ASM_EXAMPLE_PFORM;
    for (int k = EXP_YMIN; k <= EXP_XMAX; ++k) {
      const exp_feat& b = s->got[k];
      if ((b.kind != EXP_K_NONE && b.kind != EXP_K_FLOAT) || b.count != s->got[EXP_YMIN].count) s->cls |= ASM_EXAMPLE_PSCHEMA;
    }
    if (s->cls == 0) {
      r.label = label.kind == EXP_K_NONE ? -1 : (int32_t)label.value;
      r.enc_offset = offset + enc.begin;              // begin and length are 0 for a feature that is absent or has no kind
      r.enc_length = enc.length;
      r.name_offset = offset + name.begin;
      r.name_length = name.length;
      r.logit_count = logit.count;
      r.logit_offset = offset + (logit.count ? logit.begin : 0);
      r.n_boxes = s->got[EXP_YMIN].count;
    }
  }
  r.cls = s->cls;
  *out = r;
}

// ---- the KD label row: records._kd_label from the payload bytes ------------------------------------------------------------
// the same for every lane: 0, or why the row is left as it is
EXP_HD int32_t exl_status(const asm_example_row& r, int num_classes, int64_t buf_bytes) {
  if (r.cls != 0 || r.logit_count != num_classes) return ASM_EXAMPLE_LSKIP;
  const int64_t bytes = 4 * (int64_t)num_classes;
  if (r.logit_offset < 0 || r.logit_offset > buf_bytes || bytes > buf_bytes - r.logit_offset) return ASM_EXAMPLE_LRANGE;
  return 0;
}

// column `col` of [0, 2 * num_classes) as its bit pattern: one_hot(label), then the logits byte by byte (they lie at any
// alignment; no float arithmetic touches them)
EXP_HD uint32_t exl_word(const uint8_t* buf, const asm_example_row& r, int num_classes, int col) {
  if (col < num_classes) return col == r.label ? 0x3f800000u : 0u;
  const uint8_t* p = buf + r.logit_offset + 4 * (int64_t)(col - num_classes);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
