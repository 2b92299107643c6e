// Host run of the device JPEG header parser (assembled_cnn_amd/csrc/jpeg_parse.h) under the address and undefined-behaviour
// sanitizers.  The header's functions are the text jpeg_parse_kernel and jpeg_parse_fill_kernel compile; here the lanes of
// the workgroup are a loop and every barrier is the end of that loop, so each phase runs as the kernels run it.
//
//   c++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread jpeg_parse_host.cpp -o jpeg_parse_host
//   jpeg_parse_host cases.bin [threads]
//
// cases.bin (tests/test_jpeg_parse_host_sanitizer.py writes it; little endian): int32 count, then per case
//   int64 n, n file bytes; int32 accepted (what jpeg.parse says); int32 k, then k times the rows jpeg.pack makes for the file
//   alone: int32 segment_bytes, asm_jpeg_desc, asm_jpeg_tables, int32 rows + asm_jpeg_interval rows, int32 rows + int32
//   segment_first entries, int64 total_segments.
// Every case runs with its span starting at each offset 0..15 of a 16-byte vector, inside an exact-size heap block, between
// a neighbour in front and one behind that begin with FF D8, and guard bytes of FF: a byte read outside the span changes the
// result or is an AddressSanitizer report.  The class must be 0 exactly where `accepted` is set, and then the two launches'
// rows must equal the recorded ones field by field, byte positions compared relative to scan_offset.  The program prints
// the number of cases it ran; the test compares it with the number it wrote.  The thread pool is jpeg_probe.h's.
#include "jpeg_probe.h"

#include "../../assembled_cnn_amd/csrc/jpeg_parse.h"

#include <memory>

static_assert(sizeof(asm_jpeg_head) == 72 && sizeof(asm_jpeg_place) == 32 && sizeof(asm_span_desc) == 24, "ABI");

struct Rows {
  int32_t segment_bytes;
  asm_jpeg_desc d;
  asm_jpeg_tables t;
  std::vector<asm_jpeg_interval> iv;
  std::vector<int32_t> segment_first;
  int64_t total_segments;
};

struct Case {
  std::vector<uint8_t> file;
  int32_t accepted;
  std::vector<Rows> rows;
};

static const int kFront = 96, kBehind = 64;      // bytes of the block in front of alignment 0 and behind the span

// what scan_passes of jpeg_parse.hip does
static void scan_passes(jpp_state* s, const uint8_t* span, int64_t limit, int segment_bytes, const jpp_rows* out) {
  for (int64_t base = jpp_pass_base(span, s->scan_begin); base < limit - 1; base += JPP_WINDOW) {
    for (int lane = 0; lane < JPP_LANES; ++lane) jpp_mark(s, lane, jpp_scan_lane(s, span, limit, base, lane));
    jpp_scan_combine(s, span, base, segment_bytes, out);
    if (s->scan_done) break;
  }
}

// what jpeg_parse_kernel does for one span
static void parse_span(const uint8_t* buf, int64_t buf_bytes, const asm_span_desc& d, int segment_bytes, asm_jpeg_head* head,
                       asm_jpeg_tables* tables) {
  std::unique_ptr<jpp_state> state(new jpp_state);
  jpp_state* s = state.get();
  jpp_init(s);
  if (!jpp_span_ok(d.offset, d.length, buf_bytes)) s->cls = ASM_JPEG_PSPAN;
  if (s->cls == 0) {
    const uint8_t* span = buf + d.offset;
    const int64_t n = d.length;
    for (;;) {
      int r;
      do {
        for (int lane = 0; lane < JPP_LANES; ++lane) jpp_load_window(s, span, n, lane);
        r = s->ret = jpp_walk(s, n);
      } while (r == JPP_REFILL);
      if (r == JPP_END) break;
      scan_passes(s, span, n, segment_bytes, nullptr);
      if (!s->scan_done) s->cls |= ASM_JPEG_PNOEOI;
      else if (s->n_iv > 2147483647) s->cls |= ASM_JPEG_PLIMIT;
      else jpp_after_scan(s);
      if (s->cls) break;
    }
  }
  jpp_head(s, head);
  for (int lane = 0; lane < JPP_LANES; ++lane) jpp_tables(s, reinterpret_cast<uint32_t*>(tables), lane);
}

// what jpeg_parse_fill_kernel does for row 0 of a one-row batch; the tables are exact-size heap blocks
static int fill_row(const uint8_t* buf, int64_t buf_bytes, const asm_span_desc& d, const asm_jpeg_head& h,
                    const asm_jpeg_place& p, int segment_bytes, asm_jpeg_desc* desc, std::vector<asm_jpeg_interval>* iv,
                    std::vector<int32_t>* segment_first) {
  iv->assign((size_t)h.n_intervals, asm_jpeg_interval());
  segment_first->assign((size_t)h.n_intervals, -1);
  if (!jpp_span_ok(d.offset, d.length, buf_bytes) || !jpp_head_ok(h, d.length)) return ASM_JPEG_EDESC;
  std::unique_ptr<jpp_state> state(new jpp_state);
  jpp_state* s = state.get();
  jpp_rows rows;
  jpp_init(s);
  s->scan_begin = s->iv_begin = h.scan_begin;
  rows.intervals = iv->data() + p.first_interval;
  rows.segment_first = segment_bytes ? segment_first->data() + p.first_interval : nullptr;
  rows.n_intervals = h.n_intervals;
  rows.n_segments = h.n_segments;
  rows.byte_shift = d.offset;
  rows.image = 0;
  rows.restart_interval = h.restart_interval;
  rows.n_mcus = (int64_t)((h.width + 8 * h.hs - 1) / (8 * h.hs)) * ((h.height + 8 * h.vs - 1) / (8 * h.vs));
  rows.first_segment = p.first_segment;
  const int64_t limit = h.scan_begin + h.scan_bytes;
  scan_passes(s, buf + d.offset, limit, segment_bytes, &rows);
  bool good = !s->scan_done;
  if (good) jpp_close_interval(s, limit, -1, segment_bytes, &rows);
  good = good && !s->bad_rows && s->n_iv == h.n_intervals && s->n_seg == h.n_segments;
  if (good) jpp_desc(h, d.offset, p, desc);
  return good ? 0 : ASM_JPEG_EDESC;
}

static bool same_desc(const asm_jpeg_desc& a, const asm_jpeg_desc& e) {
  return a.scan_bytes == e.scan_bytes && a.coef_offset == e.coef_offset && a.plane_offset == e.plane_offset &&
         a.dst_offset == e.dst_offset && a.width == e.width && a.height == e.height && a.ncomp == e.ncomp && a.hs == e.hs &&
         a.vs == e.vs && a.mcus_x == e.mcus_x && a.mcus_y == e.mcus_y && a.restart_interval == e.restart_interval &&
         a.first_interval == e.first_interval && a.n_intervals == e.n_intervals && !memcmp(a.qsel, e.qsel, 4) &&
         !memcmp(a.dcsel, e.dcsel, 4) && !memcmp(a.acsel, e.acsel, 4) && a.reserved == e.reserved;
}

// one case at one start alignment: empty string, or what differs
static const char* run_case(const Case& c, int align) {
  const int64_t n = (int64_t)c.file.size(), at = kFront + align, total = at + n + kBehind;
  uint8_t* buf = (uint8_t*)aligned_alloc(16, (size_t)((total + 15) / 16 * 16));
  if (!buf) return "no memory";
  struct Free {
    uint8_t* p;
    ~Free() { free(p); }
  } guard{buf};
  memset(buf, 0xFF, (size_t)total);
  buf[kFront - 16 + 1] = 0xD8;                       // the neighbour in front, FF bytes up to the span
  if (n) memcpy(buf + at, c.file.data(), (size_t)n);
  buf[at + n + 1] = 0xD8;                            // the neighbour behind
  asm_span_desc d = {at, n, 0u, 0u};
  const int sizes[3] = {0, 16, 128};
  for (int sb : sizes) {
    asm_jpeg_head h;
    std::unique_ptr<asm_jpeg_tables> t(new asm_jpeg_tables);
    parse_span(buf, total, d, sb, &h, t.get());
    if ((h.cls == 0) != (c.accepted != 0)) return c.accepted ? "refused a file jpeg.parse accepts" : "accepted a file jpeg.parse refuses";
    if (h.cls != 0) {
      static const asm_jpeg_tables zero = {};
      if (memcmp(t.get(), &zero, sizeof zero)) return "a refused file with a table block that is not zero";
      continue;
    }
    for (const Rows& e : c.rows) {
      if (e.segment_bytes != sb && !(sb == 0 && &e == &c.rows[0])) continue;
      if (memcmp(t.get(), &e.t, sizeof e.t)) return "table block differs";
      if (h.n_intervals != (int32_t)e.iv.size() || (sb && h.n_segments != e.total_segments) || (!sb && h.n_segments != 0))
        return "interval or segment count differs";
      asm_jpeg_place p = {0, 0, 0, 0, e.d.coef_offset, e.d.dst_offset};
      asm_jpeg_desc desc = {};
      std::vector<asm_jpeg_interval> iv;
      std::vector<int32_t> first;
      if (fill_row(buf, total, d, h, p, sb, &desc, &iv, &first)) return "fill refused its own head row";
      if (!same_desc(desc, e.d) || desc.scan_offset != at + h.scan_begin) return "descriptor differs";
      for (size_t k = 0; k < iv.size(); ++k) {
        const asm_jpeg_interval &a = iv[k], &x = e.iv[k];
        if (a.image != x.image || a.first_mcu != x.first_mcu || a.n_mcus != x.n_mcus || a.rst != x.rst ||
            a.byte_begin - desc.scan_offset != x.byte_begin - e.d.scan_offset ||
            a.byte_end - desc.scan_offset != x.byte_end - e.d.scan_offset)
          return "interval row differs";
        if (sb && first[k] != e.segment_first[k]) return "segment_first differs";
      }
    }
  }
  return "";
}

int main(int argc, char** argv) {
  int32_t count = 0;
  FILE* f = probe::open_cases(argc, argv, &count);
  if (!f) return 2;
  std::vector<Case> cases((size_t)count);
  for (auto& c : cases) {
    int32_t k = 0;
    if (!probe::read_rows<int64_t>(f, &c.file, 1ll << 30) || !probe::read_exact(f, &c.accepted, 4) ||
        !probe::read_exact(f, &k, 4) || k < 0 || k > 4)
      return 2;
    c.rows.resize((size_t)k);
    for (auto& r : c.rows)
      if (!probe::read_exact(f, &r.segment_bytes, 4) || !probe::read_exact(f, &r.d, sizeof r.d) ||
          !probe::read_exact(f, &r.t, sizeof r.t) || !probe::read_rows<int32_t>(f, &r.iv, 1 << 24) ||
          !probe::read_rows<int32_t>(f, &r.segment_first, 1 << 24) || !probe::read_exact(f, &r.total_segments, 8) ||
          r.segment_first.size() != r.iv.size())
        return 2;
    if (c.accepted && c.rows.empty()) return 2;
  }
  fclose(f);
  std::atomic<long> ran{0}, accepted{0}, mismatches{0};
  probe::run_pool(cases.size(), argc, argv, [&](size_t k) {
    for (int align = 0; align < 16; ++align) {
      const char* why = run_case(cases[k], align);
      if (*why && mismatches++ < 20) fprintf(stderr, "case %zu at alignment %d: %s\n", k, align, why);
    }
    ++ran;
    if (cases[k].accepted) ++accepted;
  });
  printf("jpeg_parse_host: %ld cases at 16 alignments, %ld accepted, %ld mismatches\n", ran.load(), accepted.load(),
         mismatches.load());
  return mismatches.load() ? 1 : 0;
}
