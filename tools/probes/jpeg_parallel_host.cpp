// Host run of the segment-parallel JPEG entropy decoder (assembled_cnn_amd/csrc/jpeg_parallel.h) under the address and
// undefined-behaviour sanitizers.  The header's functions are the text jpeg_entropy_parallel_kernel compiles; here the
// lanes of the workgroup are a loop and every barrier is the end of that loop, so each phase runs as the kernel runs it.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread jpeg_parallel_host.cpp -o jpeg_parallel_host
//   jpeg_parallel_host cases.bin [threads]
//
// cases.bin has the layout of jpeg_entropy_host.cpp's (tests/test_jpeg_parallel_host_sanitizer.py writes it).  Every run
// is made at segment_bytes 16, 48 and 128 and at 5 and 256 simulated lanes, and compared with the sequential decoder
// (jpeg_decode_lane) on the same bytes:
//   (1) intact: status 0, coefficients equal to the reference's and to the sequential decoder's;
//   (2) every truncation of the scan, (3) every byte replaced by 00, FF and D9: the same status word.
// A scan longer than kFullSweepBytes is damaged at every kStride-th position and at its middle (the cut the GPU tests
// use) instead of at every position; it runs intact in full.
//   (4) damaged rows (a wrong RSTm, an interval count off by one, an interval row one byte past the scan): the same
//       status word, which has the bit of the damage's kind;
//   (5) shared state rows: two images whose segment tables name the same rows of the state region, their phases
//       interleaved, in both orders: any result, but no access out of range and no more than segments + 1 rounds.
// The scan, the tables and the state region are exact-size heap blocks of their own, so one byte read or one row written
// past them is an AddressSanitizer report.  One line per case and configuration reports segments and rounds.  The damage
// and the thread pool are jpeg_probe.h's.
#include "jpeg_probe.h"

static_assert(sizeof(asm_jpeg_desc) == 96 && sizeof(asm_jpeg_tables) == 1600 && sizeof(asm_jpeg_interval) == 32 &&
                  sizeof(jpeg_seg) == 32,
              "ABI");

struct Case {
  asm_jpeg_desc d;
  asm_jpeg_tables t;
  std::vector<asm_jpeg_interval> iv;
  std::vector<uint8_t> scan;
  std::vector<int16_t> expected;
  std::vector<jpeg_dtab> tab;      // dc 0, dc 1, ac 0, ac 1
};

static const uint8_t kZigzag[64] = JPEG_ZIGZAG_INIT;
static const int kSegmentBytes[3] = {16, 48, 128};
static const int kLanes[2] = {5, 256};
static const int64_t kFullSweepBytes = 8192, kStride = 7;

// the sequential decoder: one workgroup, one lane
static int decode_sequential(const Case& c, const uint8_t* scan, int64_t limit, std::vector<int16_t>* out) {
  asm_jpeg_desc d;
  jpeg_geom g;
  std::vector<asm_jpeg_interval> iv;
  int st = 0;
  if (!probe::cut_rows(c, limit, &d, &g, &iv, &st)) return st;
  out->assign((size_t)g.n_coefs, 0);
  return jpeg_decode_lane(scan, d, g, iv.data(), iv.empty() ? 0 : iv[0].image, c.tab.data(), kZigzag, 0, 1, out->data());
}

// what jpeg_entropy_parallel_kernel does for one image, the lanes one after another
static int decode_parallel(const Case& c, const uint8_t* scan, int64_t limit, int segment_bytes, int lanes,
                           std::vector<int16_t>* out, int* n_segs, int* n_rounds) {
  jpeg_par_ctx x;
  std::vector<asm_jpeg_interval> iv;
  int st = 0;
  *n_segs = *n_rounds = 0;
  if (!probe::cut_rows(c, limit, &x.d, &x.g, &iv, &st)) return st;
  out->assign((size_t)x.g.n_coefs, 0);
  // the segment table, by the rule of include/asm_hip.h
  std::vector<int32_t> first(iv.size());
  int64_t total = 0;
  for (size_t k = 0; k < iv.size(); ++k) {
    first[k] = (int32_t)total;
    total += jpeg_par_interval_segments(iv[k], segment_bytes);
  }
  std::vector<jpeg_seg> segs((size_t)total);
  jpeg_par_ctx_fill(&x, scan, iv.data(), first.data(), iv.empty() ? 0 : iv[0].image, segment_bytes, c.tab.data(), kZigzag,
                    out->data());
  bool bad = false;
  for (int l = 0; l < lanes; ++l) bad |= jpeg_par_check_table(x, total, l, lanes);
  if (bad) return ASM_JPEG_EDESC;
  x.segs = segs.data();
  x.n_segs = jpeg_par_segments(x);
  if (x.n_segs != (int)total) return ASM_JPEG_EDESC;
  int err = 0;
  for (int l = 0; l < lanes; ++l) err |= jpeg_par_init(x, l, lanes);
  int rounds = 0;
  for (bool more = true; more && rounds <= x.n_segs; ++rounds) {
    for (int l = 0; l < lanes; ++l) jpeg_par_decode(x, l, lanes);
    more = false;
    for (int l = 0; l < lanes; ++l) more |= jpeg_par_publish(x, l, lanes);
  }
  std::vector<int32_t> chain((size_t)lanes);
  std::vector<uint32_t> dc(3 * (size_t)lanes);
  std::vector<uint8_t> flags((size_t)lanes);
  for (int l = 0; l < lanes; ++l) jpeg_par_chain_sum(x, l, lanes, chain.data(), flags.data());
  for (int l = 0; l < lanes; ++l) jpeg_par_chain_apply(x, l, lanes, chain.data(), flags.data());
  for (int l = 0; l < lanes; ++l) err |= jpeg_par_write(x, l, lanes);
  for (int l = 0; l < lanes; ++l) jpeg_par_dc_sum(x, l, lanes, dc.data(), flags.data());
  for (int l = 0; l < lanes; ++l) jpeg_par_dc_apply(x, l, lanes, dc.data(), flags.data());
  *n_segs = x.n_segs;
  *n_rounds = rounds;
  return err;
}

// (5): what two workgroups do when the segment table gives image 1 the state rows of image 0.  Each image has its own
// exact-size interval and segment tables (an index past the image's own rows is a report), the scans share one block.
static bool shared_rows(const Case& a, const Case& b, int segment_bytes, int lanes) {
  const Case* cs[2] = {&a, &b};
  const int64_t off[2] = {0, ((int64_t)a.scan.size() + 15) / 16 * 16};
  std::vector<uint8_t> files((size_t)off[1] + b.scan.size(), 0);
  std::copy(a.scan.begin(), a.scan.end(), files.begin());
  std::copy(b.scan.begin(), b.scan.end(), files.begin() + off[1]);
  jpeg_par_ctx x[2];
  std::vector<asm_jpeg_interval> iv[2];
  std::vector<int32_t> first[2];
  std::vector<int16_t> coefs[2];
  int64_t total[2];
  for (int i = 0; i < 2; ++i) {
    int st = 0;
    if (!probe::cut_rows(*cs[i], (int64_t)cs[i]->scan.size(), &x[i].d, &x[i].g, &iv[i], &st)) return false;
    x[i].d.scan_offset = off[i];
    total[i] = 0;
    for (auto& r : iv[i]) {
      r.image = i;
      r.byte_begin += off[i];
      r.byte_end += off[i];
      first[i].push_back((int32_t)total[i]);      // both images start at row 0
      total[i] += jpeg_par_interval_segments(r, segment_bytes);
    }
    coefs[i].assign((size_t)x[i].g.n_coefs, 0);
  }
  const int64_t rows = std::max(total[0], total[1]);
  std::vector<jpeg_seg> segs((size_t)rows);
  for (int i = 0; i < 2; ++i) {
    jpeg_par_ctx_fill(&x[i], files.data(), iv[i].data(), first[i].data(), i, segment_bytes, cs[i]->tab.data(), kZigzag,
                      coefs[i].data());
    x[i].segs = segs.data();
    for (int l = 0; l < lanes; ++l)
      if (jpeg_par_check_table(x[i], rows, l, lanes)) return false;
    x[i].n_segs = jpeg_par_segments(x[i]);
  }
  for (int i = 0; i < 2; ++i)
    for (int l = 0; l < lanes; ++l) jpeg_par_init(x[i], l, lanes);
  bool more[2] = {true, true};
  int rounds[2] = {0, 0};
  while ((more[0] && rounds[0] <= x[0].n_segs) || (more[1] && rounds[1] <= x[1].n_segs)) {
    for (int i = 0; i < 2; ++i) {
      if (!(more[i] && rounds[i] <= x[i].n_segs)) continue;
      for (int l = 0; l < lanes; ++l) jpeg_par_decode(x[i], l, lanes);
    }
    for (int i = 0; i < 2; ++i) {
      if (!(more[i] && rounds[i] <= x[i].n_segs)) continue;
      more[i] = false;
      for (int l = 0; l < lanes; ++l) more[i] |= jpeg_par_publish(x[i], l, lanes);
      ++rounds[i];
    }
  }
  std::vector<int32_t> chain((size_t)lanes);
  std::vector<uint32_t> dc(3 * (size_t)lanes);
  std::vector<uint8_t> flags((size_t)lanes);
  for (int i = 0; i < 2; ++i) {
    for (int l = 0; l < lanes; ++l) jpeg_par_chain_sum(x[i], l, lanes, chain.data(), flags.data());
    for (int l = 0; l < lanes; ++l) jpeg_par_chain_apply(x[i], l, lanes, chain.data(), flags.data());
  }
  for (int i = 1; i >= 0; --i) {      // the other image's ordinals are in the rows by now
    for (int l = 0; l < lanes; ++l) jpeg_par_write(x[i], l, lanes);
    for (int l = 0; l < lanes; ++l) jpeg_par_dc_sum(x[i], l, lanes, dc.data(), flags.data());
    for (int l = 0; l < lanes; ++l) jpeg_par_dc_apply(x[i], l, lanes, dc.data(), flags.data());
  }
  return rounds[0] <= x[0].n_segs + 1 && rounds[1] <= x[1].n_segs + 1;
}

int main(int argc, char** argv) {
  int32_t count = 0;
  FILE* f = probe::open_cases(argc, argv, &count);
  if (!f) return 2;
  std::vector<Case> cases((size_t)count);
  for (auto& c : cases) {
    if (!probe::read_exact(f, &c.d, sizeof c.d) || !probe::read_exact(f, &c.t, sizeof c.t) ||
        !probe::read_rows<int32_t>(f, &c.iv, 1 << 24) || !probe::read_rows<int64_t>(f, &c.scan, 1ll << 30) ||
        !probe::read_rows<int64_t>(f, &c.expected, 1ll << 30))
      return 2;
    c.tab = probe::baseline_tabs(c.t);
  }
  fclose(f);

  // (1) intact
  for (size_t k = 0; k < cases.size(); ++k) {
    const Case& c = cases[k];
    std::vector<int16_t> seq, par;
    std::vector<uint8_t> scan(c.scan);
    const int st = decode_sequential(c, scan.data(), (int64_t)scan.size(), &seq);
    probe::require_intact(k, st, seq == c.expected, " (sequential)");
    for (int sb : kSegmentBytes) {
      for (int lanes : kLanes) {
        int n_segs, rounds;
        const int pst = decode_parallel(c, scan.data(), (int64_t)scan.size(), sb, lanes, &par, &n_segs, &rounds);
        printf("case %zu segment_bytes %d lanes %d segments %d rounds %d\n", k, sb, lanes, n_segs, rounds);
        fflush(stdout);
        probe::require_intact(k, pst, par == c.expected, " (parallel, the configuration printed last)");
      }
    }
  }
  // (5) shared state rows: the single-interval case with the most bytes against the case with the most intervals
  {
    size_t one = 0, many = 0;
    for (size_t k = 0; k < cases.size(); ++k) {
      if (cases[k].iv.size() == 1 && (cases[one].iv.size() != 1 || cases[k].scan.size() > cases[one].scan.size())) one = k;
      if (cases[k].iv.size() > cases[many].iv.size()) many = k;
    }
    int done = 0;
    for (int sb : kSegmentBytes) {
      for (int lanes : kLanes) {
        if (!shared_rows(cases[one], cases[many], sb, lanes) || !shared_rows(cases[many], cases[one], sb, lanes)) {
          fprintf(stderr, "shared state rows (cases %zu and %zu, segment_bytes %d, %d lanes): refused or too many rounds\n", one,
                  many, sb, lanes);
          return 1;
        }
        done += 2;
      }
    }
    printf("shared state rows: cases %zu (%zu intervals) and %zu (%zu intervals), %d runs\n", one, cases[one].iv.size(), many,
           cases[many].iv.size(), done);
  }
  // (2), (3) damaged scans: work items of 64 byte positions of one case
  std::vector<probe::Item> items;
  for (size_t k = 0; k < cases.size(); ++k) probe::add_items(&items, k, 0, 0, (int64_t)cases[k].scan.size(), 64);
  // one damaged input at every segment size and lane count: the parallel decoder against the sequential one
  std::atomic<long> runs{0}, with_status{0}, mismatches{0};
  auto compare = [&](const Case& c, size_t k, const uint8_t* scan, int64_t n, probe::Damage kind, int64_t at) {
    std::vector<int16_t> seq, par;
    const int want = decode_sequential(c, scan, n, &seq);
    for (int sb : kSegmentBytes) {
      for (int lanes : kLanes) {
        int n_segs, rounds;
        const int got = decode_parallel(c, scan, n, sb, lanes, &par, &n_segs, &rounds);
        const bool same = got == want && (want != 0 || par == seq) && rounds >= (n_segs > 0 ? 1 : 0) && rounds <= n_segs + 1;
        if (!same && mismatches++ < 20)
          fprintf(stderr, "case %zu, %s at %lld (segment_bytes %d, %d lanes): status %d, sequential %d, %d rounds for %d segments\n",
                  k, probe::kDamageName[kind], (long long)at, sb, lanes, got, want, rounds, n_segs);
        ++runs;
      }
    }
    if (want) ++with_status;
    return want;
  };
  probe::run_pool(items.size(), argc, argv, [&](size_t i) {
    const size_t k = items[i].k;
    const Case& c = cases[k];
    const int64_t n = (int64_t)c.scan.size();
    probe::Sweep sw;
    if (n > kFullSweepBytes) {
      sw.stride = kStride;
      sw.also = n / 2;
    }
    probe::sweep_damage(c.scan, items[i].from, items[i].to, sw, [&](probe::Damage kind, int64_t at, const uint8_t* scan, int64_t m) {
      compare(c, k, scan, m, kind, at);
    });
  });
  // (4) damaged rows
  long rows_damaged = 0;
  for (size_t k = 0; k < cases.size(); ++k) {
    Case w = cases[k];
    probe::damage_rows(&w.iv, 0, &w.d.n_intervals, (int64_t)w.scan.size(), [&](probe::Damage kind, int want) {
      std::vector<uint8_t> scan(w.scan);
      const int st = compare(w, k, scan.data(), (int64_t)scan.size(), kind, 0);
      ++rows_damaged;
      probe::require_row_status(k, kind, st, want, (st & want) != 0);
    });
  }
  printf("jpeg_parallel_host: %zu cases intact and equal, %ld damaged runs (%ld damaged scans ended with a status), %ld mismatches\n",
         cases.size(), runs.load(), with_status.load(), mismatches.load());
  printf("damaged rows: %ld\n", rows_damaged);
  return mismatches.load() ? 1 : 0;
}
