// Host run of the device JPEG entropy decoder (assembled_cnn_amd/csrc/jpeg_entropy.h) under the address and
// undefined-behaviour sanitizers: the header's functions are the text the kernel compiles, so a clean run here is the
// bounds proof for the kernel's bitstream reads and coefficient writes.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread jpeg_entropy_host.cpp -o jpeg_entropy_host
//   jpeg_entropy_host cases.bin [threads]
//
// cases.bin (written by tests/test_jpeg_host_sanitizer.py): int32 count, then per case
//   asm_jpeg_desc, asm_jpeg_tables, int32 n_intervals, asm_jpeg_interval[n_intervals], int64 scan_bytes, the scan,
//   int64 n_coefs, int16 expected[n_coefs] (tests/jpeg_ref.py's coefficients)
// For every case: (1) the decode must succeed and equal `expected`; (2) every truncation of the scan and (3) the scan with
// each single byte replaced by 00, FF and D9 must end with a non-zero status or a completed decode; (4) damaged rows (a
// wrong RSTm, an interval count off by one, an interval row one byte past the scan) must end with the status bit of
// their kind.  The scan is copied into an exact-size heap block for every run, so one byte read past it is an
// AddressSanitizer report.  The damage itself and the thread pool are jpeg_probe.h's.  `status digest` is the sum of
// probe::digest_term over every damaged run: it pins each status word (tests/golden/jpeg_status_digests.json).
#include "jpeg_probe.h"

static_assert(sizeof(asm_jpeg_desc) == 96 && sizeof(asm_jpeg_tables) == 1600 && sizeof(asm_jpeg_interval) == 32, "ABI");

struct Case {
  asm_jpeg_desc d;
  asm_jpeg_tables t;
  std::vector<asm_jpeg_interval> iv;
  std::vector<uint8_t> scan;
  std::vector<int16_t> expected;
  std::vector<jpeg_dtab> tab;      // dc 0, dc 1, ac 0, ac 1: built once, as the workgroup builds them in LDS
};

// what one workgroup does for one image, on one "lane"; limit: the scan is cut to its first `limit` bytes
static int decode(const Case& c, const uint8_t* scan, int64_t limit, std::vector<int16_t>* out) {
  static const uint8_t zigzag[64] = JPEG_ZIGZAG_INIT;
  asm_jpeg_desc d;
  jpeg_geom g;
  std::vector<asm_jpeg_interval> iv;      // the tables, the interval rows and the coefficients are heap blocks of their own
  int st = 0;
  if (!probe::cut_rows(c, limit, &d, &g, &iv, &st)) return st;
  out->assign((size_t)g.n_coefs, 0);
  return jpeg_decode_lane(scan, d, g, iv.data(), iv.empty() ? 0 : iv[0].image, c.tab.data(), zigzag, 0, 1, out->data());
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
    std::vector<int16_t> out;
    std::vector<uint8_t> scan(c.scan);
    const int st = decode(c, scan.data(), (int64_t)scan.size(), &out);
    probe::require_intact(k, st, out == c.expected);
  }
  // (2), (3) damaged scans: work items of 128 byte positions of one case
  std::vector<probe::Item> items;
  for (size_t k = 0; k < cases.size(); ++k) probe::add_items(&items, k, 0, 0, (int64_t)cases[k].scan.size(), 128);
  std::atomic<long> runs{0}, failed_status{0}, completed{0};
  std::atomic<uint64_t> digest{0};
  probe::run_pool(items.size(), argc, argv, [&](size_t i) {
    const size_t k = items[i].k;
    std::vector<int16_t> out;
    probe::sweep_damage(cases[k].scan, items[i].from, items[i].to, probe::Sweep(),
                        [&](probe::Damage kind, int64_t at, const uint8_t* scan, int64_t n) {
                          const int st = decode(cases[k], scan, n, &out);
                          st ? ++failed_status : ++completed;
                          ++runs;
                          digest += probe::digest_term(k, 0, kind, at, st);
                        });
  });
  // (4) damaged rows
  long rows_damaged = 0;
  for (size_t k = 0; k < cases.size(); ++k) {
    Case w = cases[k];
    probe::damage_rows(&w.iv, 0, &w.d.n_intervals, (int64_t)w.scan.size(), [&](probe::Damage kind, int want) {
      std::vector<int16_t> out;
      std::vector<uint8_t> scan(w.scan);
      const int st = decode(w, scan.data(), (int64_t)scan.size(), &out);
      ++rows_damaged;
      digest += probe::digest_term(k, 0, kind, 0, st);
      probe::require_row_status(k, kind, st, want, (st & want) != 0);
    });
  }
  printf("jpeg_entropy_host: %zu cases intact and equal, %ld damaged runs (%ld ended with a status, %ld completed)\n",
         cases.size(), runs.load(), failed_status.load(), completed.load());
  printf("damaged rows: %ld\n", rows_damaged);
  printf("status digest: %016llx\n", (unsigned long long)digest.load());
  return 0;
}
