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
// each single byte replaced by 00, FF and D9 must end with a non-zero status or a completed decode.  The scan is copied
// into an exact-size heap block for every run, so one byte read past it is an AddressSanitizer report.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "../../assembled_cnn_amd/csrc/jpeg_entropy.h"

static_assert(sizeof(asm_jpeg_desc) == 96 && sizeof(asm_jpeg_tables) == 1600 && sizeof(asm_jpeg_interval) == 32, "ABI");

struct Case {
  asm_jpeg_desc d;
  asm_jpeg_tables t;
  std::vector<asm_jpeg_interval> iv;
  std::vector<uint8_t> scan;
  std::vector<int16_t> expected;
  std::vector<jpeg_dtab> tab;      // dc 0, dc 1, ac 0, ac 1: built once, as the workgroup builds them in LDS
};

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// what one workgroup does for one image, on one "lane"; limit: the scan is cut to its first `limit` bytes
static int decode(const Case& c, const uint8_t* scan, int64_t limit, std::vector<int16_t>* out) {
  static const uint8_t zigzag[64] = JPEG_ZIGZAG_INIT;
  jpeg_geom g;
  asm_jpeg_desc d = c.d;
  if (!jpeg_make_geom(d, &g)) return ASM_JPEG_EDESC;
  if (d.n_intervals != jpeg_expected_intervals(d, g) || d.n_intervals != (int)c.iv.size()) return ASM_JPEG_ERESTART;
  // exact-size copies: the tables, the interval rows and the coefficient region are heap blocks of their own
  std::vector<asm_jpeg_interval> iv(c.iv);
  d.scan_offset = 0;
  d.scan_bytes = limit;
  d.first_interval = 0;
  for (auto& r : iv) {      // a file cut at `limit`: the ranges the host parser would find end there
    if (r.byte_begin > limit) r.byte_begin = limit;
    if (r.byte_end > limit) r.byte_end = limit;
  }
  out->assign((size_t)g.n_coefs, 0);
  return jpeg_decode_lane(scan, d, g, iv.data(), iv.empty() ? 0 : iv[0].image, c.tab.data(), zigzag, 0, 1, out->data());
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s cases.bin [threads]\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  int32_t count = 0;
  if (!read_exact(f, &count, 4) || count < 0 || count > 100000) return 2;
  std::vector<Case> cases((size_t)count);
  for (auto& c : cases) {
    int32_t ni = 0;
    int64_t nb = 0, nc = 0;
    if (!read_exact(f, &c.d, sizeof c.d) || !read_exact(f, &c.t, sizeof c.t) || !read_exact(f, &ni, 4) || ni < 0 ||
        ni > (1 << 24))
      return 2;
    c.iv.resize((size_t)ni);
    if (!read_exact(f, c.iv.data(), sizeof(asm_jpeg_interval) * (size_t)ni) || !read_exact(f, &nb, 8) || nb < 0 ||
        nb > (1ll << 30))
      return 2;
    c.scan.resize((size_t)nb);
    if (!read_exact(f, c.scan.data(), (size_t)nb) || !read_exact(f, &nc, 8) || nc < 0 || nc > (1ll << 30)) return 2;
    c.expected.resize((size_t)nc);
    if (!read_exact(f, c.expected.data(), 2 * (size_t)nc)) return 2;
    c.tab.resize(4);
    for (int i = 0; i < 4; ++i) {
      jpeg_dtab_prepare(i < 2 ? c.t.dc[i] : c.t.ac[i - 2], &c.tab[i]);
      jpeg_dtab_fill_look(&c.tab[i], 0, 1);
    }
  }
  fclose(f);

  // (1) intact
  for (size_t k = 0; k < cases.size(); ++k) {
    const Case& c = cases[k];
    std::vector<int16_t> out;
    std::vector<uint8_t> scan(c.scan);
    const int st = decode(c, scan.data(), (int64_t)scan.size(), &out);
    if (st != 0) {
      fprintf(stderr, "case %zu: status %d on the intact scan\n", k, st);
      return 1;
    }
    if (out != c.expected) {
      fprintf(stderr, "case %zu: coefficients differ from the reference\n", k);
      return 1;
    }
  }
  // (2), (3) damaged scans: work items of CHUNK byte positions of one case, shared out over a few threads
  const int64_t CHUNK = 128;
  struct Item {
    size_t k;
    int64_t from, to;
  };
  std::vector<Item> items;
  for (size_t k = 0; k < cases.size(); ++k)
    for (int64_t at = 0; at < (int64_t)cases[k].scan.size(); at += CHUNK)
      items.push_back({k, at, std::min<int64_t>(at + CHUNK, (int64_t)cases[k].scan.size())});
  std::atomic<size_t> next{0};
  std::atomic<long> runs{0}, failed_status{0}, completed{0};
  auto worker = [&]() {
    std::vector<int16_t> out;
    for (size_t i = next++; i < items.size(); i = next++) {
      const Case& c = cases[items[i].k];
      const int64_t n = (int64_t)c.scan.size();
      for (int64_t cut = items[i].from; cut < items[i].to; ++cut) {      // a block of exactly `cut` bytes
        std::vector<uint8_t> scan(c.scan.begin(), c.scan.begin() + cut);
        decode(c, scan.data(), cut, &out) ? ++failed_status : ++completed;
        ++runs;
      }
      const uint8_t repl[3] = {0x00, 0xFF, 0xD9};
      std::vector<uint8_t> scan(c.scan);
      for (int64_t at = items[i].from; at < items[i].to; ++at) {
        const uint8_t keep = scan[(size_t)at];
        for (uint8_t r : repl) {
          if (r == keep) continue;
          scan[(size_t)at] = r;
          decode(c, scan.data(), n, &out) ? ++failed_status : ++completed;
          ++runs;
        }
        scan[(size_t)at] = keep;
      }
    }
  };
  const unsigned hw = std::thread::hardware_concurrency();
  const unsigned nthreads = argc > 2 ? (unsigned)atoi(argv[2]) : std::max(1u, std::min(8u, hw));
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < nthreads; ++t) pool.emplace_back(worker);
  worker();
  for (auto& t : pool) t.join();
  printf("jpeg_entropy_host: %zu cases intact and equal, %ld damaged runs (%ld ended with a status, %ld completed)\n",
         cases.size(), runs.load(), failed_status.load(), completed.load());
  return 0;
}
