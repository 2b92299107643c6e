// Host run of the device decoder's progressive entropy stage (assembled_cnn_amd/csrc/jpeg_entropy.h) under the address
// and undefined-behaviour sanitizers: the header's functions are the text jpeg_progressive_kernel compiles, so a clean run
// here is the bounds proof for the kernel's bitstream reads and coefficient reads and writes.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread jpeg_progressive_host.cpp -o jpeg_progressive_host
//   jpeg_progressive_host cases.bin [threads]
//
// cases.bin (written by tests/test_jpeg_progressive_host_sanitizer.py): int32 count, then per case
//   asm_jpeg_desc, int32 n_scans, asm_jpeg_scan[n_scans], int32 n_huff, asm_jpeg_huff[n_huff], int32 n_intervals,
//   asm_jpeg_interval[n_intervals], int64 n_bytes, the image's bytes (first scan to the end of the last),
//   int64 n_coefs, int16 expected[n_coefs] (tests/jpeg_progressive_ref.py's coefficients)
// For every case: (1) the decode must succeed and equal `expected`; (2) every truncation of every scan (the bytes are
// copied into a heap block that ends where the cut is, and the scan is decoded on top of what the scans before it left;
// if that ends without a status the scans after it follow, as they would on the device) and (3) every entropy-coded byte
// replaced by 00, FF and D9, and every pair of bytes by FF D9 (that scan and all scans after it are decoded, so the
// refinement scans run over whatever the damaged scan left) must end with a non-zero status or a completed decode.
// (4) Damaged rows, per case: a wrong RSTm, an interval count off by one, a Huffman-pool index out of range must each end
// with the status bit of their kind.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "../../assembled_cnn_amd/csrc/jpeg_entropy.h"

static_assert(sizeof(asm_jpeg_desc) == 96 && sizeof(asm_jpeg_scan) == 56 && sizeof(asm_jpeg_huff) == 272 &&
                  sizeof(asm_jpeg_interval) == 32,
              "ABI");

struct Case {
  asm_jpeg_desc d;
  std::vector<asm_jpeg_scan> scans;
  std::vector<asm_jpeg_huff> huff;
  std::vector<asm_jpeg_interval> iv;
  std::vector<uint8_t> bytes;
  std::vector<int16_t> expected;
  std::vector<std::vector<int16_t>> before;      // [k] the coefficients as the intact scans 0..k-1 leave them
};

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

template <class T>
static bool read_rows(FILE* f, std::vector<T>* v, int32_t limit) {
  int32_t n = 0;
  if (!read_exact(f, &n, 4) || n < 0 || n > limit) return false;
  v->resize((size_t)n);
  return read_exact(f, v->data(), sizeof(T) * (size_t)n);
}

// What the workgroup does for scans [from, to) of the image, on one "lane", on top of the coefficients in *coefs.
// bytes: the image's bytes, of which only the first `limit` exist (a file cut there: rows are clipped to it).
static int decode_scans(const Case& c, const uint8_t* bytes, int64_t limit, int from, int to, std::vector<int16_t>* coefs,
                        std::vector<std::vector<int16_t>>* snapshots = nullptr) {
  static const uint8_t zigzag[64] = JPEG_ZIGZAG_INIT;
  jpeg_geom g;
  asm_jpeg_desc d = c.d;
  d.scan_offset = 0;
  d.scan_bytes = limit;
  if (!jpeg_make_geom(d, &g) || (int64_t)coefs->size() != g.n_coefs) return ASM_JPEG_EDESC;
  std::vector<asm_jpeg_interval> iv(c.iv);      // exact-size copies: heap blocks of their own
  for (auto& r : iv) {
    r.byte_begin = std::min(r.byte_begin, limit);
    r.byte_end = std::min(r.byte_end, limit);
  }
  std::vector<jpeg_dtab> tab(3);
  int err = 0;
  for (int k = from; k < to && !err; ++k) {
    if (snapshots) snapshots->push_back(*coefs);
    asm_jpeg_scan sc = c.scans[(size_t)k];
    sc.byte_begin = std::min(sc.byte_begin, limit);
    sc.byte_end = std::min(sc.byte_end, limit);
    jpeg_scan_geom sg;
    err = jpeg_check_scan(d, g, sc, sc.image, (int)c.huff.size(), (int)iv.size(), &sg);
    if (err) break;
    const int n_tab = jpeg_scan_tables(sc);
    for (int t = 0; t < n_tab; ++t) {      // as the workgroup builds them in LDS
      jpeg_dtab_prepare(c.huff[(size_t)sc.huff[t]], &tab[(size_t)t]);
      jpeg_dtab_fill_look(&tab[(size_t)t], 0, 1);
    }
    err = jpeg_prog_decode_lane(bytes, g, sc, sg, iv.data(), sc.image, tab.data(), zigzag, 0, 1, coefs->data());
  }
  return err;
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
    int64_t nb = 0, nc = 0;
    if (!read_exact(f, &c.d, sizeof c.d) || !read_rows(f, &c.scans, 256) || !read_rows(f, &c.huff, 1024) ||
        !read_rows(f, &c.iv, 1 << 24) || !read_exact(f, &nb, 8) || nb < 0 || nb > (1ll << 30))
      return 2;
    c.bytes.resize((size_t)nb);
    if (!read_exact(f, c.bytes.data(), (size_t)nb) || !read_exact(f, &nc, 8) || nc < 0 || nc > (1ll << 30)) return 2;
    c.expected.resize((size_t)nc);
    if (!read_exact(f, c.expected.data(), 2 * (size_t)nc)) return 2;
  }
  fclose(f);

  // (1) intact
  for (size_t k = 0; k < cases.size(); ++k) {
    Case& c = cases[k];
    std::vector<int16_t> out(c.expected.size(), 0);
    std::vector<uint8_t> bytes(c.bytes);
    const int st = decode_scans(c, bytes.data(), (int64_t)bytes.size(), 0, (int)c.scans.size(), &out, &c.before);
    if (st != 0) {
      fprintf(stderr, "case %zu: status %d on the intact file\n", k, st);
      return 1;
    }
    if (out != c.expected) {
      fprintf(stderr, "case %zu: coefficients differ from the reference\n", k);
      return 1;
    }
  }
  // (2), (3) damaged scans: work items of CHUNK byte positions of one scan, shared out over a few threads
  const int64_t CHUNK = 128;
  struct Item {
    size_t k;
    int scan;
    int64_t from, to;
  };
  std::vector<Item> items;
  for (size_t k = 0; k < cases.size(); ++k)
    for (size_t s = 0; s < cases[k].scans.size(); ++s) {
      const asm_jpeg_scan& sc = cases[k].scans[s];
      for (int64_t at = sc.byte_begin; at < sc.byte_end; at += CHUNK)
        items.push_back({k, (int)s, at, std::min<int64_t>(at + CHUNK, sc.byte_end)});
    }
  std::atomic<size_t> next{0};
  std::atomic<long> runs{0}, failed_status{0}, completed{0};
  auto worker = [&]() {
    std::vector<int16_t> out;
    for (size_t i = next++; i < items.size(); i = next++) {
      const Case& c = cases[items[i].k];
      const int s = items[i].scan, n_scans = (int)c.scans.size();
      const int64_t n = (int64_t)c.bytes.size();
      for (int64_t cut = items[i].from; cut < items[i].to; ++cut) {      // a block of exactly `cut` bytes
        std::vector<uint8_t> bytes(c.bytes.begin(), c.bytes.begin() + cut);
        out = c.before[(size_t)s];
        int st = decode_scans(c, bytes.data(), cut, s, s + 1, &out);
        if (!st && s + 1 < n_scans) {      // the shortened scan decoded: the scans after it run on what it left
          std::vector<uint8_t> whole(c.bytes);
          st = decode_scans(c, whole.data(), n, s + 1, n_scans, &out);
        }
        st ? ++failed_status : ++completed;
        ++runs;
      }
      const uint8_t repl[3] = {0x00, 0xFF, 0xD9};
      std::vector<uint8_t> bytes(c.bytes);
      for (int64_t at = items[i].from; at < items[i].to; ++at) {
        const uint8_t keep = bytes[(size_t)at];
        for (uint8_t r : repl) {
          if (r == keep) continue;
          bytes[(size_t)at] = r;
          out = c.before[(size_t)s];
          decode_scans(c, bytes.data(), n, s, n_scans, &out) ? ++failed_status : ++completed;
          ++runs;
        }
        bytes[(size_t)at] = keep;
        if (at + 1 < c.scans[(size_t)s].byte_end) {      // a marker written over two bytes
          const uint8_t keep1 = bytes[(size_t)at + 1];
          bytes[(size_t)at] = 0xFF;
          bytes[(size_t)at + 1] = 0xD9;
          out = c.before[(size_t)s];
          decode_scans(c, bytes.data(), n, s, n_scans, &out) ? ++failed_status : ++completed;
          ++runs;
          bytes[(size_t)at] = keep;
          bytes[(size_t)at + 1] = keep1;
        }
      }
    }
  };
  const unsigned hw = std::thread::hardware_concurrency();
  const unsigned nthreads = argc > 2 ? (unsigned)atoi(argv[2]) : std::max(1u, std::min(8u, hw));
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < nthreads; ++t) pool.emplace_back(worker);
  worker();
  for (auto& t : pool) t.join();
  // (4) damaged rows
  long rows_damaged = 0;
  for (size_t k = 0; k < cases.size(); ++k) {
    const Case& c = cases[k];
    const int n_scans = (int)c.scans.size();
    auto run = [&](const Case& damaged, int want, const char* what) {
      std::vector<int16_t> out(c.expected.size(), 0);
      std::vector<uint8_t> bytes(c.bytes);
      const int st = decode_scans(damaged, bytes.data(), (int64_t)bytes.size(), 0, n_scans, &out);
      ++rows_damaged;
      if (st != want) {
        fprintf(stderr, "case %zu: %s gave status %d, expected %d\n", k, what, st, want);
        exit(1);
      }
    };
    for (int s = 0; s < n_scans; ++s) {
      const asm_jpeg_scan& sc = c.scans[(size_t)s];
      if (sc.n_intervals > 1) {
        Case w = c;
        w.iv[(size_t)sc.first_interval].rst ^= 1;
        run(w, ASM_JPEG_ERESTART, "a wrong RSTm");
      }
      {
        Case w = c;
        w.scans[(size_t)s].n_intervals += sc.n_intervals > 1 ? -1 : 1;
        if (sc.n_intervals == 1) w.iv.push_back(w.iv.back());      // keep first_interval + n_intervals inside the table
        run(w, ASM_JPEG_ERESTART, "an interval count off by one");
      }
      if (jpeg_scan_tables(sc) > 0) {
        Case w = c;
        w.scans[(size_t)s].huff[0] = (int32_t)c.huff.size();
        run(w, ASM_JPEG_EDESC, "a Huffman-pool index out of range");
      }
    }
  }
  printf("jpeg_progressive_host: %zu cases intact and equal, %ld damaged runs (%ld ended with a status, %ld completed), %ld damaged rows\n",
         cases.size(), runs.load(), failed_status.load(), completed.load(), rows_damaged);
  return 0;
}
