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
// (4) Damaged rows, per scan: a wrong RSTm, an interval count off by one, an interval row one byte past its scan's range
// and a Huffman-pool index out of range must each end with the status of their kind.
// The damage itself and the thread pool are jpeg_probe.h's.  `status digest` is the sum of probe::digest_term over every
// damaged run: it pins each status word (tests/golden/jpeg_status_digests.json).
#include "jpeg_probe.h"

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

// What the workgroup does for scans [from, to) of the image, on one "lane", on top of the coefficients in *coefs.
// bytes: the image's bytes, of which only the first `limit` exist (a file cut there: rows are clipped to it).
static int decode_scans(const Case& c, const uint8_t* bytes, int64_t limit, int from, int to, std::vector<int16_t>* coefs,
                        std::vector<std::vector<int16_t>>* snapshots = nullptr) {
  static const uint8_t zigzag[64] = JPEG_ZIGZAG_INIT;
  const bool cut = limit < (int64_t)c.bytes.size();
  jpeg_geom g;
  asm_jpeg_desc d = c.d;
  d.scan_offset = 0;
  d.scan_bytes = limit;
  if (!jpeg_make_geom(d, &g) || (int64_t)coefs->size() != g.n_coefs) return ASM_JPEG_EDESC;
  std::vector<asm_jpeg_interval> iv(c.iv);      // exact-size copies: heap blocks of their own
  if (cut)
    for (auto& r : iv) probe::clip_row(&r, limit);
  std::vector<jpeg_dtab> tab(3);
  int err = 0;
  for (int k = from; k < to && !err; ++k) {
    if (snapshots) snapshots->push_back(*coefs);
    asm_jpeg_scan sc = c.scans[(size_t)k];
    if (cut) probe::clip_row(&sc, limit);
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
  int32_t count = 0;
  FILE* f = probe::open_cases(argc, argv, &count);
  if (!f) return 2;
  std::vector<Case> cases((size_t)count);
  for (auto& c : cases) {
    if (!probe::read_exact(f, &c.d, sizeof c.d) || !probe::read_rows<int32_t>(f, &c.scans, 256) ||
        !probe::read_rows<int32_t>(f, &c.huff, 1024) || !probe::read_rows<int32_t>(f, &c.iv, 1 << 24) ||
        !probe::read_rows<int64_t>(f, &c.bytes, 1ll << 30) || !probe::read_rows<int64_t>(f, &c.expected, 1ll << 30))
      return 2;
  }
  fclose(f);

  // (1) intact
  for (size_t k = 0; k < cases.size(); ++k) {
    Case& c = cases[k];
    std::vector<int16_t> out(c.expected.size(), 0);
    std::vector<uint8_t> bytes(c.bytes);
    const int st = decode_scans(c, bytes.data(), (int64_t)bytes.size(), 0, (int)c.scans.size(), &out, &c.before);
    probe::require_intact(k, st, out == c.expected);
  }
  // (2), (3) damaged scans: work items of 128 byte positions of one scan
  std::vector<probe::Item> items;
  for (size_t k = 0; k < cases.size(); ++k)
    for (size_t s = 0; s < cases[k].scans.size(); ++s)
      probe::add_items(&items, k, (int)s, cases[k].scans[s].byte_begin, cases[k].scans[s].byte_end, 128);
  std::atomic<long> runs{0}, failed_status{0}, completed{0};
  std::atomic<uint64_t> digest{0};
  probe::run_pool(items.size(), argc, argv, [&](size_t i) {
    const size_t k = items[i].k;
    const Case& c = cases[k];
    const int s = items[i].scan, n_scans = (int)c.scans.size();
    std::vector<int16_t> out;
    probe::Sweep sw;
    sw.pair_end = c.scans[(size_t)s].byte_end;
    probe::sweep_damage(c.bytes, items[i].from, items[i].to, sw,
                        [&](probe::Damage kind, int64_t at, const uint8_t* bytes, int64_t n) {
                          out = c.before[(size_t)s];
                          int st;
                          if (kind == probe::CUT) {
                            st = decode_scans(c, bytes, n, s, s + 1, &out);
                            if (!st && s + 1 < n_scans) {      // the shortened scan decoded: the scans after it run on what it left
                              std::vector<uint8_t> whole(c.bytes);
                              st = decode_scans(c, whole.data(), (int64_t)whole.size(), s + 1, n_scans, &out);
                            }
                          } else {
                            st = decode_scans(c, bytes, n, s, n_scans, &out);
                          }
                          st ? ++failed_status : ++completed;
                          ++runs;
                          digest += probe::digest_term(k, s, kind, at, st);
                        });
  });
  // (4) damaged rows
  long rows_damaged = 0;
  for (size_t k = 0; k < cases.size(); ++k) {
    const int n_scans = (int)cases[k].scans.size();
    for (int s = 0; s < n_scans; ++s) {
      Case w = cases[k];
      auto run = [&](probe::Damage kind, int want) {
        std::vector<int16_t> out(w.expected.size(), 0);
        std::vector<uint8_t> bytes(w.bytes);
        const int st = decode_scans(w, bytes.data(), (int64_t)bytes.size(), 0, n_scans, &out);
        ++rows_damaged;
        digest += probe::digest_term(k, s, kind, 0, st);
        probe::require_row_status(k, kind, st, want, st == want);
      };
      asm_jpeg_scan& sc = w.scans[(size_t)s];
      probe::damage_rows(&w.iv, sc.first_interval, &sc.n_intervals, sc.byte_end, run);
      if (jpeg_scan_tables(sc) > 0) {
        sc.huff[0] = (int32_t)w.huff.size();
        run(probe::ROW_HUFF, ASM_JPEG_EDESC);
      }
    }
  }
  printf("jpeg_progressive_host: %zu cases intact and equal, %ld damaged runs (%ld ended with a status, %ld completed), %ld damaged rows\n",
         cases.size(), runs.load(), failed_status.load(), completed.load(), rows_damaged);
  printf("status digest: %016llx\n", (unsigned long long)digest.load());
  return 0;
}
