// What the three host programs of the JPEG entropy stages (jpeg_entropy_host.cpp, jpeg_parallel_host.cpp,
// jpeg_progressive_host.cpp) do alike: reading a case file, clipping table rows to a cut file, sharing work items out
// over a few threads, and the enumeration of damage -- to the bytes (every truncation, every byte replaced by 00 / FF /
// D9, byte pairs by FF D9) and to the interval rows (a wrong RSTm, a count off by one, a row that ends past its range).
// Each program keeps its own Case, its own decode and its own summary line; the damage calls back into that decode.
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "../../assembled_cnn_amd/csrc/jpeg_entropy.h"

namespace probe {

inline bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// a count of type N (int32 for table rows, int64 for bytes and coefficients), then that many T
template <class N, class T>
bool read_rows(FILE* f, std::vector<T>* v, int64_t limit) {
  N n = 0;
  if (!read_exact(f, &n, sizeof n) || n < 0 || (int64_t)n > limit) return false;
  v->resize((size_t)n);
  return read_exact(f, v->data(), sizeof(T) * (size_t)n);
}

// the case file argv[1] and its count of cases, or null after saying why (usage, no such file, no count)
inline FILE* open_cases(int argc, char** argv, int32_t* count) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s cases.bin [threads]\n", argv[0]);
    return nullptr;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) perror(argv[1]);
  if (f && (!read_exact(f, count, 4) || *count < 0 || *count > 100000)) {
    fclose(f);
    f = nullptr;
  }
  return f;
}

// dc 0, dc 1, ac 0, ac 1 of a baseline image, built once, as the workgroup builds them in LDS
inline std::vector<jpeg_dtab> baseline_tabs(const asm_jpeg_tables& t) {
  std::vector<jpeg_dtab> tab(4);
  for (int i = 0; i < 4; ++i) {
    jpeg_dtab_prepare(i < 2 ? t.dc[i] : t.ac[i - 2], &tab[i]);
    jpeg_dtab_fill_look(&tab[i], 0, 1);
  }
  return tab;
}

// a file cut at `limit`: the byte ranges the host parser would find end there (interval rows and scan rows)
template <class Row>
void clip_row(Row* r, int64_t limit) {
  r->byte_begin = std::min<int64_t>(r->byte_begin, limit);
  r->byte_end = std::min<int64_t>(r->byte_end, limit);
}

// The descriptor, geometry and interval rows of a baseline case (its d, iv and scan) whose scan is cut at `limit`, as the
// workgroup would meet them: false and *st set where the kernel refuses the descriptor or the interval count.
template <class Case>
bool cut_rows(const Case& c, int64_t limit, asm_jpeg_desc* d, jpeg_geom* g, std::vector<asm_jpeg_interval>* iv, int* st) {
  *d = c.d;
  *st = 0;
  if (!jpeg_make_geom(*d, g)) *st = ASM_JPEG_EDESC;
  else if (d->n_intervals != jpeg_expected_intervals(d->restart_interval, g->n_mcus) || d->n_intervals != (int)c.iv.size())
    *st = ASM_JPEG_ERESTART;
  if (*st) return false;
  *iv = c.iv;      // an exact-size copy: a heap block of its own
  d->scan_offset = 0;
  d->scan_bytes = limit;
  d->first_interval = 0;
  if (limit < (int64_t)c.scan.size())
    for (auto& r : *iv) clip_row(&r, limit);
  return true;
}

// (1) of every program: the intact case k must end with status 0 and the reference's coefficients
inline void require_intact(size_t k, int st, bool equal, const char* how = "") {
  if (st != 0) fprintf(stderr, "case %zu%s: status %d on the intact input\n", k, how, st);
  else if (!equal) fprintf(stderr, "case %zu%s: coefficients differ from the reference\n", k, how);
  if (st != 0 || !equal) exit(1);
}

// work(i) for every i < n_items, shared out over argv[2] threads (default: up to 8)
template <class Work>
void run_pool(size_t n_items, int argc, char** argv, Work work) {
  std::atomic<size_t> next{0};
  auto worker = [&]() {
    for (size_t i = next++; i < n_items; i = next++) work(i);
  };
  const unsigned hw = std::thread::hardware_concurrency();
  const unsigned nthreads = argc > 2 ? (unsigned)atoi(argv[2]) : std::max(1u, std::min(8u, hw));
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < nthreads; ++t) pool.emplace_back(worker);
  worker();
  for (auto& t : pool) t.join();
}

// a work item: byte positions [from, to) of scan `scan` of case `k`
struct Item {
  size_t k;
  int scan;
  int64_t from, to;
};

inline void add_items(std::vector<Item>* items, size_t k, int scan, int64_t begin, int64_t end, int64_t chunk) {
  for (int64_t at = begin; at < end; at += chunk) items->push_back({k, scan, at, std::min(at + chunk, end)});
}

enum Damage { CUT, BYTE_00, BYTE_FF, BYTE_D9, PAIR_FF_D9, ROW_RST, ROW_COUNT, ROW_END, ROW_HUFF };
static const char* const kDamageName[] = {"cut", "00", "FF", "D9", "FF D9", "a wrong RSTm", "an interval count off by one",
                                          "an interval row one byte past its range", "a Huffman-pool index out of range"};

// which positions a sweep visits and whether it writes markers over byte pairs
struct Sweep {
  int64_t stride = 1;          // > 1: only every stride-th position ...
  int64_t also = -1;           // ... and this one
  int64_t pair_end = 0;        // FF D9 over (at, at + 1) while at + 1 < pair_end; 0: no pairs
};

// Every damage of the positions [from, to) of `whole`: decode(kind, at, bytes, n) sees either a heap block of exactly
// n = `at` bytes (CUT: one byte read past the cut is an AddressSanitizer report) or all n bytes with the replacement at `at`.
template <class Decode>
void sweep_damage(const std::vector<uint8_t>& whole, int64_t from, int64_t to, const Sweep& sw, Decode decode) {
  auto wanted = [&](int64_t at) { return sw.stride <= 1 || at % sw.stride == 0 || at == sw.also; };
  for (int64_t cut = from; cut < to; ++cut) {
    if (!wanted(cut)) continue;
    std::vector<uint8_t> head(whole.begin(), whole.begin() + cut);
    decode(CUT, cut, head.data(), cut);
  }
  const uint8_t repl[3] = {0x00, 0xFF, 0xD9};
  const int64_t n = (int64_t)whole.size();
  std::vector<uint8_t> bytes(whole);
  for (int64_t at = from; at < to; ++at) {
    if (!wanted(at)) continue;
    const uint8_t keep = bytes[(size_t)at];
    for (int r = 0; r < 3; ++r) {
      if (repl[r] == keep) continue;
      bytes[(size_t)at] = repl[r];
      decode((Damage)(BYTE_00 + r), at, bytes.data(), n);
    }
    bytes[(size_t)at] = keep;
    if (at + 1 < sw.pair_end) {      // a marker written over two bytes
      const uint8_t keep1 = bytes[(size_t)at + 1];
      bytes[(size_t)at] = 0xFF;
      bytes[(size_t)at + 1] = 0xD9;
      decode(PAIR_FF_D9, at, bytes.data(), n);
      bytes[(size_t)at] = keep;
      bytes[(size_t)at + 1] = keep1;
    }
  }
}

// Damaged rows of one scan: its rows [first, first + *n_intervals) of the interval table `iv`, which must lie in the bytes
// [.., range_end).  Each damage is made in place, run(kind, status it must end with) is called, and it is undone.
template <class Run>
void damage_rows(std::vector<asm_jpeg_interval>* iv, int32_t first, int32_t* n_intervals, int64_t range_end, Run run) {
  const int32_t n = *n_intervals;
  if (n > 1) {
    (*iv)[(size_t)first].rst ^= 1;
    run(ROW_RST, ASM_JPEG_ERESTART);
    (*iv)[(size_t)first].rst ^= 1;
  }
  *n_intervals = n > 1 ? n - 1 : 2;
  if (n == 1) iv->push_back(iv->back());      // keep first_interval + n_intervals inside the table
  run(ROW_COUNT, ASM_JPEG_ERESTART);
  if (n == 1) iv->pop_back();
  *n_intervals = n;
  asm_jpeg_interval& last = (*iv)[(size_t)first + (size_t)n - 1];
  const int64_t keep = last.byte_end;
  last.byte_end = range_end + 1;
  run(ROW_END, ASM_JPEG_EDESC);
  last.byte_end = keep;
}

// a damaged-row run of case k ended with `st`: `ok` says whether that is the status of the damage's kind
inline void require_row_status(size_t k, Damage kind, int st, int want, bool ok) {
  if (ok) return;
  fprintf(stderr, "case %zu: %s gave status %d, expected %d\n", k, kDamageName[kind], st, want);
  exit(1);
}

// One run's term of the status digest: a 64-bit hash of (case, scan, kind of damage, position, status word).  The
// programs add the terms mod 2^64, so the digest does not depend on the order the threads finish in.
inline uint64_t mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

inline uint64_t digest_term(size_t k, int scan, Damage kind, int64_t at, int status) {
  uint64_t h = 0;
  for (uint64_t v : {(uint64_t)k, (uint64_t)scan, (uint64_t)kind, (uint64_t)at, (uint64_t)(uint32_t)status}) h = mix64(h ^ v);
  return h;
}

}  // namespace probe
