// Host run of the span checksum's device text (assembled_cnn_amd/csrc/crc32c_spans.h) under the address and
// undefined-behaviour sanitizers: the header's functions are what every lane of crc32c_spans_kernel executes, so a clean run
// here is the bounds proof for the kernel's reads.
//
//   c++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=all crc32c_spans_host.cpp -o crc32c_spans_host
//   crc32c_spans_host
//
// (1) known answers: the RFC 3720 B.4 vectors and "123456789"; (2) spans of the lengths at which the chunking changes
// shape, at start alignments 0, 1, 7 and 15 modulo 16, cut into 256 lanes as the kernel does and into 1, 3 and 64: every
// span is copied to the END of a heap block of exactly head + length bytes, so one byte read past it is an
// AddressSanitizer report, and the `head` bytes in front of it differ from run to run, so a byte read before it changes the
// result; the chunks must tile the span and the XOR of the lanes must equal the byte-at-a-time crc; (3) descriptors that
// are out of range -- negative offset, negative length, end past the buffer, offset + length overflowing int64 -- must be
// refused by crc_span_ok (the kernel reads nothing for them) without signed overflow.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../assembled_cnn_amd/csrc/crc32c_spans.h"

static const crc_tables kTables = crc_make_tables();

static uint32_t reference(const uint8_t* p, int64_t n) {
  uint32_t c = 0xffffffffu;
  for (int64_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0x82f63b78u : c >> 1;
  }
  return c ^ 0xffffffffu;
}

// what one workgroup of `lanes` lanes computes for the span [offset, offset + length) of buf
static uint32_t workgroup(const uint8_t* buf, int64_t offset, int64_t length, int lanes, bool* tiled) {
  uint32_t r = 0;
  int64_t at = 0;
  for (int lane = 0; lane < lanes; ++lane) {
    int64_t b, e;
    crc_chunk_bounds((uint64_t)(uintptr_t)(buf + offset), length, lane, lanes, &b, &e);
    if (b != at || e < b || e > length) *tiled = false;
    if (lane > 0 && b < e && ((uintptr_t)(buf + offset + b) & 15u)) *tiled = false;    // only chunk 0 has a ragged head
    at = e;
    r ^= crc_lane(buf, offset, length, lane, lanes, kTables.byte, kTables.shift);
  }
  if (at != length) *tiled = false;
  return r ^ 0xffffffffu;
}

int main() {
  int failures = 0;
  // (1)
  struct { const char* name; uint32_t want; std::vector<uint8_t> data; } known[4] = {
      {"32 x 00", 0x8a9136aau, std::vector<uint8_t>(32, 0x00)},
      {"32 x ff", 0x62a8ab43u, std::vector<uint8_t>(32, 0xff)},
      {"00 .. 1f", 0x46dd794eu, {}},
      {"123456789", 0xe3069283u, {'1', '2', '3', '4', '5', '6', '7', '8', '9'}}};
  for (int i = 0; i < 32; ++i) known[2].data.push_back((uint8_t)i);
  for (auto& k : known) {
    bool tiled = true;
    std::vector<uint8_t> copy(k.data);
    const uint32_t got = workgroup(copy.data(), 0, (int64_t)copy.size(), 256, &tiled);
    if (got != k.want || !tiled || reference(copy.data(), (int64_t)copy.size()) != k.want) {
      printf("FAIL known answer %s: %08x, want %08x\n", k.name, got, k.want);
      ++failures;
    }
  }
  if (crc_mask(0xe3069283u) != 0xc78ab0e5u) {       // the trailer of the record of "123456789"
    printf("FAIL mask\n");
    ++failures;
  }
  // (2)
  const int64_t lengths[] = {0, 1, 3, 4, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537, 1048577};
  const int heads[] = {0, 1, 7, 15}, lane_counts[] = {256, 1, 3, 64};
  uint64_t seed = 0x9e3779b97f4a7c15ull;
  long spans = 0;
  for (int64_t length : lengths)
    for (int head : heads)
      for (int lanes : lane_counts) {
        void* block = nullptr;
        const size_t bytes = (size_t)(head + length);
        if (posix_memalign(&block, 16, bytes ? bytes : 1) != 0) return 2;
        uint8_t* p = static_cast<uint8_t*>(block);
        for (size_t i = 0; i < bytes; ++i) {
          seed = seed * 6364136223846793005ull + 1442695040888963407ull;
          p[i] = (uint8_t)(seed >> 56);
        }
        bool tiled = true;
        const uint32_t got = workgroup(p, head, length, lanes, &tiled), want = reference(p + head, length);
        if (got != want || !tiled) {
          printf("FAIL length %lld head %d lanes %d: %08x, want %08x, tiled %d\n", (long long)length, head, lanes, got, want,
                 (int)tiled);
          ++failures;
        }
        if (crc_span_status(got, crc_mask(want), 1) != 0 || crc_span_status(got, crc_mask(want) ^ 1u, 1) != ASM_SPAN_EMISMATCH ||
            crc_span_status(got, crc_mask(want) ^ 1u, 0) != 0) {
          printf("FAIL status word, length %lld\n", (long long)length);
          ++failures;
        }
        free(block);
        ++spans;
      }
  // (3)
  const int64_t big = INT64_MAX, size = 3000000;
  const int64_t bad[][2] = {{-1, 4},       {0, -1},      {size - 3, 4}, {size + 1, 0}, {big, 1},   {big - 2, big},
                            {1, big},      {big, big},   {INT64_MIN, 0}, {0, INT64_MIN}, {INT64_MIN, INT64_MIN}, {0, size + 1}};
  const int64_t good[][2] = {{0, 0}, {size, 0}, {0, size}, {size - 4, 4}, {17, 1}};
  long refused = 0;
  for (auto& d : bad) {
    if (crc_span_ok(d[0], d[1], size)) {
      printf("FAIL descriptor (%lld, %lld) accepted\n", (long long)d[0], (long long)d[1]);
      ++failures;
    }
    ++refused;
  }
  for (auto& d : good)
    if (!crc_span_ok(d[0], d[1], size)) {
      printf("FAIL descriptor (%lld, %lld) refused\n", (long long)d[0], (long long)d[1]);
      ++failures;
    }
  if (crc_span_ok(0, 1, 0) || !crc_span_ok(0, 0, 0)) ++failures;
  printf("%ld spans equal the byte-at-a-time crc, 4 known answers, %ld descriptors refused, %d failures\n", spans, refused,
         failures);
  return failures ? 1 : 0;
}
