// CRC-32C (Castagnoli) of a byte span cut into chunks that run side by side: the range check, the chunk bounds, the chunk
// routine and the "feed 2^k zero bytes" operators of asm_crc32c_spans (records.hip).  Host and device compile this text:
// the kernel's lanes call it, and tools/probes/crc32c_spans_host.cpp runs the same lanes in a loop under the sanitizers.
//
// The register update c <- T[(c ^ b) & 0xff] ^ (c >> 8) is linear over GF(2) in (c, b): the register after a chunk followed
// by k more bytes is  Z_k . (register after the chunk)  ^  (register of those k bytes run from zero), with Z_k the 32 x 32
// matrix of k zero bytes.  So the span is cut into chunks, chunk 0 starts from the init state 0xffffffff and the others
// from zero, every chunk's register is advanced by the bytes BEHIND it (Z_k from the squarings Z_1, Z_2, Z_4, ...: the
// algebra of tf_bundle._shift_matrix), and the crc is the XOR of all of them, final-xored.  No serial combine.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/asm_hip.h"

#if defined(__HIPCC__)
#define CRC_HD __host__ __device__ inline
#else
#define CRC_HD inline
#endif

#define CRC_SHIFT_OPS 40                  // Z_(2^j), j = 0 .. 39: spans shorter than 2^40 bytes
#define CRC_MAX_BYTES (((int64_t)1 << CRC_SHIFT_OPS) - 1)

struct crc_tables {
  uint32_t byte[256];                     // the reflected Castagnoli byte table
  uint32_t shift[CRC_SHIFT_OPS][32];      // shift[j][i] = image of register bit i under 2^j zero bytes
};

// m . v for a 32 x 32 bit matrix kept as the images of the 32 unit vectors
CRC_HD constexpr uint32_t crc_mat_vec(const uint32_t* m, uint32_t v) {
  uint32_t out = 0;
  for (int i = 0; i < 32; ++i) out ^= ((v >> i) & 1u) ? m[i] : 0u;
  return out;
}

inline constexpr crc_tables crc_make_tables() {
  crc_tables t = {};
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0x82f63b78u : c >> 1;
    t.byte[i] = c;
  }
  for (int i = 0; i < 32; ++i) t.shift[0][i] = t.byte[(1u << i) & 0xffu] ^ ((1u << i) >> 8);
  for (int j = 1; j < CRC_SHIFT_OPS; ++j)
    for (int i = 0; i < 32; ++i) t.shift[j][i] = crc_mat_vec(t.shift[j - 1], t.shift[j - 1][i]);
  return t;
}

// the register after `nbytes` more zero bytes (0 <= nbytes < 2^40; higher bits are ignored)
CRC_HD uint32_t crc_advance(const uint32_t (*shift)[32], uint32_t reg, int64_t nbytes) {
  for (int j = 0; j < CRC_SHIFT_OPS; ++j)
    if ((nbytes >> j) & 1) reg = crc_mat_vec(shift[j], reg);
  return reg;
}

// descriptor check without int64 overflow: [offset, offset + length) lies inside [0, buf_bytes)
CRC_HD bool crc_span_ok(int64_t offset, int64_t length, int64_t buf_bytes) {
  return offset >= 0 && length >= 0 && offset <= buf_bytes && length <= buf_bytes - offset;
}

// Chunk `lane` of `lanes` of a span of `length` bytes whose first byte sits at address `addr`: [*begin, *end) relative to the
// span.  Chunks are whole 16-byte vectors of the ADDRESS space (so only the first has a ragged head and only the last a
// ragged tail), in order, and cover the span exactly; chunks past the end are empty (*begin == *end == length).
CRC_HD void crc_chunk_bounds(uint64_t addr, int64_t length, int lane, int lanes, int64_t* begin, int64_t* end) {
  const int64_t head = (int64_t)(addr & 15u);                     // bytes between the vector boundary below and the span
  const int64_t vectors = (head + length + 15) >> 4;              // < 2^37
  const int64_t step = ((vectors + lanes - 1) / lanes) << 4;      // bytes of address space per chunk
  int64_t b = step * lane - head, e = step * (lane + 1) - head;
  b = b < 0 ? 0 : b;
  *begin = b < length ? b : length;
  *end = e < length ? e : length;
}

CRC_HD uint32_t crc_step(const uint32_t* table, uint32_t c, uint32_t b) { return table[(c ^ b) & 0xffu] ^ (c >> 8); }

// the register after the n bytes at p, from `reg`: single bytes up to the first 16-byte boundary, whole aligned vectors,
// single bytes again.  Reads p[0 .. n) and nothing else.
CRC_HD uint32_t crc_chunk(const uint8_t* p, int64_t n, const uint32_t* table, uint32_t reg) {
  int64_t i = 0;
  const int64_t head = (int64_t)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u);
  for (; i < n && i < head; ++i) reg = crc_step(table, reg, p[i]);
  for (; i + 16 <= n; i += 16) {
    uint32_t w[4];
    memcpy(w, __builtin_assume_aligned(p + i, 16), 16);
    for (int k = 0; k < 4; ++k) {
      uint32_t v = w[k];
      for (int s = 0; s < 4; ++s, v >>= 8) reg = crc_step(table, reg, v & 0xffu);
    }
  }
  for (; i < n; ++i) reg = crc_step(table, reg, p[i]);
  return reg;
}

CRC_HD uint32_t crc_mask(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

// What lane `lane` of `lanes` contributes to the span's register: its chunk's register advanced by the bytes behind the
// chunk.  The XOR over all lanes, final-xored with 0xffffffff, is the crc.  The caller has checked the span (crc_span_ok).
CRC_HD uint32_t crc_lane(const uint8_t* buf, int64_t offset, int64_t length, int lane, int lanes, const uint32_t* table,
                         const uint32_t (*shift)[32]) {
  int64_t b, e;
  crc_chunk_bounds((uint64_t)(uintptr_t)(buf + offset), length, lane, lanes, &b, &e);
  if (lane != 0 && b == e) return 0;                               // an empty chunk from zero stays zero
  const uint32_t reg = crc_chunk(buf + offset + b, e - b, table, lane == 0 ? 0xffffffffu : 0u);
  return crc_advance(shift, reg, length - e);
}

// status word of one span from its crc (ASM_SPAN_EMISMATCH under flags & 1)
CRC_HD int32_t crc_span_status(uint32_t crc, uint32_t expect_masked, uint32_t flags) {
  return ((flags & 1u) && crc_mask(crc) != expect_masked) ? ASM_SPAN_EMISMATCH : 0;
}
