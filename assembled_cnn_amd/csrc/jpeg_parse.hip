// asm_jpeg_parse / asm_jpeg_parse_fill: the tables of the JPEG decoders made on the device from whole files that already lie
// there (a batch of TFRecord payloads, or the files staged in one copy), in two launches around one small read-back -- the
// host only lays the class-0 files out between them (jpeg.py pack_device).  jpeg_parse.h has every rule and every routine,
// compiled for the host as well (tools/probes/jpeg_parse_host.cpp); this file only runs them on a 256-lane workgroup: lane
// 0 walks the marker segments through a window in LDS that all lanes load, then all lanes scan the entropy-coded bytes 16
// per lane per pass and lane 0 takes their markers in order.
#include "common.h"
#include "jpeg_parse.h"

namespace {

static_assert(sizeof(asm_span_desc) == 24 && sizeof(asm_jpeg_head) == 72 && sizeof(asm_jpeg_place) == 32 &&
                  sizeof(asm_jpeg_tables) == 1600 && sizeof(asm_jpeg_tables) % 4 == 0,
              "ABI");

// s->any of one pass: one ballot per wave
__device__ __forceinline__ void mark_wave(jpp_state* s, int lane, bool any) {
  const uint64_t m = __ballot(any);
  if ((lane & 63) == 0) s->any[lane >> 6] = m;
}

// the passes over the entropy-coded bytes [s->scan_begin, limit) until the scan's end is found or the bytes run out
__device__ void scan_passes(jpp_state* s, const uint8_t* span, int64_t limit, int segment_bytes, const jpp_rows* out,
                            int lane) {
  for (int64_t base = jpp_pass_base(span, s->scan_begin); base < limit - 1; base += JPP_WINDOW) {
    mark_wave(s, lane, jpp_scan_lane(s, span, limit, base, lane));
    __syncthreads();
    if (lane == 0) jpp_scan_combine(s, span, base, segment_bytes, out);
    __syncthreads();
    if (s->scan_done) break;          // the same for every lane; written again only behind the next barrier
  }
}

__global__ __launch_bounds__(JPP_LANES) void jpeg_parse_kernel(const uint8_t* __restrict__ buf, int64_t buf_bytes,
                                                               const asm_span_desc* __restrict__ spans, int segment_bytes,
                                                               asm_jpeg_head* __restrict__ heads,
                                                               asm_jpeg_tables* __restrict__ tables) {
  __shared__ jpp_state st;
  jpp_state* s = &st;
  const int i = blockIdx.x, lane = threadIdx.x;
  const asm_span_desc d = spans[i];
  if (lane == 0) {
    jpp_init(s);
    if (!jpp_span_ok(d.offset, d.length, buf_bytes)) s->cls = ASM_JPEG_PSPAN;
  }
  __syncthreads();
  if (s->cls == 0) {                  // the same for every lane
    const uint8_t* span = buf + d.offset;
    const int64_t n = d.length;
    for (;;) {
      int r;
      do {                            // the marker segments, window by window
        jpp_load_window(s, span, n, lane);
        __syncthreads();
        if (lane == 0) s->ret = jpp_walk(s, n);
        __syncthreads();
        r = s->ret;
      } while (r == JPP_REFILL);
      if (r == JPP_END) break;
      scan_passes(s, span, n, segment_bytes, nullptr, lane);
      if (lane == 0) {
        if (!s->scan_done) s->cls |= ASM_JPEG_PNOEOI;
        else if (s->n_iv > 2147483647) s->cls |= ASM_JPEG_PLIMIT;
        else jpp_after_scan(s);
      }
      __syncthreads();
      if (s->cls) break;
    }
  }
  __syncthreads();
  if (lane == 0) jpp_head(s, &heads[i]);
  jpp_tables(s, reinterpret_cast<uint32_t*>(&tables[i]), lane);
}

__global__ __launch_bounds__(JPP_LANES) void jpeg_parse_fill_kernel(
    const uint8_t* __restrict__ buf, int64_t buf_bytes, const asm_span_desc* __restrict__ spans, int n_spans,
    const asm_jpeg_head* __restrict__ heads, const asm_jpeg_tables* __restrict__ tables,
    const asm_jpeg_place* __restrict__ place, int n_intervals, int64_t total_segments, int segment_bytes,
    asm_jpeg_desc* __restrict__ descs, asm_jpeg_tables* __restrict__ tables_out, asm_jpeg_interval* __restrict__ intervals,
    int32_t* __restrict__ segment_first, int32_t* __restrict__ status) {
  __shared__ jpp_state st;
  __shared__ jpp_rows rows;
  jpp_state* s = &st;
  const int row = blockIdx.x, lane = threadIdx.x;
  const asm_jpeg_place p = place[row];
  // the same decisions in every lane: nothing below depends on the lane until the rows are written
  bool ok = p.span >= 0 && p.span < n_spans;
  asm_span_desc d = {};
  asm_jpeg_head h = {};
  if (ok) {
    d = spans[p.span];
    h = heads[p.span];
    ok = jpp_span_ok(d.offset, d.length, buf_bytes) && jpp_head_ok(h, d.length) && p.first_interval >= 0 &&
         p.first_interval <= n_intervals && h.n_intervals <= n_intervals - p.first_interval && p.first_segment >= 0 &&
         p.first_segment <= total_segments && h.n_segments <= total_segments - p.first_segment &&
         (segment_bytes != 0 || h.n_segments == 0);
  }
  uint32_t* tout = reinterpret_cast<uint32_t*>(&tables_out[row]);
  if (!ok) {
    for (int k = lane; k < (int)(sizeof(asm_jpeg_tables) / 4); k += JPP_LANES) tout[k] = 0;
    if (lane == 0) {
      memset(&descs[row], 0, sizeof(asm_jpeg_desc));
      status[row] = ASM_JPEG_EDESC;
    }
    return;
  }
  const uint32_t* tin = reinterpret_cast<const uint32_t*>(&tables[p.span]);
  for (int k = lane; k < (int)(sizeof(asm_jpeg_tables) / 4); k += JPP_LANES) tout[k] = tin[k];
  const int64_t limit = h.scan_begin + h.scan_bytes;
  if (lane == 0) {
    jpp_init(s);
    s->scan_begin = s->iv_begin = h.scan_begin;
    rows.intervals = intervals + p.first_interval;
    rows.segment_first = segment_bytes ? segment_first + p.first_interval : nullptr;
    rows.n_intervals = h.n_intervals;
    rows.n_segments = h.n_segments;
    rows.byte_shift = d.offset;
    rows.image = row;
    rows.restart_interval = h.restart_interval;
    rows.n_mcus = (int64_t)((h.width + 8 * h.hs - 1) / (8 * h.hs)) * ((h.height + 8 * h.vs - 1) / (8 * h.vs));
    rows.first_segment = p.first_segment;
  }
  __syncthreads();
  const uint8_t* span = buf + d.offset;
  scan_passes(s, span, limit, segment_bytes, &rows, lane);
  if (lane == 0) {
    // no marker but RSTm lies inside the bytes the head row names; the last interval ends with them
    bool good = !s->scan_done;
    if (good) jpp_close_interval(s, limit, -1, segment_bytes, &rows);
    good = good && !s->bad_rows && s->n_iv == h.n_intervals && s->n_seg == h.n_segments;
    if (good) jpp_desc(h, d.offset, p, &descs[row]);
    else memset(&descs[row], 0, sizeof(asm_jpeg_desc));
    status[row] = good ? 0 : ASM_JPEG_EDESC;
  }
}

bool segment_bytes_ok(int segment_bytes) {
  return segment_bytes == 0 || (segment_bytes >= 16 && segment_bytes <= 65536 && segment_bytes % 16 == 0);
}

}  // namespace

extern "C" int asm_jpeg_parse(const uint8_t* buf, int64_t buf_bytes, const asm_span_desc* spans, int n, int segment_bytes,
                              asm_jpeg_head* heads, asm_jpeg_tables* tables, void* stream) {
  ASM_REQUIRE(buf && spans && heads && tables, "jpeg_parse: null pointer");
  ASM_REQUIRE(n >= 0, "jpeg_parse: n = %d", n);
  ASM_REQUIRE(segment_bytes_ok(segment_bytes), "jpeg_parse: segment_bytes = %d is not 0 or a multiple of 16 in 16..65536",
              segment_bytes);
  ASM_REQUIRE(buf_bytes >= 0 && buf_bytes <= JPP_MAX_BYTES, "jpeg_parse: buf_bytes outside 0 .. 2^40 - 1");
  if (n == 0) return ASM_OK;
  ASM_LAUNCH(jpeg_parse_kernel, dim3(n), dim3(JPP_LANES), 0, (hipStream_t)stream, buf, buf_bytes, spans, segment_bytes, heads,
             tables);
  ASM_CHECK_LAUNCH("jpeg_parse");
  return ASM_OK;
}

extern "C" int asm_jpeg_parse_fill(const uint8_t* buf, int64_t buf_bytes, const asm_span_desc* spans, int n_spans,
                                   const asm_jpeg_head* heads, const asm_jpeg_tables* tables, const asm_jpeg_place* place,
                                   int n_rows, int n_intervals, int64_t total_segments, int segment_bytes,
                                   asm_jpeg_desc* descs, asm_jpeg_tables* tables_out, asm_jpeg_interval* intervals,
                                   int32_t* segment_first, int32_t* status, void* stream) {
  ASM_REQUIRE(buf && spans && heads && tables && place && descs && tables_out && intervals && status,
              "jpeg_parse_fill: null pointer");
  ASM_REQUIRE(segment_bytes_ok(segment_bytes),
              "jpeg_parse_fill: segment_bytes = %d is not 0 or a multiple of 16 in 16..65536", segment_bytes);
  ASM_REQUIRE(segment_first || segment_bytes == 0, "jpeg_parse_fill: null segment_first");
  ASM_REQUIRE(n_spans >= 0 && n_rows >= 0 && n_intervals >= 0 && total_segments >= 0 && total_segments < ((int64_t)1 << 30),
              "jpeg_parse_fill: n_spans = %d, n_rows = %d, n_intervals = %d, total_segments = %lld", n_spans, n_rows,
              n_intervals, (long long)total_segments);
  ASM_REQUIRE(buf_bytes >= 0 && buf_bytes <= JPP_MAX_BYTES, "jpeg_parse_fill: buf_bytes outside 0 .. 2^40 - 1");
  if (n_rows == 0) return ASM_OK;
  ASM_LAUNCH(jpeg_parse_fill_kernel, dim3(n_rows), dim3(JPP_LANES), 0, (hipStream_t)stream, buf, buf_bytes, spans, n_spans,
             heads, tables, place, n_intervals, total_segments, segment_bytes, descs, tables_out, intervals, segment_first,
             status);
  ASM_CHECK_LAUNCH("jpeg_parse_fill");
  return ASM_OK;
}
