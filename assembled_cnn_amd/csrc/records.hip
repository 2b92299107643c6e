// asm_crc32c_spans: the CRC-32C of many byte spans in one launch -- the payload checksums of a batch of TFRecord records
// (tf.data.TFRecordDataset verifies them in its reader, functions/input_fns.py:63-74), checked on the device where the
// encoded bytes are needed anyway.  One 256-lane workgroup per span: the span is cut into 256 chunks of whole 16-byte
// vectors, lane l runs chunk l through the byte table (in LDS), advances its register by the bytes behind its chunk with
// the "2^k zero bytes" operators (in LDS as well) and the workgroup XORs the 256 registers together: crc32c_spans.h has
// the algebra and every routine; this file only stages the tables and reduces.
//
// asm_example_parse / asm_example_label_rows: the tf.train.Example protos of those payloads read where they lie.  One
// workgroup of EXP_LANES lanes per record: lane 0 walks the proto through a window in LDS that all lanes load, and writes
// the record's row; then one 256-lane workgroup per row writes the KD label row from the logit bytes.  example_parse.h has
// every rule and every routine, compiled for the host as well (tools/probes/example_parse_host.cpp).
#include "common.h"
#include "crc32c_spans.h"
#include "example_parse.h"

namespace {

constexpr int kLanes = 256;
static_assert(sizeof(asm_span_desc) == 24, "ABI");

__device__ const crc_tables g_crc_tables = crc_make_tables();

__global__ __launch_bounds__(kLanes) void crc32c_spans_kernel(const uint8_t* __restrict__ buf, int64_t buf_bytes,
                                                              const asm_span_desc* __restrict__ spans,
                                                              uint32_t* __restrict__ crc, int32_t* __restrict__ status) {
  __shared__ crc_tables tab;
  __shared__ uint32_t part[kLanes / 64];
  const int i = blockIdx.x, lane = threadIdx.x;
  const asm_span_desc d = spans[i];
  if (!crc_span_ok(d.offset, d.length, buf_bytes)) {                    // same for every lane: nothing is read
    if (lane == 0) {
      crc[i] = 0;
      status[i] = ASM_SPAN_EDESC;
    }
    return;
  }
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&g_crc_tables);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&tab);
    for (int k = lane; k < (int)(sizeof(crc_tables) / 4); k += kLanes) dst[k] = src[k];
  }
  __syncthreads();
  uint32_t r = crc_lane(buf, d.offset, d.length, lane, kLanes, tab.byte, tab.shift);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r ^= (uint32_t)__shfl_xor((int)r, o, 64);
  if ((lane & 63) == 0) part[lane >> 6] = r;
  __syncthreads();
  if (lane == 0) {
    const uint32_t c = part[0] ^ part[1] ^ part[2] ^ part[3] ^ 0xffffffffu;
    crc[i] = c;
    status[i] = crc_span_status(c, d.expect_masked, d.flags);
  }
}

__global__ __launch_bounds__(EXP_LANES) void example_parse_kernel(const uint8_t* __restrict__ buf, int64_t buf_bytes,
                                                                  const asm_span_desc* __restrict__ spans,
                                                                  asm_example_row* __restrict__ rows) {
  __shared__ exp_state st;
  exp_state* s = &st;
  const int i = blockIdx.x, lane = threadIdx.x;
  const asm_span_desc d = spans[i];
  if (lane == 0) exp_init(s, d.offset, d.length, buf_bytes);
  __syncthreads();
  if (s->cls == 0) {                  // the same for every lane; lane 0 changes it only inside the loop, whose exit is s->ret
    const uint8_t* span = buf + d.offset;
    int r;
    do {                              // window by window
      exp_load_window(s, span, d.length, lane);
      __syncthreads();
      if (lane == 0) s->ret = exp_walk(s, d.length);
      __syncthreads();
      r = s->ret;
    } while (r == EXP_REFILL);
  }
  if (lane == 0) exp_row(s, d.offset, &rows[i]);
}

__global__ __launch_bounds__(kLanes) void example_label_rows_kernel(const uint8_t* __restrict__ buf, int64_t buf_bytes,
                                                                    const asm_example_row* __restrict__ rows, int num_classes,
                                                                    uint32_t* __restrict__ out, int ld,
                                                                    int32_t* __restrict__ status) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const asm_example_row r = rows[i];
  const int32_t st = exl_status(r, num_classes, buf_bytes);            // the same for every lane
  if (lane == 0) status[i] = st;
  if (st) return;
  uint32_t* row = out + (int64_t)i * ld;
  for (int64_t col = lane; col < 2 * (int64_t)num_classes; col += kLanes)      // (2 * num_classes <= ld fits an int)
    row[col] = exl_word(buf, r, num_classes, (int)col);
}

}  // namespace

extern "C" int asm_crc32c_spans(const uint8_t* buf, int64_t buf_bytes, const asm_span_desc* spans, int n, uint32_t* crc,
                                int32_t* status, void* stream) {
  ASM_REQUIRE(buf && spans && crc && status, "crc32c_spans: null pointer");
  ASM_REQUIRE(n >= 0, "crc32c_spans: n = %d", n);
  ASM_REQUIRE(buf_bytes >= 0 && buf_bytes <= CRC_MAX_BYTES, "crc32c_spans: buf_bytes outside 0 .. 2^40 - 1");
  if (n == 0) return ASM_OK;
  ASM_LAUNCH(crc32c_spans_kernel, dim3(n), dim3(kLanes), 0, (hipStream_t)stream, buf, buf_bytes, spans, crc, status);
  ASM_CHECK_LAUNCH("crc32c_spans");
  return ASM_OK;
}

extern "C" int asm_example_parse(const uint8_t* buf, int64_t buf_bytes, const asm_span_desc* spans, int n,
                                 asm_example_row* rows, void* stream) {
  ASM_REQUIRE(buf && spans && rows, "example_parse: null pointer");
  ASM_REQUIRE(n >= 0, "example_parse: n = %d", n);
  ASM_REQUIRE(buf_bytes >= 0 && buf_bytes <= EXP_MAX_BYTES, "example_parse: buf_bytes outside 0 .. 2^40 - 1");
  if (n == 0) return ASM_OK;
  ASM_LAUNCH(example_parse_kernel, dim3(n), dim3(EXP_LANES), 0, (hipStream_t)stream, buf, buf_bytes, spans, rows);
  ASM_CHECK_LAUNCH("example_parse");
  return ASM_OK;
}

extern "C" int asm_example_label_rows(const uint8_t* buf, int64_t buf_bytes, const asm_example_row* rows, int n,
                                      int num_classes, float* out, int ld, int32_t* status, void* stream) {
  ASM_REQUIRE(buf && rows && out && status, "example_label_rows: null pointer");
  ASM_REQUIRE(n >= 0 && num_classes >= 1 && (int64_t)ld >= 2 * (int64_t)num_classes,
              "example_label_rows: n = %d, num_classes = %d, ld = %d", n, num_classes, ld);
  ASM_REQUIRE(buf_bytes >= 0 && buf_bytes <= EXP_MAX_BYTES, "example_label_rows: buf_bytes outside 0 .. 2^40 - 1");
  if (n == 0) return ASM_OK;
  ASM_LAUNCH(example_label_rows_kernel, dim3(n), dim3(kLanes), 0, (hipStream_t)stream, buf, buf_bytes, rows, num_classes,
             reinterpret_cast<uint32_t*>(out), ld, status);
  ASM_CHECK_LAUNCH("example_label_rows");
  return ASM_OK;
}
