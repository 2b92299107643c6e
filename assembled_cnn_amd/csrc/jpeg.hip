// JPEG decode on the device for a ragged batch (include/asm_hip.h): three launches, no host round trip.
//   jpeg_entropy_kernel  one 64-lane workgroup per image: Huffman tables -> LDS, coefficient region zeroed, then lane s
//                        decodes restart intervals s, s + 64, ... (jpeg_entropy.h; an image without DRI is one interval,
//                        so one lane works and the batch supplies the parallelism)
//   jpeg_entropy_parallel_kernel  the same stage for asm_jpeg_decode_parallel: one 256-lane workgroup per image decodes
//                        every interval in segments, all lanes at once, to the same coefficients and status
//                        (jpeg_parallel.h)
//   jpeg_progressive_kernel  the entropy stage of progressive files (asm_jpeg_decode_progressive): the same workgroup
//                        walks the image's scans in file order, tables rebuilt in LDS per scan, a barrier between scans
//   jpeg_idct_kernel     one thread per 8x8 block: dequantise + jidctint.c's jpeg_idct_islow -> uint8 planes
//   jpeg_colour_kernel   one thread per pixel: jdsample.c's fancy h2v1 / h2v2 upsampling + jdcolor.c's YCbCr -> RGB
// The entropy kernels open with the same text: jpeg_image_begin, jpeg_image_clear and (sequential, parallel)
// jpeg_baseline_tables; the three entry points share jpeg_call_begin / jpeg_call_finish around their own launch.
// Every index is checked against the image's own geometry and the sizes the caller passed; an image whose entropy decode
// failed (status != 0) gets zeros (a refused descriptor too, as long as its slot in dst fits on its own).
#include "common.h"
#include "jpeg_entropy.h"

static_assert(sizeof(asm_jpeg_desc) == 96 && sizeof(asm_jpeg_huff) == 272 && sizeof(asm_jpeg_tables) == 1600 &&
                  sizeof(asm_jpeg_interval) == 32 && sizeof(asm_jpeg_scan) == 56 && sizeof(jpeg_seg) == 32,
              "JPEG ABI structs");

namespace {

// the descriptor's regions lie inside the buffers of this call
__device__ __forceinline__ bool desc_fits(const asm_jpeg_desc& d, const jpeg_geom& g, long long files_bytes,
                                          long long total_blocks, long long dst_bytes) {
  const long long px = (long long)d.width * d.height * 3;
  return d.scan_offset >= 0 && d.scan_bytes >= 0 && d.scan_offset <= files_bytes - d.scan_bytes && d.coef_offset >= 0 &&
         (d.coef_offset & 63) == 0 && d.coef_offset <= total_blocks * 64 - g.n_coefs && d.plane_offset >= 0 &&
         (d.plane_offset & 7) == 0 && d.plane_offset <= total_blocks * 64 - g.n_coefs && d.dst_offset >= 0 && d.dst_offset <= dst_bytes - px &&
         d.qsel[0] < 4 && d.qsel[1] < 4 && d.qsel[2] < 4 && d.dcsel[0] < 2 && d.dcsel[1] < 2 && d.dcsel[2] < 2 &&
         d.acsel[0] < 2 && d.acsel[1] < 2 && d.acsel[2] < 2;
}

// What every entropy kernel does first: the image's descriptor, its geometry, and whether its regions fit this call.
// Uniform over the workgroup; writes nothing and contains no barrier.  The kernel ANDs its own conditions to the result
// and, on false, leaves with the one write a refused descriptor gets: status[img] = ASM_JPEG_EDESC from lane 0.
__device__ __forceinline__ bool jpeg_image_begin(const asm_jpeg_desc* __restrict__ descs, int img, long long files_bytes,
                                                 long long total_blocks, long long dst_bytes, asm_jpeg_desc* d, jpeg_geom* g) {
  *d = descs[img];
  return jpeg_make_geom(*d, g) && desc_fits(*d, *g, files_bytes, total_blocks, dst_bytes);
}

// What follows acceptance: the zig-zag table into LDS and the image's coefficients zeroed (64 coefficients = 128 bytes
// per block, 16 bytes per store), by `lanes` lanes.  Contains no barrier: the caller's next one publishes both.
__device__ __forceinline__ void jpeg_image_clear(const jpeg_geom& g, uint8_t* zigzag, int16_t* my_coefs, int lane, int lanes) {
  if (lane < 64) {
    const uint8_t zz[64] = JPEG_ZIGZAG_INIT;
    zigzag[lane] = zz[lane];
  }
  uint4* z = reinterpret_cast<uint4*>(my_coefs);
  const long long n16 = g.n_coefs / 8;
  for (long long i = lane; i < n16; i += lanes) z[i] = make_uint4(0u, 0u, 0u, 0u);
}

// The sequential and the parallel kernel after that: status[img] = 0, or ASM_JPEG_ERESTART for an interval count that is
// not the geometry's; the four tables built by lanes 0..3 and their look-ups filled by all lanes.  Contains ONE barrier,
// between the two, which also publishes jpeg_image_clear's stores; the look-ups are published by the caller's next
// barrier.  false (uniform): the count is wrong and the kernel returns -- after that barrier of its own, if it has one.
__device__ __forceinline__ bool jpeg_baseline_tables(const asm_jpeg_desc& d, const jpeg_geom& g, const asm_jpeg_tables& tb,
                                                     jpeg_dtab* tab, int* status_word, int lane, int lanes) {
  const bool counted = d.n_intervals == jpeg_expected_intervals(d.restart_interval, g.n_mcus);
  if (lane == 0) *status_word = counted ? 0 : ASM_JPEG_ERESTART;
  if (lane < 4) jpeg_dtab_prepare(lane < 2 ? tb.dc[lane] : tb.ac[lane - 2], &tab[lane]);
  __syncthreads();
  for (int t = 0; t < 4; ++t) jpeg_dtab_fill_look(&tab[t], lane, lanes);
  return counted;
}

__global__ void __launch_bounds__(64)
jpeg_entropy_kernel(const uint8_t* __restrict__ files, long long files_bytes, const asm_jpeg_desc* __restrict__ descs,
                    const asm_jpeg_tables* __restrict__ tables, const asm_jpeg_interval* __restrict__ intervals,
                    int n_intervals_total, long long total_blocks, long long dst_bytes, int16_t* __restrict__ coefs,
                    int* __restrict__ status) {
  __shared__ jpeg_dtab tab[4];       // dc 0, dc 1, ac 0, ac 1
  __shared__ uint8_t zigzag[64];
  const int img = blockIdx.x, lane = threadIdx.x;
  asm_jpeg_desc d;
  jpeg_geom g;
  const bool ok = jpeg_image_begin(descs, img, files_bytes, total_blocks, dst_bytes, &d, &g) && d.restart_interval >= 0 &&
                  d.first_interval >= 0 && d.n_intervals >= 1 && d.first_interval <= n_intervals_total - d.n_intervals;
  if (!ok) {       // uniform over the workgroup
    if (lane == 0) status[img] = ASM_JPEG_EDESC;
    return;
  }
  int16_t* my_coefs = coefs + d.coef_offset;
  jpeg_image_clear(g, zigzag, my_coefs, lane, 64);
  const bool counted = jpeg_baseline_tables(d, g, tables[img], tab, &status[img], lane, 64);
  __syncthreads();
  if (!counted) return;
  const int err = jpeg_decode_lane(files, d, g, intervals, img, tab, zigzag, lane, 64, my_coefs);
  if (err) atomicOr(&status[img], err);
}

// One scan on many lanes (jpeg_parallel.h): one 256-lane workgroup per image, the image's segments shared out lane,
// lane + 256, ...  Every branch around a barrier is uniform: it depends on the descriptor, on the segment count read
// alike by all lanes, or on a __syncthreads_or.  The state rows live in global memory (an 8192 x 8192 image has more
// segments than LDS holds); the barriers order the workgroup's own traffic to them.
#define JPEG_PAR_LANES 256
__global__ void __launch_bounds__(JPEG_PAR_LANES)
jpeg_entropy_parallel_kernel(const uint8_t* __restrict__ files, long long files_bytes, const asm_jpeg_desc* __restrict__ descs,
                             const asm_jpeg_tables* __restrict__ tables, const asm_jpeg_interval* __restrict__ intervals,
                             int n_intervals_total, const int32_t* __restrict__ seg_first, long long total_segments,
                             int segment_bytes, jpeg_seg* __restrict__ segs, long long total_blocks, long long dst_bytes,
                             int16_t* __restrict__ coefs, int* __restrict__ status, int32_t* __restrict__ info) {
  __shared__ jpeg_dtab tab[4];       // dc 0, dc 1, ac 0, ac 1
  __shared__ uint8_t zigzag[64];
  __shared__ int32_t chain_sum[JPEG_PAR_LANES];
  __shared__ uint32_t dc_sum[3 * JPEG_PAR_LANES];
  __shared__ uint8_t run_flags[JPEG_PAR_LANES];
  const int img = blockIdx.x, lane = threadIdx.x;
  if (info && lane < 2) info[2 * img + lane] = 0;
  jpeg_par_ctx c;
  const asm_jpeg_desc& d = c.d;
  const bool ok = jpeg_image_begin(descs, img, files_bytes, total_blocks, dst_bytes, &c.d, &c.g) && d.restart_interval >= 0 &&
                  d.first_interval >= 0 && d.n_intervals >= 1 && d.first_interval <= n_intervals_total - d.n_intervals;
  if (!ok) {       // uniform over the workgroup
    if (lane == 0) status[img] = ASM_JPEG_EDESC;
    return;
  }
  int16_t* my_coefs = coefs + d.coef_offset;
  jpeg_image_clear(c.g, zigzag, my_coefs, lane, JPEG_PAR_LANES);
  // the look-ups are published by the barrier of the table check below
  if (!jpeg_baseline_tables(d, c.g, tables[img], tab, &status[img], lane, JPEG_PAR_LANES)) return;
  jpeg_par_ctx_fill(&c, files, intervals + d.first_interval, seg_first + d.first_interval, img, segment_bytes, tab, zigzag,
                    my_coefs);
  if (__syncthreads_or(jpeg_par_check_table(c, total_segments, lane, JPEG_PAR_LANES) ? 1 : 0)) {
    if (lane == 0) atomicOr(&status[img], ASM_JPEG_EDESC);
    return;
  }
  c.segs = segs + c.seg_first[0];
  c.n_segs = jpeg_par_segments(c);
  int err = jpeg_par_init(c, lane, JPEG_PAR_LANES);
  __syncthreads();
  // the fixed point: the truth advances at least one segment per round, so n_segs + 1 rounds always suffice
  int rounds = 0;
  for (int more = 1; more && rounds <= c.n_segs; ++rounds) {
    jpeg_par_decode(c, lane, JPEG_PAR_LANES);
    __syncthreads();
    more = __syncthreads_or(jpeg_par_publish(c, lane, JPEG_PAR_LANES) ? 1 : 0);
  }
  jpeg_par_chain_sum(c, lane, JPEG_PAR_LANES, chain_sum, run_flags);
  __syncthreads();
  jpeg_par_chain_apply(c, lane, JPEG_PAR_LANES, chain_sum, run_flags);
  __syncthreads();
  err |= jpeg_par_write(c, lane, JPEG_PAR_LANES);
  __syncthreads();
  jpeg_par_dc_sum(c, lane, JPEG_PAR_LANES, dc_sum, run_flags);
  __syncthreads();
  jpeg_par_dc_apply(c, lane, JPEG_PAR_LANES, dc_sum, run_flags);
  if (err) atomicOr(&status[img], err);
  if (info && lane == 0) {
    info[2 * img] = c.n_segs;
    info[2 * img + 1] = rounds;
  }
}

// Progressive files: the scans of one image one after another.  One workgroup is one wave on one CU, so the barrier
// between scans is all the ordering the coefficient traffic needs (a refinement scan reads what earlier scans stored).
// Every loop bound around a barrier is uniform: the scan count and the table count come from rows all lanes read alike.
// A lane that has seen an error stops decoding and keeps arriving at the barriers.
__global__ void __launch_bounds__(64)
jpeg_progressive_kernel(const uint8_t* __restrict__ files, long long files_bytes, const asm_jpeg_desc* __restrict__ descs,
                        const asm_jpeg_scan* __restrict__ scans, int n_scans_total, const asm_jpeg_huff* __restrict__ huff,
                        int n_huff, const asm_jpeg_interval* __restrict__ intervals, int n_intervals_total,
                        long long total_blocks, long long dst_bytes, int16_t* __restrict__ coefs,
                        int* __restrict__ status) {
  __shared__ jpeg_dtab tab[3];       // DC-first scan: one per scan component; AC scan: [0]
  __shared__ uint8_t zigzag[64];
  __shared__ int failed;             // some lane has seen an error: the scans that follow are skipped
  const int img = blockIdx.x, lane = threadIdx.x;
  asm_jpeg_desc d;
  jpeg_geom g;
  const bool fits = jpeg_image_begin(descs, img, files_bytes, total_blocks, dst_bytes, &d, &g);
  // first_interval / n_intervals name the image's rows of the scan table here
  const int first_scan = d.first_interval, n_scans = d.n_intervals;
  const bool ok = fits && d.restart_interval == 0 &&
                  (d.dcsel[0] | d.dcsel[1] | d.dcsel[2] | d.acsel[0] | d.acsel[1] | d.acsel[2]) == 0 && d.reserved == 0 &&
                  first_scan >= 0 && n_scans >= 1 && n_scans <= 256 && first_scan <= n_scans_total - n_scans;
  if (!ok) {       // uniform over the workgroup
    if (lane == 0) status[img] = ASM_JPEG_EDESC;
    return;
  }
  if (lane == 0) {
    status[img] = 0;
    failed = 0;
  }
  int16_t* my_coefs = coefs + d.coef_offset;
  jpeg_image_clear(g, zigzag, my_coefs, lane, 64);
  __syncthreads();
  int err = 0;
  for (int k = 0; k < n_scans; ++k) {
    const asm_jpeg_scan sc = scans[first_scan + k];
    const bool skip = failed != 0;       // written before the barrier that ended the previous scan: uniform
    jpeg_scan_geom sg;
    const int n_tab = jpeg_scan_tables(sc);
    const int scan_err = skip ? 0 : jpeg_check_scan(d, g, sc, img, n_huff, n_intervals_total, &sg);
    const bool run = !skip && scan_err == 0;      // uniform: every lane read the same rows
    if (run && lane < n_tab) jpeg_dtab_prepare(huff[sc.huff[lane]], &tab[lane]);
    __syncthreads();
    if (run)
      for (int t = 0; t < n_tab; ++t) jpeg_dtab_fill_look(&tab[t], lane, 64);
    __syncthreads();
    if (run && err == 0)
      err = jpeg_prog_decode_lane(files, g, sc, sg, intervals, img, tab, zigzag, lane, 64, my_coefs);
    err |= scan_err;
    if (err) failed = 1;
    __syncthreads();
  }
  if (err) atomicOr(&status[img], err);
}

// jidctint.c: CONST_BITS 13, PASS1_BITS 2; FIX(x) = round(x * 2^13)
#define FIX_0_298631336 2446
#define FIX_0_390180644 3196
#define FIX_0_541196100 4433
#define FIX_0_765366865 6270
#define FIX_0_899976223 7373
#define FIX_1_175875602 9633
#define FIX_1_501321110 12299
#define FIX_1_847759065 15137
#define FIX_1_961570560 16069
#define FIX_2_053119869 16819
#define FIX_2_562915447 20995
#define FIX_3_072711026 25172

// one 1-D pass of jpeg_idct_islow on eight values: out = DESCALE(..., shift).  64-bit intermediates: a legal file never
// leaves 32 bits, and no bit string can make this overflow.
__device__ __forceinline__ void islow_1d(const long long (&in)[8], int shift, long long (&out)[8]) {
  long long z1 = (in[2] + in[6]) * FIX_0_541196100;
  long long tmp2 = z1 + in[6] * (-FIX_1_847759065);
  long long tmp3 = z1 + in[2] * FIX_0_765366865;
  long long tmp0 = (in[0] + in[4]) * 8192;
  long long tmp1 = (in[0] - in[4]) * 8192;
  const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7];
  tmp1 = in[5];
  tmp2 = in[3];
  tmp3 = in[1];
  z1 = tmp0 + tmp3;
  long long z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
  const long long z5 = (z3 + z4) * FIX_1_175875602;
  tmp0 *= FIX_0_298631336;
  tmp1 *= FIX_2_053119869;
  tmp2 *= FIX_3_072711026;
  tmp3 *= FIX_1_501321110;
  z1 *= -FIX_0_899976223;
  z2 *= -FIX_2_562915447;
  z3 *= -FIX_1_961570560;
  z4 *= -FIX_0_390180644;
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  const long long r = 1ll << (shift - 1);
  out[0] = (tmp10 + tmp3 + r) >> shift;
  out[7] = (tmp10 - tmp3 + r) >> shift;
  out[1] = (tmp11 + tmp2 + r) >> shift;
  out[6] = (tmp11 - tmp2 + r) >> shift;
  out[2] = (tmp12 + tmp1 + r) >> shift;
  out[5] = (tmp12 - tmp1 + r) >> shift;
  out[3] = (tmp13 + tmp0 + r) >> shift;
  out[4] = (tmp13 - tmp0 + r) >> shift;
}

__global__ void __launch_bounds__(64)
jpeg_idct_kernel(const asm_jpeg_desc* __restrict__ descs, const asm_jpeg_tables* __restrict__ tables, long long files_bytes,
                 long long total_blocks, long long dst_bytes, const int16_t* __restrict__ coefs,
                 const int* __restrict__ status, uint8_t* __restrict__ planes) {
  const int img = blockIdx.y;
  const long long blk = (long long)blockIdx.x * 64 + threadIdx.x;
  if (status[img] != 0) return;
  const asm_jpeg_desc d = descs[img];
  jpeg_geom g;
  if (!jpeg_make_geom(d, &g) || !desc_fits(d, g, files_bytes, total_blocks, dst_bytes)) return;
  if (blk * 64 >= g.n_coefs) return;
  int c = 0;
  if (d.ncomp == 3) c = blk * 64 >= g.base[2] ? 2 : blk * 64 >= g.base[1] ? 1 : 0;
  const long long local = blk - g.base[c] / 64;
  const int by = (int)(local / g.bw[c]), bx = (int)(local - (long long)by * g.bw[c]);
  const uint16_t* q = tables[img].quant[d.qsel[c]];
  // 64 coefficients = eight 16-byte rows (coef_offset is a multiple of 64 and the workspace 16-byte aligned)
  const uint4* in = reinterpret_cast<const uint4*>(coefs + d.coef_offset + blk * 64);
  int ws[8][8];             // [row][column] after the column pass
  int cf[8][8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint4 w = in[r];
    const unsigned u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      cf[r][2 * x] = (int)(short)(u[x] & 0xFFFFu) * (int)min((unsigned)q[r * 8 + 2 * x], 255u);
      cf[r][2 * x + 1] = (int)(short)(u[x] >> 16) * (int)min((unsigned)q[r * 8 + 2 * x + 1], 255u);
    }
  }
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    long long v[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = cf[r][col];
    islow_1d(v, 11, o);       // CONST_BITS - PASS1_BITS
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[r][col] = (int)o[r];
  }
  // the component's plane: [blocks high * 8][bw * 8] uint8
  const int pitch = g.bw[c] * 8;
  uint8_t* out = planes + d.plane_offset + g.base[c] + ((long long)by * 8 * pitch + bx * 8);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    long long v[8], o[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) v[x] = ws[r][x];
    islow_1d(v, 18, o);   // CONST_BITS + PASS1_BITS + 3
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      lo |= (unsigned)min(max(o[x] + 128, 0ll), 255ll) << (8 * x);
      hi |= (unsigned)min(max(o[x + 4] + 128, 0ll), 255ll) << (8 * x);
    }
    *reinterpret_cast<uint2*>(out + (long long)r * pitch) = make_uint2(lo, hi);
  }
}

// jdcolor.c build_ycc_rgb_table: SCALEBITS 16, ONE_HALF 32768
__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// chroma sample for output pixel (x, y) from a plane of true size cw x ch (pitch bytes per row)
__device__ __forceinline__ int chroma_at(const uint8_t* p, int pitch, int cw, int ch, int hs, int vs, int x, int y) {
  if (hs == 1) return p[(long long)y * pitch + x];
  const int cx = x >> 1;
  if (vs == 1) {
    const int c = p[(long long)y * pitch + cx];
    if (cw <= 2) return c;                               // jdsample.c: fancy only for more than two columns
    if (x & 1) return cx == cw - 1 ? c : (3 * c + p[(long long)y * pitch + cx + 1] + 2) >> 2;
    return cx == 0 ? c : (3 * c + p[(long long)y * pitch + cx - 1] + 1) >> 2;
  }
  const int cy = y >> 1;
  if (cw <= 2) return p[(long long)cy * pitch + cx];
  // the nearer row weighs 3, the other (above for an even output row, below for an odd one; itself at the edge) 1
  const int oy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
  const uint8_t* r0 = p + (long long)cy * pitch;
  const uint8_t* r1 = p + (long long)oy * pitch;
  const int s = 3 * r0[cx] + r1[cx];
  if (x & 1) return cx == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * r0[cx + 1] + r1[cx + 1] + 7) >> 4;
  return cx == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * r0[cx - 1] + r1[cx - 1] + 8) >> 4;
}

__global__ void __launch_bounds__(256)
jpeg_colour_kernel(const asm_jpeg_desc* __restrict__ descs, long long files_bytes, long long total_blocks,
                   long long dst_bytes, const int* __restrict__ status, const uint8_t* __restrict__ planes,
                   uint8_t* __restrict__ dst) {
  const int img = blockIdx.y;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  const asm_jpeg_desc d = descs[img];
  jpeg_geom g;
  // the image's slot in dst, judged on its own: width, height and dst_offset alone
  const bool slot_ok = d.width >= 1 && d.height >= 1 && d.width <= 8192 && d.height <= 8192 && d.dst_offset >= 0 &&
                       d.dst_offset <= dst_bytes - (long long)d.width * d.height * 3;
  if (!slot_ok || p >= (long long)d.width * d.height) return;
  uint8_t* o = dst + d.dst_offset + p * 3;
  // a descriptor the entropy kernel refused (ASM_JPEG_EDESC) still gets its zeros where the slot fits
  const bool desc_ok = jpeg_make_geom(d, &g) && desc_fits(d, g, files_bytes, total_blocks, dst_bytes);
  if (!desc_ok || status[img] != 0) {
    o[0] = o[1] = o[2] = 0;
    return;
  }
  const int y = (int)(p / d.width), x = (int)(p - (long long)y * d.width);
  const uint8_t* base = planes + d.plane_offset;
  const int Y = base[(long long)y * (g.bw[0] * 8) + x];
  if (d.ncomp == 1) {
    o[0] = o[1] = o[2] = (uint8_t)Y;
    return;
  }
  const int cw = (d.width + d.hs - 1) / d.hs, ch = (d.height + d.vs - 1) / d.vs;
  const int cb = chroma_at(base + g.base[1], g.bw[1] * 8, cw, ch, d.hs, d.vs, x, y) - 128;
  const int cr = chroma_at(base + g.base[2], g.bw[2] * 8, cw, ch, d.hs, d.vs, x, y) - 128;
  o[0] = (uint8_t)clamp255(Y + ((91881 * cr + 32768) >> 16));
  o[1] = (uint8_t)clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  o[2] = (uint8_t)clamp255(Y + ((116130 * cb + 32768) >> 16));
}

}  // namespace

// workspace of a call: int16 coefficients, then uint8 planes, per 8x8 block (both multiples of 16 bytes)
#define JPEG_COEF_BYTES_PER_BLOCK 128
#define JPEG_PLANE_BYTES_PER_BLOCK 64
static int64_t jpeg_workspace_bytes(int64_t total_blocks) {
  return total_blocks * (JPEG_COEF_BYTES_PER_BLOCK + JPEG_PLANE_BYTES_PER_BLOCK);
}

extern "C" int asm_jpeg_decode_workspace_bytes(int64_t total_blocks, int64_t* bytes) {
  ASM_REQUIRE(bytes && total_blocks >= 0 && total_blocks < (1ll << 36), "jpeg_decode_workspace_bytes: bad sizes");
  *bytes = jpeg_workspace_bytes(total_blocks);
  return ASM_OK;
}

extern "C" int asm_jpeg_decode_parallel_workspace_bytes(int64_t total_blocks, int64_t total_segments, int64_t* bytes) {
  ASM_REQUIRE(bytes && total_blocks >= 0 && total_blocks < (1ll << 36) && total_segments >= 0 &&
                  total_segments < (1ll << 30),
              "jpeg_decode_parallel_workspace_bytes: bad sizes");
  *bytes = jpeg_workspace_bytes(total_blocks) + total_segments * (int64_t)sizeof(jpeg_seg);
  return ASM_OK;
}

// the inverse DCT and the colour launch for N rows whose coefficients are in place (every entry point ends here)
static int launch_pixel_stages(const asm_jpeg_desc* descs, const asm_jpeg_tables* tables, int N, int64_t files_bytes,
                               int64_t total_blocks, int max_blocks, int max_pixels, uint8_t* dst, int64_t dst_bytes,
                               const int32_t* status, const int16_t* coefs, uint8_t* planes, hipStream_t s) {
  if (max_blocks > 0) {
    ASM_LAUNCH(jpeg_idct_kernel, dim3((max_blocks + 63) / 64, N), dim3(64), 0, s, descs, tables, files_bytes,
               total_blocks, dst_bytes, coefs, status, planes);
    ASM_CHECK_LAUNCH("jpeg_decode (idct)");
  }
  if (max_pixels > 0) {
    ASM_LAUNCH(jpeg_colour_kernel, dim3((max_pixels + 255) / 256, N), dim3(256), 0, s, descs, files_bytes, total_blocks,
               dst_bytes, status, planes, dst);
    ASM_CHECK_LAUNCH("jpeg_decode (colour)");
  }
  return ASM_OK;
}

// The arguments the three entry points have in common, and what jpeg_call_begin carves from the workspace.
struct jpeg_call {
  const uint8_t* files;
  const asm_jpeg_desc* descs;
  const asm_jpeg_tables* tables;
  uint8_t* dst;
  int32_t* status;
  void* workspace;
  int64_t files_bytes, dst_bytes, total_blocks, workspace_bytes;
  int N, max_blocks, max_pixels, stages;
  hipStream_t s;
  int16_t* coefs;       // workspace
  uint8_t* planes;      // workspace + total_blocks * JPEG_COEF_BYTES_PER_BLOCK
};

// What the entry points check alike, in their order: sizes (own_sizes_ok: the entry point's own counts), own_error (null,
// or what is wrong with an argument only this entry point has), stages, N, the workspace (own_bytes: what the entry point
// keeps behind coefficients and planes); nothing more for N == 0; then the pointers (own_pointers: the entry point's own
// tables) and the alignment.  `name` keeps every message the entry point's.
static int jpeg_call_begin(const char* name, jpeg_call* c, bool own_sizes_ok, const char* own_error, bool own_pointers,
                           int64_t own_bytes) {
  ASM_REQUIRE(c->N >= 0 && c->files_bytes >= 0 && c->dst_bytes >= 0 && c->total_blocks >= 0 && c->total_blocks < (1ll << 36) &&
                  c->max_blocks >= 0 && c->max_pixels >= 0 && own_sizes_ok,
              "%s: bad sizes", name);
  ASM_REQUIRE(!own_error, "%s: %s", name, own_error);
  ASM_REQUIRE(c->stages >= 1 && c->stages <= 3, "%s: stages must be 1, 2 or 3", name);
  ASM_REQUIRE(c->N <= 65535, "%s: at most 65535 images per call", name);
  ASM_REQUIRE(c->workspace_bytes >= jpeg_workspace_bytes(c->total_blocks) + own_bytes, "%s: workspace too small", name);
  if (c->N == 0) return ASM_OK;
  ASM_REQUIRE(c->files && c->descs && c->tables && own_pointers && c->dst && c->status && c->workspace, "%s: null pointer",
              name);
  ASM_REQUIRE(((uintptr_t)c->workspace & 15) == 0, "%s: workspace must be 16-byte aligned", name);
  c->coefs = (int16_t*)c->workspace;
  c->planes = (uint8_t*)c->workspace + c->total_blocks * JPEG_COEF_BYTES_PER_BLOCK;
  return ASM_OK;
}

// after the entry point's own entropy launch
static int jpeg_call_finish(const jpeg_call& c) {
  if (!(c.stages & 2)) return ASM_OK;
  return launch_pixel_stages(c.descs, c.tables, c.N, c.files_bytes, c.total_blocks, c.max_blocks, c.max_pixels, c.dst,
                             c.dst_bytes, c.status, c.coefs, c.planes, c.s);
}

extern "C" int asm_jpeg_decode(const uint8_t* files, int64_t files_bytes, const asm_jpeg_desc* descs,
                               const asm_jpeg_tables* tables, const asm_jpeg_interval* intervals, int N, int n_intervals,
                               int64_t total_blocks, int max_blocks, int max_pixels, uint8_t* dst, int64_t dst_bytes,
                               int32_t* status, void* workspace, int64_t workspace_bytes, int stages, void* stream) {
  jpeg_call c = {files, descs, tables, dst, status, workspace, files_bytes, dst_bytes, total_blocks, workspace_bytes,
                 N, max_blocks, max_pixels, stages, (hipStream_t)stream, nullptr, nullptr};
  const int rc = jpeg_call_begin("jpeg_decode", &c, n_intervals >= 0, nullptr, intervals != nullptr, 0);
  if (rc != ASM_OK || N == 0) return rc;
  if (stages & 1) {
    ASM_LAUNCH(jpeg_entropy_kernel, dim3(N), dim3(64), 0, c.s, files, files_bytes, descs, tables, intervals, n_intervals,
               total_blocks, dst_bytes, c.coefs, status);
    ASM_CHECK_LAUNCH("jpeg_decode (entropy)");
  }
  return jpeg_call_finish(c);
}

extern "C" int asm_jpeg_decode_parallel(const uint8_t* files, int64_t files_bytes, const asm_jpeg_desc* descs,
                                        const asm_jpeg_tables* tables, const asm_jpeg_interval* intervals,
                                        const int32_t* segment_first, int N, int n_intervals, int64_t total_segments,
                                        int segment_bytes, int64_t total_blocks, int max_blocks, int max_pixels,
                                        uint8_t* dst, int64_t dst_bytes, int32_t* status, int32_t* info, void* workspace,
                                        int64_t workspace_bytes, int stages, void* stream) {
  jpeg_call c = {files, descs, tables, dst, status, workspace, files_bytes, dst_bytes, total_blocks, workspace_bytes,
                 N, max_blocks, max_pixels, stages, (hipStream_t)stream, nullptr, nullptr};
  const bool segment_ok = segment_bytes >= 16 && segment_bytes <= 65536 && segment_bytes % 16 == 0;
  const int rc = jpeg_call_begin(
      "jpeg_decode_parallel", &c,
      n_intervals >= 0 && files_bytes < (1ll << 40) && total_segments >= 0 && total_segments < (1ll << 30),
      segment_ok ? nullptr : "segment_bytes must be a multiple of 16 in 16..65536", intervals && segment_first,
      total_segments * (int64_t)sizeof(jpeg_seg));
  if (rc != ASM_OK || N == 0) return rc;
  // the state rows follow the planes; 16-byte aligned: both per-block sizes are multiples of 16
  jpeg_seg* segs = (jpeg_seg*)((uint8_t*)workspace + jpeg_workspace_bytes(total_blocks));
  if (stages & 1) {
    ASM_LAUNCH(jpeg_entropy_parallel_kernel, dim3(N), dim3(JPEG_PAR_LANES), 0, c.s, files, files_bytes, descs, tables,
               intervals, n_intervals, segment_first, total_segments, segment_bytes, segs, total_blocks, dst_bytes, c.coefs,
               status, info);
    ASM_CHECK_LAUNCH("jpeg_decode_parallel (entropy)");
  }
  return jpeg_call_finish(c);
}

extern "C" int asm_jpeg_decode_progressive(const uint8_t* files, int64_t files_bytes, const asm_jpeg_desc* descs,
                                           const asm_jpeg_tables* tables, const asm_jpeg_scan* scans,
                                           const asm_jpeg_huff* huff, const asm_jpeg_interval* intervals, int N, int n_scans,
                                           int n_huff, int n_intervals, int64_t total_blocks, int max_blocks, int max_pixels,
                                           uint8_t* dst, int64_t dst_bytes, int32_t* status, void* workspace,
                                           int64_t workspace_bytes, int stages, void* stream) {
  jpeg_call c = {files, descs, tables, dst, status, workspace, files_bytes, dst_bytes, total_blocks, workspace_bytes,
                 N, max_blocks, max_pixels, stages, (hipStream_t)stream, nullptr, nullptr};
  const int rc = jpeg_call_begin("jpeg_decode_progressive", &c, n_scans >= 0 && n_huff >= 0 && n_intervals >= 0, nullptr,
                                 scans && huff && intervals, 0);
  if (rc != ASM_OK || N == 0) return rc;
  if (stages & 1) {
    ASM_LAUNCH(jpeg_progressive_kernel, dim3(N), dim3(64), 0, c.s, files, files_bytes, descs, scans, n_scans, huff, n_huff,
               intervals, n_intervals, total_blocks, dst_bytes, c.coefs, status);
    ASM_CHECK_LAUNCH("jpeg_decode_progressive (entropy)");
  }
  return jpeg_call_finish(c);
}
