// Batch-norm kernels for NHWC bf16 activations viewed as [M, C] (HBM-bound, 16-byte vectors).
// Reductions are two-level and atomics-free: per-block partials [blocks][2][C] (the same layout the
// conv epilogue emits) followed by a tiny finalize that sums the partials in fp64.
#include "common.h"
#include <stdlib.h>


// Cache policy of the streaming kernels (same-box A/B, whole step): the APPLY passes read and write with non-temporal
// hints (their operands are dead afterwards / the result is consumed by a convolution that streams it once): -0.3 ms per
// step in round 1.  The backward REDUCE passes load dy / x plainly (round 4): the apply pass behind them re-reads exactly
// these bytes, and what still sits in L2 / the memory-side cache then is served from there -- 26.42 -> 26.17 ms per step;
// plain stores in the apply passes measured +0.1 .. 0.2 ms.
#define BN_LD_RED(p) (*(p))
#define BN_ST_BWD(v, p) __builtin_nontemporal_store(v, p)
#define BN_ST_FWD(v, p) __builtin_nontemporal_store(v, p)

namespace {

struct RowTiling {
  int vcols;      // C / 8
  int vcb;        // vector columns handled concurrently (<= 256)
  int rpb;        // row lanes per block
  int rows_per_block;
  int blocks;     // row blocks = partial rows per channel
  int slices;     // channel slices: a workgroup reduces rows_per_block rows of ONE slice (grid = blocks * slices)
  int vc_slice;   // vector columns per slice
};

RowTiling make_tiling(int M, int C) {
  RowTiling t;
  t.vcols = C / 8;
  // Channel slices (round 4).  The reducers want ~1024 workgroups (4 per CU: with 512 they ran at 4.4 TB/s, with 1024 at
  // 5.7 TB/s -- occupancy-bound streaming), and until now every workgroup covered ALL channels of its rows: 1024 partial
  // rows per channel, which the finalize kernel behind the reducer walks as a chain of dependent L2 round trips (16 rows
  // per lane: 6.5 us for a launch that moves a few hundred KB, ~80 such launches per backward pass).  With the channels
  // cut into slices of >= 64 (a row segment stays a whole 128-byte line) the same 1024 workgroups leave 1024 / slices
  // partial rows per channel.
  const int want = 8;
  int sl = t.vcols / 8;
  if (sl > want) sl = want;
  if (sl < 1) sl = 1;
  t.slices = sl;
  t.vc_slice = cdiv(t.vcols, sl);
  t.vcb = t.vc_slice < 256 ? t.vc_slice : 256;
  t.rpb = 256 / t.vcb;
  const int cap = asm_tune().bn_rows / sl > 0 ? asm_tune().bn_rows / sl : 1;
  int rows = cdiv(M, cap);
  rows = cdiv(rows, t.rpb) * t.rpb;
  if (rows < t.rpb * 4) rows = t.rpb * 4;
  t.rows_per_block = rows;
  t.blocks = cdiv(M, rows);
  // Which rows a workgroup takes: workgroup b takes the row tiles b, b + blocks, b + 2 blocks, ... (a tile = rpb x 2 rows), the
  // way the apply passes' grid-stride loops sweep ONE compact window over the tensor.  (One contiguous block of rows each --
  // rounds 1 - 3 -- put ~1000 streams M / blocks rows apart: 1.6 MB for the 56 x 56 x 256 tensor, a multiple of 32 KB, so in lock
  // step they asked the same HBM channels for different DRAM pages: 4.3 - 4.5 TB/s against 6.2.)
  return t;
}

// ---- row reductions: NSTAT sums per channel over the rows of [M, C] ----------------------------------------------------
// One skeleton for the three reducers.  Thread = (vector column vc0, row lane rr); a workgroup reduces the row tiles of its
// row block in ONE channel slice and writes one partial row.  `Row` owns what differs: a thread's per-column setup
// (setup(vc)), the operands of one row (load(ld, element offset, mask-byte index)), their accumulation into acc[NSTAT][8]
// (accum(ld, acc)) and where statistic `which` of channel ch in row block rblk is stored (store(rblk, which, ch, v)).
template <int NSTAT, class Row>
__device__ __forceinline__ void row_reduce(Row row, int M, int C, const RowTiling& t) {
  __shared__ float red[NSTAT * 2048];   // NSTAT stats x 256 threads x 8 lanes
  const int tid = threadIdx.x;
  const int vc0 = tid % t.vcb;
  const int rr = tid / t.vcb;
  const bool active = rr < t.rpb;
  const int rblk = blockIdx.x / t.slices, slice = blockIdx.x - rblk * t.slices;
  const int vc_lo = slice * t.vc_slice, vc_hi = min(t.vcols, vc_lo + t.vc_slice);
  constexpr int U = 2;
  const int row_begin = rblk * (U * t.rpb);
  const int row_end = M;
  const int row_step = t.blocks * (U * t.rpb);
  for (int vcbase = vc_lo; vcbase < vc_hi; vcbase += t.vcb) {
    const int vc = vcbase + vc0;
    float acc[NSTAT][8];
#pragma unroll
    for (int q = 0; q < NSTAT; ++q)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[q][e] = 0.f;
    if (active && vc < vc_hi) {
      row.setup(vc);
      // 2 rows per trip (4 was ~5 % slower, 8 ~35 %: registers cost occupancy): all loads of a trip are issued before any is consumed (the reduction is
      // bandwidth-bound only if enough bytes are in flight per CU)
      for (int r0 = row_begin + rr; r0 < row_end; r0 += row_step) {
        typename Row::Loaded ld[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int r = r0 + u * t.rpb;
          const size_t rq = (size_t)(r < row_end ? r : r0);   // the tail re-loads row r0 and is not consumed
          row.load(ld[u], rq * C + vc * 8, rq * t.vcols + vc);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (r0 + u * t.rpb >= row_end) break;
          row.accum(ld[u], acc);
        }
      }
    }
    __syncthreads();   // the previous column group's sums have been read
    row_lanes_sum<NSTAT>(red, acc, active, vc0, rr, t.rpb, t.vcb * 8, [&](int which, int col, float v) {
      const int ch = vcbase * 8 + col;
      if (ch < vc_hi * 8) row.store(rblk, which, ch, v);
    });
  }
}

// (sum x, sum x^2) -> partial [blocks][2][C]
struct StatsRow {
  const bf16_t* __restrict__ x;
  float* __restrict__ partial;
  int C;
  struct Loaded { u32x4 vx; };
  __device__ __forceinline__ void setup(int) {}
  __device__ __forceinline__ void load(Loaded& ld, size_t off, size_t) const {
    ld.vx = BN_LD_RED(reinterpret_cast<const u32x4*>(x + off));
  }
  __device__ __forceinline__ void accum(const Loaded& ld, float (&acc)[2][8]) const {
    float f[8];
    unpack8(ld.vx, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      acc[0][e] += f[e];
      acc[1][e] += f[e] * f[e];
    }
  }
  __device__ __forceinline__ void store(int rblk, int which, int ch, float v) const {
    partial[((size_t)rblk * 2 + which) * C + ch] = v;
  }
};

// (sum dz, sum dz * xhat) -> partial [blocks][2][C]; dz = dy masked by relu: 0 none, 1 the bf16 forward output > 0,
// 2 the packed ReLU mask (yout is then the mask bytes)
struct BwdRow {
  const bf16_t* __restrict__ dy;
  const bf16_t* __restrict__ x;
  const bf16_t* __restrict__ yout;
  int relu;
  const float* __restrict__ mean;
  const float* __restrict__ invstd;
  float* __restrict__ partial;
  int C;
  float mu[8], is[8];
  struct Loaded { u32x4 vg, vx, vy; unsigned mk; };
  __device__ __forceinline__ void setup(int vc) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      mu[e] = mean[vc * 8 + e];
      is[e] = invstd[vc * 8 + e];
    }
  }
  __device__ __forceinline__ void load(Loaded& ld, size_t off, size_t mi) const {
    ld.vg = BN_LD_RED(reinterpret_cast<const u32x4*>(dy + off));
    ld.vx = BN_LD_RED(reinterpret_cast<const u32x4*>(x + off));
    if (relu == 1) ld.vy = *reinterpret_cast<const u32x4*>(yout + off);
    if (relu == 2) ld.mk = reinterpret_cast<const uint8_t*>(yout)[mi];
  }
  __device__ __forceinline__ void accum(const Loaded& ld, float (&acc)[2][8]) const {
    float g[8], fx[8];
    unpack8(ld.vg, g);
    unpack8(ld.vx, fx);
    if (relu == 1) {
      float fy[8];
      unpack8(ld.vy, fy);
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] = fy[e] > 0.f ? g[e] : 0.f;
    } else if (relu == 2) {
      mask8(g, ld.mk);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      acc[0][e] += g[e];
      acc[1][e] += g[e] * ((fx[e] - mu[e]) * is[e]);
    }
  }
  __device__ __forceinline__ void store(int rblk, int which, int ch, float v) const {
    partial[((size_t)rblk * 2 + which) * C + ch] = v;
  }
};

__global__ __launch_bounds__(256) void bn_stats_kernel(const bf16_t* __restrict__ x, int M, int C, RowTiling t,
                                                       float* __restrict__ partial) {
  row_reduce<2>(StatsRow{x, partial, C}, M, C, t);
}

__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                            const bf16_t* __restrict__ yout, int relu, int M, int C,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, RowTiling t,
                                                            float* __restrict__ partial) {
  row_reduce<2>(BwdRow{dy, x, yout, relu, mean, invstd, partial, C}, M, C, t);
}


// ---- finalize: partials -> per-channel statistics / coefficients --------------------------------
// block = 16 channels x FL partial-lanes.  These kernels are pure latency (one per BN layer and direction, ~200 per
// step): 64 lanes keep the dependent trip count at <= 4 for the <= 512 partial rows the reducers emit.
constexpr int FL = 64;
// Rows b0 + lane, b0 + lane + nl, ... < b1 of the [blocks][2][C] partials for channel ch, summed in fp64.  SU row pairs
// (2 * SU loads) are issued before any is consumed: the serial form was a chain of dependent L2 / HBM round trips -- ~5-6 us
// per finalize launch, ~190 such launches per training step.  The summation order is fixed (bit-reproducible).
constexpr int SU = 8;
__device__ __forceinline__ void sum_rows(const float* __restrict__ partial, int b0, int b1, int lane, int nl, int C, int ch,
                                         double& s0, double& s1) {
  double a[SU], c[SU];
#pragma unroll
  for (int u = 0; u < SU; ++u) a[u] = c[u] = 0.0;
  int b = b0 + lane;
  for (; b + (SU - 1) * nl < b1; b += SU * nl) {
    float v0[SU], v1[SU];
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      v0[u] = partial[((size_t)(b + u * nl) * 2 + 0) * C + ch];
      v1[u] = partial[((size_t)(b + u * nl) * 2 + 1) * C + ch];
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      a[u] += (double)v0[u];
      c[u] += (double)v1[u];
    }
  }
  {   // tail: up to SU - 1 rows, still issued together
    float v0[SU], v1[SU];
#pragma unroll
    for (int u = 0; u < SU - 1; ++u) {
      const bool ok = b + u * nl < b1;
      v0[u] = ok ? partial[((size_t)(b + u * nl) * 2 + 0) * C + ch] : 0.f;
      v1[u] = ok ? partial[((size_t)(b + u * nl) * 2 + 1) * C + ch] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < SU - 1; ++u) {
      a[u] += (double)v0[u];
      c[u] += (double)v1[u];
    }
  }
  s0 = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  s1 = ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7]));
}
// finalize kernels: two independent chains per lane.  (Issuing all 16 rows of a lane at once, as sum_rows does, was
// measured SLOWER here -- 12.5 vs 6.5 us for the 1024-row backward partials -- while it helps the compaction, whose lanes
// walk hundreds of rows.)
__device__ __forceinline__ void sum_partials(const float* partial, int blocks, int C, int ch, int ry,
                                             double& s0, double& s1) {
  s0 = 0.0;
  s1 = 0.0;
  if (ch < C) {
    double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
    int b = ry;
    for (; b + FL < blocks; b += 2 * FL) {   // two independent chains: loads overlap
      a0 += (double)partial[((size_t)b * 2 + 0) * C + ch];
      b0 += (double)partial[((size_t)b * 2 + 1) * C + ch];
      a1 += (double)partial[((size_t)(b + FL) * 2 + 0) * C + ch];
      b1 += (double)partial[((size_t)(b + FL) * 2 + 1) * C + ch];
    }
    if (b < blocks) {
      a0 += (double)partial[((size_t)b * 2 + 0) * C + ch];
      b0 += (double)partial[((size_t)b * 2 + 1) * C + ch];
    }
    s0 = a0 + a1;
    s1 = b0 + b1;
  }
}

// partial compaction: [blocks][2][C] -> [groups][2][C]; each output group sums a contiguous range of
// input blocks (fp64 accumulate).  Keeps the finalize kernels short when a conv epilogue emitted
// thousands of 128-row partials (25088 for the 112x112 stem at batch 256).
__global__ __launch_bounds__(16 * FL) void partials_compact_kernel(const float* __restrict__ in, int blocks, int C,
                                                                   float* __restrict__ out, int per_group) {
  __shared__ double red[2][FL][16];
  const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const int ch = blockIdx.x * 16 + cx;
  const int b0 = blockIdx.y * per_group;
  const int b1 = min(blocks, b0 + per_group);
  double s0 = 0.0, s1 = 0.0;
  if (ch < C) sum_rows(in, b0, b1, ry, FL, C, ch, s0, s1);
  fl_stage(red, ry, cx, s0, s1);
  if (ry < 2 && ch < C) out[((size_t)blockIdx.y * 2 + ry) * C + ch] = (float)fl_sum(red, ry, cx);
}

// One channel's forward statistics from its sums over the M rows (fp64): mean, clamped biased variance, invstd, the
// Bessel-corrected moving update; -> scale = gamma * invstd, shift = beta - mean * scale.
__device__ __forceinline__ void bn_fwd_channel(double sum, double sumsq, int M, int ch, const float* __restrict__ gamma,
                                               const float* __restrict__ beta, float eps, float momentum,
                                               float* moving_mean, float* moving_var, float* mean, float* invstd,
                                               float& sc, float& sh) {
  const double mu = sum / (double)M;
  double var = sumsq / (double)M - mu * mu;
  if (var < 0.0) var = 0.0;
  const float is = (float)(1.0 / sqrt(var + (double)eps));
  const float s = gamma[ch] * is;
  sc = s;
  sh = beta[ch] - (float)mu * s;
  mean[ch] = (float)mu;
  invstd[ch] = is;
  if (moving_mean) {
    const double unbiased = var * ((double)M / (double)(M > 1 ? M - 1 : 1));
    moving_mean[ch] = moving_mean[ch] * momentum + (float)mu * (1.f - momentum);
    moving_var[ch] = moving_var[ch] * momentum + (float)unbiased * (1.f - momentum);
  }
}

__global__ __launch_bounds__(16 * FL) void bn_finalize_kernel(const float* __restrict__ partial, int blocks, int M, int C,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, float momentum,
                                                          float* moving_mean, float* moving_var, float* mean,
                                                          float* invstd, float* scale, float* shift) {
  __shared__ double red[2][FL][16];
  const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const int ch = blockIdx.x * 16 + cx;
  double s0, s1;
  sum_partials(partial, blocks, C, ch, ry, s0, s1);
  fl_stage(red, ry, cx, s0, s1);
  if (ry == 0 && ch < C) {
    double a, b;
    fl_sum2(red, cx, a, b);
    bn_fwd_channel(a, b, M, ch, gamma, beta, eps, momentum, moving_mean, moving_var, mean, invstd, scale[ch], shift[ch]);
  }
}

__global__ __launch_bounds__(16 * FL) void bn_bwd_finalize_kernel(const float* __restrict__ partial, int blocks, int M,
                                                              int C, const float* __restrict__ gamma,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, float* dgamma,
                                                              float* dbeta, float* coefA, float* coefB,
                                                              float* coefC, int raw) {
  __shared__ double red[2][FL][16];
  const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const int ch = blockIdx.x * 16 + cx;
  double s0, s1;
  sum_partials(partial, blocks, C, ch, ry, s0, s1);
  fl_stage(red, ry, cx, s0, s1);
  if (ry == 0 && ch < C) {
    double db, dg;
    fl_sum2(red, cx, db, dg);
    const double is = invstd[ch], mu = mean[ch];
    if (raw) dg = is * (dg - mu * db);      // partials of (sum dz, sum dz * y) from an input-gradient epilogue: -> sum dz * xhat
    dbeta[ch] = (float)db;
    dgamma[ch] = (float)dg;
    bn_bwd_coefs(gamma[ch], is, mu, db, dg, (double)M, coefA[ch], coefB[ch], coefC[ch]);
  }
}

__global__ void bn_infer_coeffs_kernel(int C, const float* gamma, const float* beta, const float* mm,
                                       const float* mv, float eps, float* scale, float* shift) {
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch < C) {
    const float is = 1.0f / sqrtf(mv[ch] + eps);
    const float sc = gamma[ch] * is;
    scale[ch] = sc;
    shift[ch] = beta[ch] - mm[ch] * sc;
  }
}

// ---- element-wise passes over the nvec = M * C / 8 vectors of [M, C] --------------------------------------------------
// One skeleton for the four apply kernels: a grid-stride loop that calls body(i, m, vc, k) for vector i = row m x vector
// column vc, with k[q] = the 8 floats of coefficient row coef[q] at that column.
// When the grid stride is a multiple of C/8 a thread keeps the same 8 channels on every trip: their coefficients
// are loaded once (they were 4 extra 16-byte loads per 16-byte data load, all L1 hits but all TA cycles).
template <int NCOEF, class Body>
__device__ __forceinline__ void for_each_vec(size_t nvec, int C, const FastDiv& fd_vcols, const float* const (&coef)[NCOEF],
                                             Body body) {
  const int vcols = C >> 3;
  const size_t stride = (size_t)gridDim.x * 256;
  const bool fixed = (stride % (size_t)vcols) == 0;
  float k[NCOEF][8];
  auto load_coef = [&](int vc) {
#pragma unroll
    for (int q = 0; q < NCOEF; ++q) {
      const f32x4 lo = *reinterpret_cast<const f32x4*>(coef[q] + vc * 8);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(coef[q] + vc * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        k[q][e] = lo[e];
        k[q][e + 4] = hi[e];
      }
    }
  };
  // Two loops, not one with the reload under a branch: there the compiler kept the loop-carried coefficients and the
  // freshly loaded ones in different register layouts (132 VGPRs for the 6 rows of bn_bwd_apply2_kernel against 83).
  const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (fixed) {
    load_coef((int)(i0 % (size_t)vcols));
    for (size_t i = i0; i < nvec; i += stride) {
      const unsigned m = fd_div((unsigned)i, fd_vcols);
      body(i, m, (int)((unsigned)i - m * (unsigned)vcols), k);
    }
  } else {
    for (size_t i = i0; i < nvec; i += stride) {
      const unsigned m = fd_div((unsigned)i, fd_vcols);
      const int vc = (int)((unsigned)i - m * (unsigned)vcols);
      load_coef(vc);
      body(i, m, vc, k);
    }
  }
}

// ---- apply: y = [relu](x*scale + shift [+ residual]) ---------------------------------------------
template <int RES, bool RELU>
__global__ __launch_bounds__(256) void bn_apply_kernel(size_t nvec, int C, FastDiv fd_vcols,
                                                       const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift,
                                                       const bf16_t* __restrict__ res, FastDiv fd_w, FastDiv fd_h,
                                                       int H, int W, uint8_t* __restrict__ mask) {
  const float* const coef[2] = {scale, shift};
  for_each_vec<2>(nvec, C, fd_vcols, coef, [&](size_t i, unsigned m, int vc, const float (&k)[2][8]) {
    float f[8];
    unpack8(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(x + i * 8)), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = f[e] * k[0][e] + k[1][e];
    if (RES != 0) {
      size_t ri;
      if (RES == 1) {
        ri = i * 8;
      } else {
        const unsigned nh = fd_div(m, fd_w);
        const unsigned w = m - nh * (unsigned)W;
        const unsigned n = fd_div(nh, fd_h);
        const unsigned h = nh - n * (unsigned)H;
        ri = ((((size_t)n * (H >> 1) + (h >> 1)) * (W >> 1) + (w >> 1)) * (C >> 3) + vc) * 8;
      }
      float r[8];
      unpack8(*reinterpret_cast<const u32x4*>(res + ri), r);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] += r[e];
    }
    if (RELU) {
      if (mask) mask[i] = (uint8_t)relu_mask8(f);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = fmaxf(f[e], 0.f);
    }
    BN_ST_FWD(pack8(f), reinterpret_cast<u32x4*>(y + i * 8));
  });
}

// ---- backward apply: dx = A*dz + B*x + C ; dz = dy * [yout > 0] -----------------------------------
// A * dz + B * x has two products and the compiler fuses ONE of them into the add; which one depended on the code around the
// expression (the rounded product was B * x in every kernel here until the loop moved into for_each_vec, A * dz after).
// Spelled out, so that dx keeps its bits whatever surrounds it: fma(A, dz, round(B * x)) + C.
__device__ __forceinline__ float bwd_dx(float A, float dz, float B, float x, float C) {
  return __builtin_fmaf(A, dz, B * x) + C;
}

template <int RELU, bool WRITE_DZ>  // RELU: 0 none, 1 mask from the bf16 forward output, 2 packed bitmask
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(size_t nvec, int C, FastDiv fd_vcols,
                                                           const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                           const bf16_t* __restrict__ yout, const float* __restrict__ cA,
                                                           const float* __restrict__ cB,
                                                           const float* __restrict__ cC, bf16_t* __restrict__ dx,
                                                           bf16_t* __restrict__ dz) {
  const float* const coef[3] = {cA, cB, cC};
  for_each_vec<3>(nvec, C, fd_vcols, coef, [&](size_t i, unsigned, int, const float (&k)[3][8]) {
    float g[8], fx[8];
    unpack8(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(dy + i * 8)), g);
    unpack8(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(x + i * 8)), fx);
    if (RELU == 1) {
      float fy[8];
      unpack8(*reinterpret_cast<const u32x4*>(yout + i * 8), fy);
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] = fy[e] > 0.f ? g[e] : 0.f;
    } else if (RELU == 2) {
      mask8(g, reinterpret_cast<const uint8_t*>(yout)[i]);
    }
    if (WRITE_DZ) *reinterpret_cast<u32x4*>(dz + i * 8) = pack8(g);
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = bwd_dx(k[0][e], g[e], k[1][e], fx[e], k[2][e]);
    BN_ST_BWD(pack8(o), reinterpret_cast<u32x4*>(dx + i * 8));
  });
}

// ---- backward apply of a BigLittle merge layer (packed mask, no dz) + the big branch's share in the same pass ---------
// The merge adds the nearest-upsampled big branch before its ReLU, so the big branch receives the 2 x 2 block sums of the
// masked gradient g = dy * [mask bit] -- the operands this pass reads anyway.  One thread owns a 2 x 2 pixel block of its 8
// channels: 4 x (dy, x, mask byte) in, 4 x dx and one block sum out; the separate block-sum pass (upsample_bwd_kernel<true>,
// pool.hip: dy and the mask once more) disappears.  The sum runs in that kernel's order (r, then s) and is rounded to bf16
// once, dx comes out of bwd_dx as above: both are the same bits.  for_each_vec walks the quads [N][Hs][Ws][C/8], so the
// coefficients stay once per thread; a wave's lanes are consecutive (quad column, vector column), i.e. each of its loads
// covers whole C-channel pixels (every second one of a row; the s = 0 / s = 1 loads of a trip interleave to the full row).
__global__ __launch_bounds__(256) void bn_bwd_apply_bsum_kernel(size_t nquad, int C, FastDiv fd_vcols,
                                                                const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                                const uint8_t* __restrict__ mask, const float* __restrict__ cA,
                                                                const float* __restrict__ cB, const float* __restrict__ cC,
                                                                bf16_t* __restrict__ dx, bf16_t* __restrict__ bsum,
                                                                FastDiv fd_ws, FastDiv fd_hs, int Hs, int Ws) {
  const float* const coef[3] = {cA, cB, cC};
  const unsigned vcols = (unsigned)(C >> 3);
  for_each_vec<3>(nquad, C, fd_vcols, coef, [&](size_t i, unsigned m, int vc, const float (&k)[3][8]) {
    const unsigned nh = fd_div(m, fd_ws);
    const unsigned j = m - nh * (unsigned)Ws;
    const unsigned n = fd_div(nh, fd_hs);
    const unsigned h = nh - n * (unsigned)Hs;
    const unsigned p00 = (n * 2u * (unsigned)Hs + 2u * h) * (2u * (unsigned)Ws) + 2u * j;   // < M, and M * vcols < 2^31
    size_t idx[4];
    u32x4 vg[4], vx[4];
    unsigned mk[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      idx[q] = (size_t)((p00 + (unsigned)(q >> 1) * 2u * (unsigned)Ws + (unsigned)(q & 1)) * vcols + (unsigned)vc);
      vg[q] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(dy + idx[q] * 8));
      vx[q] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(x + idx[q] * 8));
      mk[q] = mask[idx[q]];
    }
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float g[8], fx[8], o[8];
      unpack8(vg[q], g);
      unpack8(vx[q], fx);
      mask8(g, mk[q]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        acc[e] += g[e];
        o[e] = bwd_dx(k[0][e], g[e], k[1][e], fx[e], k[2][e]);
      }
      BN_ST_BWD(pack8(o), reinterpret_cast<u32x4*>(dx + idx[q] * 8));
    }
    *reinterpret_cast<u32x4*>(bsum + i * 8) = pack8(acc);
  });
}

// ---- two batch norms behind ONE ReLU: the block-final BN and the projection-shortcut BN of a bottleneck ---------------
// out = relu(bn_a(ya) + bn_b(yb)): both backward passes consume the same masked gradient g = dout * [out > 0].  Run as two
// independent BN backwards that is 2 x (reduce: dout, y, mask; apply: dout, y, mask -> dy) = 20.5 B per element; here dout
// and the mask are read once per pass for both: 16.25 B per element and two launches fewer per projection block.
// Partials: pa = [blocks][2][C] (sum g, sum g * xhat_a), pb likewise for b (sum g repeated, so the finalize is unchanged).
struct BwdRow2 {
  const bf16_t* __restrict__ dy;
  const bf16_t* __restrict__ xa;
  const bf16_t* __restrict__ xb;
  const uint8_t* __restrict__ mask;
  const float* __restrict__ mean_a;
  const float* __restrict__ invstd_a;
  const float* __restrict__ mean_b;
  const float* __restrict__ invstd_b;
  float* __restrict__ pa;
  float* __restrict__ pb;
  int C;
  float ma[8], ia[8], mb[8], ib[8];
  struct Loaded { u32x4 vg, va, vb; unsigned mk; };
  __device__ __forceinline__ void setup(int vc) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      ma[e] = mean_a[vc * 8 + e];
      ia[e] = invstd_a[vc * 8 + e];
      mb[e] = mean_b[vc * 8 + e];
      ib[e] = invstd_b[vc * 8 + e];
    }
  }
  __device__ __forceinline__ void load(Loaded& ld, size_t off, size_t mi) const {
    ld.vg = BN_LD_RED(reinterpret_cast<const u32x4*>(dy + off));
    ld.va = BN_LD_RED(reinterpret_cast<const u32x4*>(xa + off));
    ld.vb = BN_LD_RED(reinterpret_cast<const u32x4*>(xb + off));
    ld.mk = mask[mi];
  }
  __device__ __forceinline__ void accum(const Loaded& ld, float (&acc)[3][8]) const {
    float g[8], fa[8], fb[8];
    unpack8(ld.vg, g);
    unpack8(ld.va, fa);
    unpack8(ld.vb, fb);
    mask8(g, ld.mk);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      acc[0][e] += g[e];
      acc[1][e] += g[e] * ((fa[e] - ma[e]) * ia[e]);
      acc[2][e] += g[e] * ((fb[e] - mb[e]) * ib[e]);
    }
  }
  __device__ __forceinline__ void store(int rblk, int which, int ch, float v) const {
    if (which == 0) {
      pa[((size_t)rblk * 2 + 0) * C + ch] = v;
      pb[((size_t)rblk * 2 + 0) * C + ch] = v;
    } else if (which == 1) {
      pa[((size_t)rblk * 2 + 1) * C + ch] = v;
    } else {
      pb[((size_t)rblk * 2 + 1) * C + ch] = v;
    }
  }
};

__global__ __launch_bounds__(256) void bn_bwd_reduce2_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ xa,
                                                             const bf16_t* __restrict__ xb, const uint8_t* __restrict__ mask,
                                                             int M, int C, const float* __restrict__ mean_a,
                                                             const float* __restrict__ invstd_a, const float* __restrict__ mean_b,
                                                             const float* __restrict__ invstd_b, RowTiling t,
                                                             float* __restrict__ pa, float* __restrict__ pb) {
  row_reduce<3>(BwdRow2{dy, xa, xb, mask, mean_a, invstd_a, mean_b, invstd_b, pa, pb, C}, M, C, t);
}

// dxa = A_a * g + B_a * xa + C_a ; dxb likewise ; g = dy * [mask bit].  co = [6][C]: A_a, B_a, C_a, A_b, B_b, C_b.
__global__ __launch_bounds__(256) void bn_bwd_apply2_kernel(size_t nvec, int C, FastDiv fd_vcols,
                                                            const bf16_t* __restrict__ dy, const bf16_t* __restrict__ xa,
                                                            const bf16_t* __restrict__ xb, const uint8_t* __restrict__ mask,
                                                            const float* __restrict__ co, bf16_t* __restrict__ dxa,
                                                            bf16_t* __restrict__ dxb) {
  const float* const coef[6] = {co, co + (size_t)C, co + (size_t)2 * C, co + (size_t)3 * C, co + (size_t)4 * C, co + (size_t)5 * C};
  for_each_vec<6>(nvec, C, fd_vcols, coef, [&](size_t i, unsigned, int, const float (&k)[6][8]) {
    float g[8], fa[8], fb[8];
    unpack8(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(dy + i * 8)), g);
    unpack8(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(xa + i * 8)), fa);
    unpack8(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(xb + i * 8)), fb);
    mask8(g, mask[i]);
    float oa[8], ob[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      oa[e] = bwd_dx(k[0][e], g[e], k[1][e], fa[e], k[2][e]);
      ob[e] = bwd_dx(k[3][e], g[e], k[4][e], fb[e], k[5][e]);
    }
    BN_ST_BWD(pack8(oa), reinterpret_cast<u32x4*>(dxa + i * 8));
    BN_ST_BWD(pack8(ob), reinterpret_cast<u32x4*>(dxb + i * 8));
  });
}

// ---- forward twin of the pair above: out = [relu](bn_a(xa) + bf16(bn_b(xb))) in one pass -----------------------------
// The projection-shortcut batch norm has no consumer but this add, so its normalised tensor need not exist in HBM: it is
// evaluated on the fly (and rounded to bf16 exactly where the separate pass stored it: results are bit-identical).
// Saves the 4 B / element the shortcut's own apply pass moved.
template <bool RELU>
__global__ __launch_bounds__(256) void bn_apply2_kernel(size_t nvec, int C, FastDiv fd_vcols, const bf16_t* __restrict__ xa,
                                                        const bf16_t* __restrict__ xb, bf16_t* __restrict__ y,
                                                        const float* __restrict__ sa, const float* __restrict__ ha,
                                                        const float* __restrict__ sb, const float* __restrict__ hb,
                                                        uint8_t* __restrict__ mask) {
  const float* const coef[4] = {sa, ha, sb, hb};
  for_each_vec<4>(nvec, C, fd_vcols, coef, [&](size_t i, unsigned, int, const float (&k)[4][8]) {
    float fa[8], fb[8];
    unpack8(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(xa + i * 8)), fa);
    unpack8(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(xb + i * 8)), fb);
#pragma unroll
    for (int e = 0; e < 8; ++e) fb[e] = fb[e] * k[2][e] + k[3][e];
    float rb[8];
    unpack8(pack8(fb), rb);                 // the bf16 rounding of the materialised shortcut tensor
#pragma unroll
    for (int e = 0; e < 8; ++e) fa[e] = fa[e] * k[0][e] + k[1][e] + rb[e];
    if (RELU) {
      if (mask) mask[i] = (uint8_t)relu_mask8(fa);
#pragma unroll
      for (int e = 0; e < 8; ++e) fa[e] = fmaxf(fa[e], 0.f);
    }
    BN_ST_FWD(pack8(fa), reinterpret_cast<u32x4*>(y + i * 8));
  });
}

// ---- small-tensor batch norm: statistics + finalize + apply in ONE launch (and reduce + finalize + apply backward) ----
// The SK / SE squeeze layers normalise [N, 1, 1, d] tensors (256 x 32..256 elements): three to four ~5 us launches
// of pure latency per direction in the general path.  Here one workgroup owns 64 channels x all M rows (M <= 4096):
// 256 threads = 8 vector columns x 32 row lanes, two passes over data that stays in L1 / L2.
constexpr int SMALL_BN_MAX_ROWS = 4096;

template <bool RELU>
__global__ __launch_bounds__(256) void bn_small_fwd_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, int M,
                                                           int C, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, float momentum,
                                                           float* moving_mean, float* moving_var, float* mean,
                                                           float* invstd, uint8_t* __restrict__ mask) {
  // [stat][channel][row lane], rows padded to 33 floats: a wave's 64 lanes (8 vector columns x 8 row lanes) write 32 banks
  // two-way (channel-major rows of 64 floats put them on 4 banks: every store was a 16-way conflict)
  __shared__ float red[2][64][33];
  __shared__ float coef[2][64];
  const int vcols = C >> 3;
  const int vcl = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int vc = blockIdx.x * 8 + vcl;
  const bool live = vc < vcols;
  float s[8], ss[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = ss[e] = 0.f;
  // M <= 256 rows (the workload: one row per image): a lane's 8 rows are loaded in ONE batch and stay in registers for the
  // apply pass.  (Round 4.  The plain loops below issue a load, wait, accumulate -- 8 + 8 dependent round trips to L2 for a
  // kernel that moves 64 KB: 9 us.)  Same accumulation order, same bits.
  constexpr int KU = 8;
  const bool keep = M <= 32 * KU;
  u32x4 kv[KU];
  if (live && keep) {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int r = rl + 32 * u;
      kv[u] = *reinterpret_cast<const u32x4*>(x + (size_t)(r < M ? r : 0) * C + vc * 8);   // (row 0 always exists)
    }
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      if (rl + 32 * u >= M) break;
      float f[8];
      unpack8(kv[u], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s[e] += f[e];
        ss[e] += f[e] * f[e];
      }
    }
  } else if (live)
    for (int r = rl; r < M; r += 32) {
      float f[8];
      unpack8(*reinterpret_cast<const u32x4*>(x + (size_t)r * C + vc * 8), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s[e] += f[e];
        ss[e] += f[e] * f[e];
      }
    }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[0][vcl * 8 + e][rl] = s[e];
    red[1][vcl * 8 + e][rl] = ss[e];
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch < C) {
      double a = 0.0, b = 0.0;
      for (int r = 0; r < 32; ++r) {
        a += (double)red[0][threadIdx.x][r];
        b += (double)red[1][threadIdx.x][r];
      }
      bn_fwd_channel(a, b, M, ch, gamma, beta, eps, momentum, moving_mean, moving_var, mean, invstd, coef[0][threadIdx.x],
                     coef[1][threadIdx.x]);
    }
  }
  __syncthreads();
  auto apply_row = [&](int r, const u32x4& vx) {
    const size_t i = (size_t)r * vcols + vc;
    float f[8];
    unpack8(vx, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = f[e] * coef[0][vcl * 8 + e] + coef[1][vcl * 8 + e];
    if (RELU) {
      if (mask) mask[i] = (uint8_t)relu_mask8(f);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = fmaxf(f[e], 0.f);
    }
    *reinterpret_cast<u32x4*>(y + i * 8) = pack8(f);
  };
  if (live && keep) {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      if (rl + 32 * u >= M) break;
      apply_row(rl + 32 * u, kv[u]);
    }
  } else if (live) {
    for (int r = rl; r < M; r += 32) apply_row(r, *reinterpret_cast<const u32x4*>(x + ((size_t)r * vcols + vc) * 8));
  }
}

template <int RELU>   // 0 none, 2 packed bitmask
__global__ __launch_bounds__(256) void bn_small_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                           const uint8_t* __restrict__ mask, int M, int C,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, float* dgamma,
                                                           float* dbeta, bf16_t* __restrict__ dx) {
  __shared__ float red[2][64][33];   // [stat][channel][row lane] (see bn_small_fwd_kernel)
  __shared__ float coef[3][64];
  const int vcols = C >> 3;
  const int vcl = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int vc = blockIdx.x * 8 + vcl;
  const bool live = vc < vcols;
  float s[8], ss[8], mu[8], is[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    s[e] = ss[e] = 0.f;
    mu[e] = live ? mean[vc * 8 + e] : 0.f;
    is[e] = live ? invstd[vc * 8 + e] : 0.f;
  }
  // as in bn_small_fwd_kernel: M <= 256 -> one batch of loads, rows kept in registers for the apply pass
  constexpr int KU = 8;
  const bool keep = M <= 32 * KU;
  u32x4 kg[KU], kx[KU];
  unsigned km[KU];
  auto masked = [&](const u32x4& vg, unsigned mk, float* g) {
    unpack8(vg, g);
    if (RELU == 2) mask8(g, mk);
  };
  auto reduce_row = [&](const u32x4& vg, const u32x4& vx, unsigned mk) {
    float g[8], fx[8];
    masked(vg, mk, g);
    unpack8(vx, fx);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s[e] += g[e];
      ss[e] += g[e] * ((fx[e] - mu[e]) * is[e]);
    }
  };
  if (live && keep) {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int r = rl + 32 * u;
      const size_t i = (size_t)(r < M ? r : 0) * vcols + vc;
      kg[u] = *reinterpret_cast<const u32x4*>(dy + i * 8);
      kx[u] = *reinterpret_cast<const u32x4*>(x + i * 8);
      km[u] = RELU == 2 ? mask[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      if (rl + 32 * u >= M) break;
      reduce_row(kg[u], kx[u], km[u]);
    }
  } else if (live) {
    for (int r = rl; r < M; r += 32) {
      const size_t i = (size_t)r * vcols + vc;
      reduce_row(*reinterpret_cast<const u32x4*>(dy + i * 8), *reinterpret_cast<const u32x4*>(x + i * 8),
                 RELU == 2 ? mask[i] : 0u);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[0][vcl * 8 + e][rl] = s[e];
    red[1][vcl * 8 + e][rl] = ss[e];
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch < C) {
      double db = 0.0, dg = 0.0;
      for (int r = 0; r < 32; ++r) {
        db += (double)red[0][threadIdx.x][r];
        dg += (double)red[1][threadIdx.x][r];
      }
      dbeta[ch] = (float)db;
      dgamma[ch] = (float)dg;
      bn_bwd_coefs(gamma[ch], invstd[ch], mean[ch], db, dg, (double)M, coef[0][threadIdx.x], coef[1][threadIdx.x],
                   coef[2][threadIdx.x]);
    }
  }
  __syncthreads();
  auto apply_row = [&](int r, const u32x4& vg, const u32x4& vx, unsigned mk) {
    float g[8], fx[8], o[8];
    masked(vg, mk, g);
    unpack8(vx, fx);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = coef[0][vcl * 8 + e] * g[e] + coef[1][vcl * 8 + e] * fx[e] + coef[2][vcl * 8 + e];
    *reinterpret_cast<u32x4*>(dx + ((size_t)r * vcols + vc) * 8) = pack8(o);
  };
  if (live && keep) {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      if (rl + 32 * u >= M) break;
      apply_row(rl + 32 * u, kg[u], kx[u], km[u]);
    }
  } else if (live) {
    for (int r = rl; r < M; r += 32) {
      const size_t i = (size_t)r * vcols + vc;
      apply_row(r, *reinterpret_cast<const u32x4*>(dy + i * 8), *reinterpret_cast<const u32x4*>(x + i * 8),
                RELU == 2 ? mask[i] : 0u);
    }
  }
}

// the for_each_vec kernels' own cap, half of common.h's ew_grid
inline unsigned bn_vec_grid(size_t nvec) {
  size_t b = cdivz(nvec, 256);
  return (unsigned)(b < 4096 ? (b ? b : 1) : 4096);
}

// launch a for_each_vec kernel -- parameters (nvec, C, fastdiv(C / 8), rest...) -- over the M * C / 8 vectors of [M, C]
template <class... P, class... A>
void launch_vecs(void (*kernel)(size_t, int, FastDiv, P...), void* stream, int M, int C, A... rest) {
  const size_t nvec = (size_t)M * (C / 8);
  ASM_LAUNCH(kernel, dim3(bn_vec_grid(nvec)), dim3(256), 0, (hipStream_t)stream, nvec, C, make_fastdiv((unsigned)(C / 8)), rest...);
}

}  // namespace

extern "C" int asm_bn_stats_blocks(int M, int C) {
  if (M <= 0 || C <= 0 || C % 8) return ASM_EINVAL;
  return make_tiling(M, C).blocks;
}

extern "C" int asm_bn_stats(const void* x, int M, int C, float* stats_partial, void* stream) {
  ASM_REQUIRE(x && stats_partial && M > 0 && C > 0 && C % 8 == 0, "bn_stats: bad arguments (M=%d C=%d)", M, C);
  RowTiling t = make_tiling(M, C);
  ASM_LAUNCH(bn_stats_kernel, dim3(t.blocks * t.slices), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, M, C, t,
             stats_partial);
  ASM_CHECK_LAUNCH("bn_stats");
  return ASM_OK;
}

extern "C" int asm_bn_partials_compact(const float* partial, int blocks, int C, float* out, int groups,
                                       void* stream) {
  ASM_REQUIRE(partial && out && blocks > 0 && C > 0 && groups > 0 && groups <= blocks, "bn_partials_compact: bad arguments");
  const int per_group = cdiv(blocks, groups);
  ASM_REQUIRE(cdiv(blocks, per_group) == groups, "bn_partials_compact: groups=%d does not tile blocks=%d", groups, blocks);
  ASM_LAUNCH(partials_compact_kernel, dim3(cdiv(C, 16), groups), dim3(16 * FL), 0, (hipStream_t)stream, partial,
                     blocks, C, out, per_group);
  ASM_CHECK_LAUNCH("bn_partials_compact");
  return ASM_OK;
}

extern "C" int asm_bn_finalize(const float* stats_partial, int blocks, int M, int C, const float* gamma,
                               const float* beta, float eps, float momentum, float* moving_mean,
                               float* moving_var, float* mean, float* invstd, float* scale, float* shift,
                               void* stream) {
  ASM_REQUIRE(stats_partial && gamma && beta && mean && invstd && scale && shift && blocks > 0 && M > 0 && C > 0,
              "bn_finalize: bad arguments");
  ASM_REQUIRE((moving_mean == nullptr) == (moving_var == nullptr), "bn_finalize: moving stats must both be given");
  ASM_LAUNCH(bn_finalize_kernel, dim3(cdiv(C, 16)), dim3(16 * FL), 0, (hipStream_t)stream, stats_partial,
                     blocks, M, C, gamma, beta, eps, momentum, moving_mean, moving_var, mean, invstd, scale, shift);
  ASM_CHECK_LAUNCH("bn_finalize");
  return ASM_OK;
}

extern "C" int asm_bn_infer_coeffs(int C, const float* gamma, const float* beta, const float* moving_mean,
                                   const float* moving_var, float eps, float* scale, float* shift, void* stream) {
  ASM_REQUIRE(C > 0 && gamma && beta && moving_mean && moving_var && scale && shift, "bn_infer_coeffs: bad arguments");
  ASM_LAUNCH(bn_infer_coeffs_kernel, dim3(cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, C, gamma, beta,
                     moving_mean, moving_var, eps, scale, shift);
  ASM_CHECK_LAUNCH("bn_infer_coeffs");
  return ASM_OK;
}

extern "C" int asm_bn_apply(const void* x, void* y, int M, int C, const float* scale, const float* shift,
                            const void* residual, int res_mode, int relu, int H, int W, uint8_t* relu_mask_out,
                            void* stream) {
  ASM_REQUIRE(x && y && scale && shift && M > 0 && C > 0 && C % 8 == 0, "bn_apply: bad arguments");
  ASM_REQUIRE(res_mode >= 0 && res_mode <= 2 && (res_mode == 0 || residual), "bn_apply: bad residual mode");
  ASM_REQUIRE((size_t)M * (C / 8) < 0x7fffffffull, "bn_apply: tensor too large");
  if (res_mode == 2)
    ASM_REQUIRE(H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && M % (H * W) == 0, "bn_apply: bad upsample geometry");
  const FastDiv fw = make_fastdiv((unsigned)(W > 0 ? W : 1)), fh = make_fastdiv((unsigned)(H > 0 ? H : 1));
  static constexpr decltype(&bn_apply_kernel<0, false>) kernels[3][2] = {
      {bn_apply_kernel<0, false>, bn_apply_kernel<0, true>},
      {bn_apply_kernel<1, false>, bn_apply_kernel<1, true>},
      {bn_apply_kernel<2, false>, bn_apply_kernel<2, true>}};   // [res_mode][relu]
  launch_vecs(kernels[res_mode][relu != 0], stream, M, C, (const bf16_t*)x, (bf16_t*)y, scale, shift, (const bf16_t*)residual,
              fw, fh, H, W, relu_mask_out);
  ASM_CHECK_LAUNCH("bn_apply");
  return ASM_OK;
}

extern "C" int asm_bn_bwd_reduce(const void* dy, const void* x, const void* yout, int relu, int M, int C,
                                 const float* mean, const float* invstd, float* partial, void* stream) {
  ASM_REQUIRE(dy && x && mean && invstd && partial && M > 0 && C > 0 && C % 8 == 0, "bn_bwd_reduce: bad arguments");
  ASM_REQUIRE(relu >= 0 && relu <= 2 && (!relu || yout), "bn_bwd_reduce: relu mask needs the forward output / bitmask");
  RowTiling t = make_tiling(M, C);
  ASM_LAUNCH(bn_bwd_reduce_kernel, dim3(t.blocks * t.slices), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy,
                     (const bf16_t*)x, (const bf16_t*)yout, relu, M, C, mean, invstd, t, partial);
  ASM_CHECK_LAUNCH("bn_bwd_reduce");
  return ASM_OK;
}

extern "C" int asm_bn_bwd_finalize(const float* partial, int blocks, int M, int C, const float* gamma,
                                   const float* mean, const float* invstd, float* dgamma, float* dbeta,
                                   float* coefA, float* coefB, float* coefC, void* stream) {
  ASM_REQUIRE(partial && gamma && mean && invstd && dgamma && dbeta && coefA && coefB && coefC && blocks > 0,
              "bn_bwd_finalize: bad arguments");
  ASM_LAUNCH(bn_bwd_finalize_kernel, dim3(cdiv(C, 16)), dim3(16 * FL), 0, (hipStream_t)stream, partial, blocks,
                     M, C, gamma, mean, invstd, dgamma, dbeta, coefA, coefB, coefC, 0);
  ASM_CHECK_LAUNCH("bn_bwd_finalize");
  return ASM_OK;
}

extern "C" int asm_bn_bwd_finalize_raw(const float* partial, int blocks, int M, int C, const float* gamma,
                                       const float* mean, const float* invstd, float* dgamma, float* dbeta,
                                       float* coefA, float* coefB, float* coefC, void* stream) {
  ASM_REQUIRE(partial && gamma && mean && invstd && dgamma && dbeta && coefA && coefB && coefC && blocks > 0,
              "bn_bwd_finalize_raw: bad arguments");
  ASM_LAUNCH(bn_bwd_finalize_kernel, dim3(cdiv(C, 16)), dim3(16 * FL), 0, (hipStream_t)stream, partial, blocks,
                     M, C, gamma, mean, invstd, dgamma, dbeta, coefA, coefB, coefC, 1);
  ASM_CHECK_LAUNCH("bn_bwd_finalize_raw");
  return ASM_OK;
}

extern "C" int asm_bn_bwd_apply(const void* dy, const void* x, const void* yout, int relu, int M, int C,
                                const float* coefA, const float* coefB, const float* coefC, void* dx,
                                void* dz_out, void* stream) {
  ASM_REQUIRE(dy && x && dx && coefA && coefB && coefC && M > 0 && C > 0 && C % 8 == 0, "bn_bwd_apply: bad arguments");
  ASM_REQUIRE(relu >= 0 && relu <= 2 && (!relu || yout), "bn_bwd_apply: relu mask needs the forward output / bitmask");
  ASM_REQUIRE((size_t)M * (C / 8) < 0x7fffffffull, "bn_bwd_apply: tensor too large");
  static constexpr decltype(&bn_bwd_apply_kernel<0, false>) kernels[3][2] = {
      {bn_bwd_apply_kernel<0, false>, bn_bwd_apply_kernel<0, true>},
      {bn_bwd_apply_kernel<1, false>, bn_bwd_apply_kernel<1, true>},
      {bn_bwd_apply_kernel<2, false>, bn_bwd_apply_kernel<2, true>}};   // [relu kind][writes dz]
  launch_vecs(kernels[relu][dz_out != nullptr], stream, M, C, (const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)yout, coefA,
              coefB, coefC, (bf16_t*)dx, (bf16_t*)dz_out);
  ASM_CHECK_LAUNCH("bn_bwd_apply");
  return ASM_OK;
}

extern "C" int asm_bn_bwd_apply_blocksum(const void* dy, const void* x, const uint8_t* relu_mask, int N, int H, int W, int C,
                                         const float* coefA, const float* coefB, const float* coefC, void* dx,
                                         void* block_sum, void* stream) {
  ASM_REQUIRE(dy && x && relu_mask && dx && block_sum && coefA && coefB && coefC, "bn_bwd_apply_blocksum: null pointer");
  ASM_REQUIRE(N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && C > 0 && C % 8 == 0,
              "bn_bwd_apply_blocksum: bad shape (N=%d H=%d W=%d C=%d; H and W must be even)", N, H, W, C);
  ASM_REQUIRE((size_t)N * H * W * (C / 8) < 0x7fffffffull, "bn_bwd_apply_blocksum: tensor too large");
  const int Hs = H / 2, Ws = W / 2;
  launch_vecs(bn_bwd_apply_bsum_kernel, stream, N * Hs * Ws, C, (const bf16_t*)dy, (const bf16_t*)x, relu_mask, coefA, coefB,
              coefC, (bf16_t*)dx, (bf16_t*)block_sum, make_fastdiv((unsigned)Ws), make_fastdiv((unsigned)Hs), Hs, Ws);
  ASM_CHECK_LAUNCH("bn_bwd_apply_blocksum");
  return ASM_OK;
}

extern "C" int asm_bn_small_max_rows(void) { return SMALL_BN_MAX_ROWS; }

extern "C" int asm_bn_small_fwd(const void* x, void* y, int M, int C, const float* gamma, const float* beta, float eps,
                                float momentum, float* moving_mean, float* moving_var, float* mean, float* invstd,
                                int relu, uint8_t* relu_mask_out, void* stream) {
  ASM_REQUIRE(x && y && gamma && beta && mean && invstd && M > 0 && M <= SMALL_BN_MAX_ROWS && C > 0 && C % 8 == 0,
              "bn_small_fwd: bad arguments (M=%d C=%d)", M, C);
  ASM_REQUIRE((moving_mean == nullptr) == (moving_var == nullptr), "bn_small_fwd: moving stats must both be given");
  const dim3 grid(cdiv(C, 64)), block(256);
  if (relu)
    ASM_LAUNCH(bn_small_fwd_kernel<true>, grid, block, 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)y, M, C,
                       gamma, beta, eps, momentum, moving_mean, moving_var, mean, invstd, relu_mask_out);
  else
    ASM_LAUNCH(bn_small_fwd_kernel<false>, grid, block, 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)y, M, C,
                       gamma, beta, eps, momentum, moving_mean, moving_var, mean, invstd, nullptr);
  ASM_CHECK_LAUNCH("bn_small_fwd");
  return ASM_OK;
}

extern "C" int asm_bn_small_bwd(const void* dy, const void* x, const uint8_t* relu_mask, int M, int C,
                                const float* gamma, const float* mean, const float* invstd, float* dgamma,
                                float* dbeta, void* dx, void* stream) {
  ASM_REQUIRE(dy && x && gamma && mean && invstd && dgamma && dbeta && dx && M > 0 && M <= SMALL_BN_MAX_ROWS && C > 0 &&
                  C % 8 == 0, "bn_small_bwd: bad arguments (M=%d C=%d)", M, C);
  const dim3 grid(cdiv(C, 64)), block(256);
  if (relu_mask)
    ASM_LAUNCH(bn_small_bwd_kernel<2>, grid, block, 0, (hipStream_t)stream, (const bf16_t*)dy, (const bf16_t*)x,
                       relu_mask, M, C, gamma, mean, invstd, dgamma, dbeta, (bf16_t*)dx);
  else
    ASM_LAUNCH(bn_small_bwd_kernel<0>, grid, block, 0, (hipStream_t)stream, (const bf16_t*)dy, (const bf16_t*)x,
                       nullptr, M, C, gamma, mean, invstd, dgamma, dbeta, (bf16_t*)dx);
  ASM_CHECK_LAUNCH("bn_small_bwd");
  return ASM_OK;
}

extern "C" int asm_bn_bwd_reduce2(const void* dy, const void* xa, const void* xb, const uint8_t* relu_mask, int M, int C,
                                  const float* mean_a, const float* invstd_a, const float* mean_b, const float* invstd_b,
                                  float* partial_a, float* partial_b, void* stream) {
  ASM_REQUIRE(dy && xa && xb && relu_mask && mean_a && invstd_a && mean_b && invstd_b && partial_a && partial_b && M > 0 &&
                  C > 0 && C % 8 == 0, "bn_bwd_reduce2: bad arguments");
  RowTiling t = make_tiling(M, C);
  ASM_LAUNCH(bn_bwd_reduce2_kernel, dim3(t.blocks * t.slices), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy,
                     (const bf16_t*)xa, (const bf16_t*)xb, relu_mask, M, C, mean_a, invstd_a, mean_b, invstd_b, t, partial_a,
                     partial_b);
  ASM_CHECK_LAUNCH("bn_bwd_reduce2");
  return ASM_OK;
}

extern "C" int asm_bn_bwd_apply2(const void* dy, const void* xa, const void* xb, const uint8_t* relu_mask, int M, int C,
                                 const float* coef6, void* dxa, void* dxb, void* stream) {
  ASM_REQUIRE(dy && xa && xb && relu_mask && coef6 && dxa && dxb && M > 0 && C > 0 && C % 8 == 0, "bn_bwd_apply2: bad arguments");
  ASM_REQUIRE((size_t)M * (C / 8) < 0x7fffffffull, "bn_bwd_apply2: tensor too large");
  launch_vecs(bn_bwd_apply2_kernel, stream, M, C, (const bf16_t*)dy, (const bf16_t*)xa, (const bf16_t*)xb, relu_mask, coef6,
              (bf16_t*)dxa, (bf16_t*)dxb);
  ASM_CHECK_LAUNCH("bn_bwd_apply2");
  return ASM_OK;
}

extern "C" int asm_bn_apply2(const void* xa, const void* xb, void* y, int M, int C, const float* scale_a,
                             const float* shift_a, const float* scale_b, const float* shift_b, int relu,
                             uint8_t* relu_mask_out, void* stream) {
  ASM_REQUIRE(xa && xb && y && scale_a && shift_a && scale_b && shift_b && M > 0 && C > 0 && C % 8 == 0, "bn_apply2: bad arguments");
  ASM_REQUIRE((size_t)M * (C / 8) < 0x7fffffffull, "bn_apply2: tensor too large");
  launch_vecs(relu ? bn_apply2_kernel<true> : bn_apply2_kernel<false>, stream, M, C, (const bf16_t*)xa, (const bf16_t*)xb,
              (bf16_t*)y, scale_a, shift_a, scale_b, shift_b, relu ? relu_mask_out : nullptr);
  ASM_CHECK_LAUNCH("bn_apply2");
  return ASM_OK;
}
