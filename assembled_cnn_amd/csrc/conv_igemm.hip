// MFMA implicit-GEMM convolution for gfx950: fprop and dgrad share one gather-GEMM kernel.
//
//   Y[m][n] = sum_{tap t=(r,s)} sum_c  X[gather(m, t)][c] * Wt[n][t][c]
//
//   fprop: m = (img, ho, wo), X = activations NHWC, Wt = filter KRSC, n = output channel
//   dgrad: m = (img, h, w) of dx, X = dy NHWC, Wt = filter CRSK, n = input channel
//
// Block tile 128(M) x BN(N) x BK(K), 256 threads = 4 waves (2 x 2), v_mfma_f32_32x32x16_bf16.
// The MFMA "A" operand is the FILTER tile and the "B" operand the ACTIVATION tile, so an
// accumulator register quad holds 4 consecutive output channels of one pixel: the epilogue packs
// them to bf16 and stages the tile through LDS for 16-byte, fully coalesced NHWC stores.  The
// same pass accumulates per-channel sum / sum-of-squares of the bf16-ROUNDED outputs (the first
// half of the following batch-norm), written as deterministic per-M-block partials (no atomics).
//
// igemm_kernel below is the GENERAL form (any filter size, stride, channel count that is a multiple of 8): global -> LDS by
// LDS-DMA (global_load_lds_dwordx4), an out-of-image tap or a channel tail reads 16 zero bytes instead.  LDS rows are
// XOR-swizzled at 16-byte granularity so the ds_read_b128 fragment reads are bank-conflict free.  The workloads' own layers
// run on the specialised kernels further down (igemm2 / igemm3 / igemm8 / conv_halo, conv_gemm1.hip); plan_conv at the end of
// this file chooses the kernel of a layer.
#include "common.h"
#include "igemm_common.h"

using namespace asm_igemm;

// conv_gemm1.hip: the 1x1 layers as a GEMM with a ring of LDS stages (configuration code, 0: the layer is not one it takes)
int asm_gemm1_config(const IGemmArgs& a, bool out_f32, bool stats, ConvTile* t);
int asm_gemm1_launch(const ConvLaunch& L, const IGemmArgs& a, hipStream_t st);
// conv_igemm8.hip: the wide 3x3 stride-1 layers on the wave-staggered multi-phase main loop
bool asm_igemm8_covers(const IGemmArgs& a, bool out_f32);
int asm_igemm8_launch(const ConvLaunch& L, const IGemmArgs& a, hipStream_t st);

namespace {

// 16 zero bytes: the source of every masked lane of an LDS-DMA load (global_load_lds has no bounds check)
__device__ __attribute__((aligned(16))) unsigned g_zero16[4] = {0u, 0u, 0u, 0u};


template <int BM, int BN, int BK, int WGM, int WGN, bool OUT_F32, bool STATS, bool BNRED = false>
__global__ __launch_bounds__(64 * WGM * WGN) void igemm_kernel(IGemmArgs p) {
  using C = Cfg<BM, BN, BK, WGM, WGN, OUT_F32, STATS>;
  constexpr int NT = C::NT, CPR = C::CPR, RPP = C::RPP, XP = C::XP, WP = C::WP, ROWB = C::ROWB, STAGE = C::STAGE;
  constexpr int TM = C::TM, TN = C::TN, WTM = C::WTM, WTN = C::WTN;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;

  // XCD-aware bijective remap: each XCD (bid % 8) gets a contiguous range of logical tiles, and
  // the N-tiles of one M-tile are adjacent, so the activation tile is re-read from that XCD's L2.
  const int logical = xcd_contiguous(blockIdx.x, p.n_blocks);
  const int tile_m = logical / p.n_tiles_n;
  const int tile_n = logical - tile_m * p.n_tiles_n;

  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, p.w_bytes);

  const int chunk = tid % CPR;
  const int r0 = tid / CPR;

  // per-thread activation rows
  int xb[XP], bh[XP], bw[XP];
#pragma unroll
  for (int j = 0; j < XP; ++j) {
    const int m = tile_m * BM + r0 + j * RPP;
    if (m < p.M) {
      const int img = m / p.HoWo;
      const int rem = m - img * p.HoWo;
      const int ho = rem / p.Wo;
      const int wo = rem - ho * p.Wo;
      xb[j] = img * p.x_img_pitch;
      bh[j] = ho * p.so - p.pad;
      bw[j] = wo * p.so - p.pad;
    } else {
      xb[j] = 0;
      bh[j] = -(1 << 24);
      bw[j] = -(1 << 24);
    }
  }
  int wb[WP];
  bool wrow_ok[WP];
#pragma unroll
  for (int j = 0; j < WP; ++j) {
    const int row = r0 + j * RPP;
    const int n = tile_n * BN + row;
    wrow_ok[j] = row < BN;
    wb[j] = (wrow_ok[j] && n < p.Co) ? n * p.w_row_pitch : -1;
  }

  int kt_r = 0, kt_s = 0, kt_c = 0;  // tap / channel-chunk cursor of the NEXT tile to load (taps innermost, chunk outermost)
  // LDS-DMA staging: the thread -> (row, chunk) map above is already lane-linear per wave and pass (a wave
  // covers 64/CPR whole rows = 1 KiB), which is what global_load_lds requires of its destination; the XOR
  // swizzle therefore moves to the SOURCE side: the lane sitting at LDS chunk position `chunk` of row r fetches
  // global chunk (chunk ^ swz(r)).  Masked lanes read 16 zero bytes.
  auto issue_tile = [&](int stage, bool live) {
    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    unsigned char* xs = smem + stage * STAGE;
    unsigned char* ws = xs + BM * ROWB;
    const int th = p.tsign * kt_r, tw = p.tsign * kt_s;
    const int wrow0 = (tid >> 6) * (64 / CPR);
#pragma unroll
    for (int j = 0; j < XP; ++j) {
      const int row = r0 + j * RPP;
      const int c = kt_c * BK + ((chunk ^ swz<BK>(row)) << 3);
      int nh = bh[j] + th, nw = bw[j] + tw;
      bool ok = live && c < p.Ci;
      if (p.sd == 2) {
        ok = ok && (((nh | nw) & 1) == 0);
        nh >>= 1;
        nw >>= 1;
      }
      ok = ok && ((unsigned)nh < (unsigned)p.Hi) && ((unsigned)nw < (unsigned)p.Wi);
      const unsigned off = ((unsigned)xb[j] + (unsigned)nh * (unsigned)p.x_row_pitch +
                            (unsigned)nw * (unsigned)p.x_pix_pitch + (unsigned)c) * 2u;
      const unsigned char* src = ok ? reinterpret_cast<const unsigned char*>(p.x) + off
                                    : reinterpret_cast<const unsigned char*>(g_zero16);
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(xs + (j * RPP + wrow0) * ROWB), 16, 0, 0);
    }
    const int tap0 = (kt_r * p.S + kt_s) * p.Ci + kt_c * BK;
#pragma unroll
    for (int j = 0; j < WP; ++j) {
      const int row = r0 + j * RPP;
      if (j * RPP + wrow0 < BN) {  // wave-uniform: rows past the filter tile are never written
        const int c = ((chunk ^ swz<BK>(row)) << 3);
        const bool ok = live && (kt_c * BK + c < p.Ci) && (wb[j] >= 0);
        const unsigned off = (unsigned)(wb[j] + tap0 + c) * 2u;
        const unsigned char* src = ok ? reinterpret_cast<const unsigned char*>(p.w) + off
                                      : reinterpret_cast<const unsigned char*>(g_zero16);
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(ws + (j * RPP + wrow0) * ROWB), 16, 0, 0);
      }
    }
    if (++kt_s == p.S) {
      kt_s = 0;
      if (++kt_r == p.R) {
        kt_r = 0;
        ++kt_c;
      }
    }
  };

  f32x16 acc[TN][TM];
  zero_acc(acc);

  const int KT = p.R * p.S * p.kchunks;
  const int l31 = lane & 31, lhi = lane >> 5;

  auto compute = [&](int stage) {
    const unsigned char* xs = smem + stage * STAGE;
    const unsigned char* ws = xs + BM * ROWB;
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      const int ch = kk * 2 + lhi;
      bf16x8 fw[TN], fx[TM];
#pragma unroll
      for (int a = 0; a < TN; ++a) {
        const int row = wn * WTN + a * 32 + l31;
        fw[a] = *reinterpret_cast<const bf16x8*>(ws + row * ROWB + ((ch ^ swz<BK>(row)) << 4));
      }
#pragma unroll
      for (int b = 0; b < TM; ++b) {
        const int row = wm * WTM + b * 32 + l31;
        fx[b] = *reinterpret_cast<const bf16x8*>(xs + row * ROWB + ((ch ^ swz<BK>(row)) << 4));
      }
#pragma unroll
      for (int a = 0; a < TN; ++a)
#pragma unroll
        for (int b = 0; b < TM; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[a], fx[b], acc[a][b], 0, 0, 0);
    }
  };

  issue_tile(0, true);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
#pragma unroll 1
  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < KT) issue_tile(cur ^ 1, true);   // DMA of tile kt+1 runs under the MFMAs of tile kt
    compute(cur);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  igemm_epilogue<C, BM, BN, WTM, WTN, TM, TN, OUT_F32, STATS, false, false, false, BNRED>(p, acc, smem, tile_m, tile_n, tid, wm, wn, l31, lhi);
}

// ------------------------------------------------------------------------------------------------------------
// igemm2_kernel: the same tiling and epilogue with a main loop stripped of per-step address arithmetic.
// PMC on the register-staged kernel showed ~10 VALU + 5 SALU instructions per MFMA (tap decode, bounds checks,
// offset selects, exec-mask branches): the waves were issue-bound, not MFMA- or LDS-bound.  Here
//   * every (staging row, filter tap) byte offset -- zero padding, stride-2 parity, row/channel tails folded in as
//     the out-of-range offset -- is computed ONCE in the prologue into VGPRs (XP x R*S of them);
//   * the K loop runs channel chunks outermost and the R*S taps fully unrolled innermost, so a step's loads are
//     `buffer_load_dwordx4 ... lds` with a pre-computed voffset and the chunk advance in the scalar soffset:
//     no VALU, no branches, no VGPR round trip (LDS-DMA zero-fills out-of-range lanes -- tools/probes);
//   * m -> (img, ho, wo) uses multiply-shift division.
// Requires R x S in {1x1, 3x3, 7x1, 3x1} and (Ci % BK == 0 or a single chunk); the rest stays on igemm_kernel.
template <int BM, int BN, int BK, int WGM, int WGN, bool OUT_F32, bool STATS, int NS>
struct Cfg2 {
  using C = Cfg<BM, BN, BK, WGM, WGN, OUT_F32, STATS>;
  // NS = LDS stages.  A ring of 3-4 stages with counted vmcnt + raw s_barrier (DMA in flight across the barrier) was
  // measured at +-2 % over NS = 2 on every layer class, so only the double buffer is instantiated.
  static constexpr int WROWS = BN;
  static constexpr int STAGE = (BM + WROWS) * C::ROWB;
  static constexpr int LDS = cmax(cmax(NS * STAGE, C::EPI), C::RED);
  static_assert(LDS <= 160 * 1024, "lds");
};

// SCHED 1: the LDS-DMA pieces of step k+1 are issued IN BETWEEN the MFMA groups of step k instead of all at once right
// after the barrier (the 3x3 layers; the 1x1 layers issue them all at the head of the step).  Also tried (round 3, same box, conv_bench): pinning
// the fragment reads of group kk+1 at the head of group kk with sched_barrier(0) -- 2.62 vs 2.55 ms over the 12 heaviest
// shapes, slower than the compiler's own interleave, dropped.  Every wave comes out of the barrier at the same moment, and one piece
// costs its wave 60-180 issue cycles (v_readfirstlane + M0 write + the buffer_load itself): with 8 pieces up front both waves
// of a SIMD sit in their issue phase together and the matrix pipe idles for that long at the head of every step.
template <int BM, int BN, int BK, int WGM, int WGN, bool OUT_F32, bool STATS, int R, int S, int NS, bool PFA = false, bool POOL = false,
          int SCHED = 0, bool BNRED = false>
__global__ __launch_bounds__(64 * WGM * WGN) void igemm2_kernel(IGemmArgs p) {
  using C = Cfg<BM, BN, BK, WGM, WGN, OUT_F32, STATS>;
  using C2 = Cfg2<BM, BN, BK, WGM, WGN, OUT_F32, STATS, NS>;
  constexpr int CPR = C::CPR, RPP = C::RPP, XP = C::XP, WP = C::WP, ROWB = C::ROWB, STAGE = C2::STAGE;
  constexpr int TM = C::TM, TN = C::TN, WTM = C::WTM, WTN = C::WTN;
  constexpr int NTAP = R * S;
  static_assert(RPP % 16 == 0, "the source-side swizzle must not depend on the pass");
  typedef __attribute__((address_space(3))) void* lptr_t;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;

  const int logical = xcd_contiguous(blockIdx.x, p.n_blocks);
  const int tile_m0 = (int)fd_div((unsigned)logical, p.fd_ntn);
  const int tile_n = logical - tile_m0 * p.n_tiles_n;
  const int tile_m = tile_m0 + p.m_tile0;

  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, p.w_bytes);

  const int chunk = tid % CPR;
  const int r0 = tid / CPR;
  const int csw = (chunk ^ swz<BK>(r0)) << 3;   // channel (element) offset of the 16-byte piece this lane fetches
  const bool c_ok = csw < p.Ci;                  // only a single-chunk layer can have a channel tail

  // ---- prologue: per-(row, tap) byte offsets of the activation tile, per-row offsets of the filter tile ----
  unsigned vx[XP][NTAP];
#pragma unroll
  for (int j = 0; j < XP; ++j) {
    const int m = tile_m * BM + r0 + j * RPP;
    const bool live = c_ok && m < p.M;
    const Pixel px = decode_pixel((unsigned)m, p.fd_howo, p.HoWo, p.fd_wo, p.Wo);
    const int bh = (int)px.ho * p.so - p.pad, bw = (int)px.wo * p.so - p.pad_w;
    const unsigned base = px.img * (unsigned)p.x_img_pitch + (unsigned)csw;
    unsigned roff[R], coff[S];
    bool rok[R], cok[S];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int nh = bh + p.tsign * r;
      bool ok = live;
      if (p.sd == 2) {
        ok = ok && ((nh & 1) == 0);
        nh >>= 1;
      }
      rok[r] = ok && ((unsigned)nh < (unsigned)p.Hi);
      roff[r] = base + (unsigned)nh * (unsigned)p.x_row_pitch;
    }
#pragma unroll
    for (int q = 0; q < S; ++q) {
      int nw = bw + p.tsign * q;
      bool ok = true;
      if (p.sd == 2) {
        ok = ((nw & 1) == 0);
        nw >>= 1;
      }
      cok[q] = ok && ((unsigned)nw < (unsigned)p.Wi);
      coff[q] = (unsigned)nw * (unsigned)p.x_pix_pitch;
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = 0; q < S; ++q) vx[j][r * S + q] = (rok[r] && cok[q]) ? (roff[r] + coff[q]) * 2u : ASM_OOB;
  }
  unsigned vw[WP];
#pragma unroll
  for (int j = 0; j < WP; ++j) {
    const int row = r0 + j * RPP;
    const int n = tile_n * BN + row;
    vw[j] = (c_ok && row < BN && n < p.Co) ? ((unsigned)n * (unsigned)p.w_row_pitch + (unsigned)csw) * 2u : ASM_OOB;
  }

  const int wrow0 = wave * (64 / CPR);
  // pieces [lo, hi) of a step's XP + WP LDS-DMA pieces (activation rows first)
  auto issue_part = [&](int stage, const int t, unsigned xso, unsigned wso, const int lo, const int hi) {
    unsigned char* xs = smem + stage * STAGE;
    unsigned char* ws = xs + BM * ROWB;
#pragma unroll
    for (int j = 0; j < XP; ++j)
      if (j >= lo && j < hi)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lptr_t)(xs + (j * RPP + wrow0) * ROWB), 16,
                                                 (int)vx[j][t], (int)xso, 0, 0);
#pragma unroll
    for (int j = 0; j < WP; ++j)
      if (XP + j >= lo && XP + j < hi && j * RPP + wrow0 < BN)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(ws + (j * RPP + wrow0) * ROWB), 16,
                                                 (int)vw[j], (int)wso, 0, 0);
  };
  auto issue = [&](int stage, const int t, unsigned xso, unsigned wso) {
    unsigned char* xs = smem + stage * STAGE;
    unsigned char* ws = xs + BM * ROWB;
#pragma unroll
    for (int j = 0; j < XP; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lptr_t)(xs + (j * RPP + wrow0) * ROWB), 16,
                                               (int)vx[j][t], (int)xso, 0, 0);
#pragma unroll
    for (int j = 0; j < WP; ++j)
      if (j * RPP + wrow0 < BN)   // wave-uniform: rows past the filter tile are never written nor read
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(ws + (j * RPP + wrow0) * ROWB), 16,
                                                 (int)vw[j], (int)wso, 0, 0);
  };

  f32x16 acc[TN][TM];   // (written out: through zero_acc one instantiation comes out with other register counts)
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int b = 0; b < TM; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

  const int l31 = lane & 31, lhi = lane >> 5;
  // fragment byte offsets inside a stage (a = b = 0); +32 rows keeps the swizzle, so the other tiles are immediates
  unsigned fwo[BK / 16], fxo[BK / 16];
#pragma unroll
  for (int kk = 0; kk < BK / 16; ++kk) {
    const int ch = kk * 2 + lhi;
    const int rw_ = wn * WTN + l31, rx_ = wm * WTM + l31;
    fwo[kk] = BM * ROWB + rw_ * ROWB + ((ch ^ swz<BK>(rw_)) << 4);
    fxo[kk] = rx_ * ROWB + ((ch ^ swz<BK>(rx_)) << 4);
  }
  // Fragments are double-buffered in registers: the ds_reads of k-substep kk+1 are issued BEFORE the MFMAs of kk, and
  // the first fragments of the next stage right after the barrier that publishes it, before the last MFMA group of
  // the current step -- so LDS latency runs under MFMA execution instead of in front of it (the compiler emitted
  // read -> wait -> 4 MFMA per substep: ~45 % of every wave's loop time was spent waiting on lgkmcnt).
  constexpr int KK = BK / 16;
  bf16x8 fwb[2][TN], fxb[2][TM];
  auto load_frags = [&](int stage, const int kk, const int buf) {
    const unsigned char* sb = smem + stage * STAGE;
#pragma unroll
    for (int a = 0; a < TN; ++a) fwb[buf][a] = *reinterpret_cast<const bf16x8*>(sb + fwo[kk] + a * 32 * ROWB);
#pragma unroll
    for (int b = 0; b < TM; ++b) fxb[buf][b] = *reinterpret_cast<const bf16x8*>(sb + fxo[kk] + b * 32 * ROWB);
  };
  auto mma = [&](const int buf) {
#pragma unroll
    for (int a = 0; a < TN; ++a)
#pragma unroll
      for (int b = 0; b < TM; ++b)
        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fwb[buf][a], fxb[buf][b], acc[a][b], 0, 0, 0);
  };
  const unsigned tapw = (unsigned)p.Ci * 2u;   // bytes between consecutive taps of a filter row
  {
    // ---- DMA of step k+1 runs under the MFMAs of step k; one barrier per step ----
    issue(0, 0, 0u, (unsigned)p.wt0 * tapw);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    load_frags(0, 0, 0);
    int cur = 0;
    unsigned kcb = 0;                            // byte offset of the current channel chunk
#pragma unroll 1
    for (int kc = 0; kc < p.kchunks; ++kc) {
#pragma unroll
      for (int t = 0; t < NTAP; ++t) {
        const bool more = (t + 1 < NTAP) || (kc + 1 < p.kchunks);
        if constexpr (SCHED == 1 && KK >= 2) {
          constexpr int NP = XP + WP, G = KK - 1;            // pieces, MFMA groups in front of the barrier
          constexpr int PPG = (NP + G - 1) / G;
          const int tn = (t + 1 < NTAP) ? t + 1 : 0;         // compile-time after unrolling
          const unsigned xso = (t + 1 < NTAP) ? kcb : kcb + BK * 2;
          const unsigned wso = xso + (unsigned)(p.wt0 + (tn / S) * p.wtr + (tn % S) * p.wts) * tapw;
#pragma unroll
          for (int kk = 0; kk + 1 < KK; ++kk) {
            if (more) issue_part(cur ^ 1, tn, xso, wso, kk * PPG, (kk + 1) * PPG < NP ? (kk + 1) * PPG : NP);
            load_frags(cur, kk + 1, (kk + 1) & 1);
            mma(kk & 1);
          }
        } else {
        if (t + 1 < NTAP) {
          issue(cur ^ 1, t + 1, kcb, kcb + (unsigned)(p.wt0 + ((t + 1) / S) * p.wtr + ((t + 1) % S) * p.wts) * tapw);
        } else if (kc + 1 < p.kchunks) {
          issue(cur ^ 1, 0, kcb + BK * 2, kcb + BK * 2 + (unsigned)p.wt0 * tapw);
        }
#pragma unroll
        for (int kk = 0; kk + 1 < KK; ++kk) {
          load_frags(cur, kk + 1, (kk + 1) & 1);
          mma(kk & 1);
        }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                         // next tile visible; everyone's reads of this stage are in registers
        if (more) load_frags(cur ^ 1, 0, 0);
        mma((KK - 1) & 1);
        cur ^= 1;
      }
      kcb += BK * 2;
    }
  }

  igemm_epilogue<C, BM, BN, WTM, WTN, TM, TN, OUT_F32, STATS, PFA, POOL, false, BNRED>(p, acc, smem, tile_m, tile_n, tid, wm, wn, l31, lhi);
}

// ------------------------------------------------------------------------------------------------------------
// igemm3_kernel: 3x3 / stride 1 / pad 1 (fprop and its input gradient) with the ACTIVATION rows resident across the taps.
//
// Over the flattened pixel index m = (img, h, w) a 3x3 stride-1 convolution reads, for tap (r, s), the pixel
// m + (r - 1) * W + (s - 1): the nine taps are nine LINEAR row shifts of one [M][C] matrix, and what zero padding adds is
// a per-(pixel, tap) predicate (row / column of the tap outside the image), not a different address pattern.  igemm2
// stages a fresh 128-row activation tile for every tap (9 x 16 KB per 64-channel chunk, nearly all of it the same pixels
// again, through L2 -> LDS); here the 128 + 2 W + 2 rows the nine taps touch are LDS-DMA'd ONCE per 64-channel chunk
// (double-buffered over chunks: the next chunk's rows arrive one 32-row piece per tap under the current chunk's MFMAs),
// only the filter tile is streamed per tap, and a tap's activation fragment is a ds_read_b128 at a shifted row.  An
// out-of-image tap redirects the lane's fragment address to an all-zero row (one v_cndmask per tap and 32-row tile; the
// predicate bits are computed once per workgroup).  LDS-DMA traffic per chunk: 24 + 9 x 16 KB instead of 9 x 32 KB.
// Measured on the standalone probe (tools/probes/conv_probe.hip, MI355X, same box, plain epilogue): 14x14x512 -> 1024
// 464 -> 396 us, 14x14x256 -> 512 126 -> 115, 28x28x128 -> 256 138 -> 122, 7x7x256 -> 512 35.6 -> 32.7 us against the
// best gather-form tile of each layer; with the filter DMA as the only per-step traffic the loop runs within 4 % of its
// own MFMA + LDS-read time.  80 KB of LDS: two workgroups per CU, so one's epilogue runs under the other's main loop.
// Requires Ci % 64 == 0, at least two chunks (a single chunk has nothing to prefetch under), W <= 30, dense NHWC input.
// halo rows per buffer: 128 + 2 W + 2 <= H3_ROWS - 1 (rows past the live ones are zero-filled by the DMA: the last one is the
// all-zero row an out-of-image tap reads); 192 for W <= 30, 256 for the single-chunk form up to W = 62

// HR / NHB (round 5): halo rows per buffer and number of halo buffers.  A layer with ONE 64-channel chunk (Ci = 64: the SK
// convolutions of the 56 x 56 and 28 x 28 stages) has no next chunk to stage under the current one, so one buffer does, and
// with it 256 rows (W <= 62) fit 64 KB together with the two filter stages: two workgroups per CU like igemm2's tile, 178 +
// 9 x 128 instead of 9 x 256 staged rows per workgroup.
template <int BN, bool STATS, bool PFA, int H3_ROWS = 192, int NHB = 2, bool BNRED = false>
__global__ __launch_bounds__(256) void igemm3_kernel(IGemmArgs p) {
  constexpr int BM = 128, BK = 64, WGM = 2, WGN = 2;
  using C = Cfg<BM, BN, BK, WGM, WGN, false, STATS>;
  constexpr int RPP = C::RPP, ROWB = C::ROWB, WP = C::WP;
  constexpr int TM = C::TM, TN = C::TN, WTM = C::WTM, WTN = C::WTN;
  constexpr int HP = H3_ROWS / RPP;                 // halo pieces per wave and chunk
  constexpr int HALO = H3_ROWS * ROWB, WST = BN * ROWB;
  constexpr int KK = BK / 16, NTAP = 9;
  constexpr unsigned ZERO_ROW = (unsigned)(H3_ROWS - 1) * ROWB;
  static_assert(RPP == 32 && H3_ROWS % RPP == 0 && (NHB == 1 || HP <= NTAP - 1), "halo pieces are issued one per tap");
  typedef __attribute__((address_space(3))) void* lptr_t;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // halo[2] | filter ring[2]; reused by the epilogue
  unsigned char* const wring = smem + NHB * HALO;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  const int logical = xcd_contiguous(blockIdx.x, p.n_blocks);
  const int tile_m0 = (int)fd_div((unsigned)logical, p.fd_ntn);
  const int tile_n = logical - tile_m0 * p.n_tiles_n;
  const int tile_m = tile_m0 + p.m_tile0;

  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, p.w_bytes);
  const int chunk = tid & 7, r0 = tid >> 3;
  const int csw = (chunk ^ swz<BK>(r0)) << 3;      // the source-side swizzle (RPP % 16 == 0: the same for every pass)
  const int Wd = p.Wi;
  const int hrows = BM + 2 * Wd + 2;

  // ---- prologue: halo / filter source offsets, per-(pixel, tap) predicates ----
  unsigned vh[HP];
#pragma unroll
  for (int j = 0; j < HP; ++j) {
    const int hr = r0 + j * RPP;
    const int g = tile_m * BM - (Wd + 1) + hr;      // pixel of halo row hr
    vh[j] = (hr < hrows && g >= 0 && g < p.M) ? ((unsigned)g * (unsigned)p.Ci + (unsigned)csw) * 2u : ASM_OOB;
  }
  unsigned vw[WP];
#pragma unroll
  for (int j = 0; j < WP; ++j) {
    const int n = tile_n * BN + r0 + j * RPP;
    vw[j] = n < p.Co ? ((unsigned)n * (unsigned)p.w_row_pitch + (unsigned)csw) * 2u : ASM_OOB;
  }
  const int l31 = lane & 31, lhi = lane >> 5;
  // loop tap t = (r, s) reads the pixel (h + ts * (r - 1), w + ts * (s - 1)), ts = +1 (fprop) / -1 (input gradient)
  unsigned vmask[TM];
#pragma unroll
  for (int b = 0; b < TM; ++b) {
    const int m = tile_m * BM + wm * WTM + b * 32 + l31;
    const Pixel px = decode_pixel(m < p.M ? (unsigned)m : 0u, p.fd_howo, p.HoWo, p.fd_wo, p.Wo);
    const int h = (int)px.ho, w = (int)px.wo;
    unsigned mk = 0;
#pragma unroll
    for (int t = 0; t < NTAP; ++t) {
      const int dr = p.tsign * (t / 3 - 1), ds = p.tsign * (t % 3 - 1);
      const bool ok = m < p.M && (unsigned)(h + dr) < (unsigned)p.Hi && (unsigned)(w + ds) < (unsigned)p.Wi;
      mk |= (ok ? 1u : 0u) << t;
    }
    vmask[b] = mk;
  }
  const int wrow0 = wave * 8;
  const unsigned tapw = (unsigned)p.Ci * 2u;

  auto issue_halo = [&](int hb, unsigned xso, const int j) {
    unsigned char* hs = smem + hb * HALO;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lptr_t)(hs + (j * RPP + wrow0) * ROWB), 16, (int)vh[j], (int)xso, 0, 0);
  };
  auto issue_w = [&](int stage, unsigned wso, const int lo, const int hi) {
    unsigned char* ws = wring + stage * WST;
#pragma unroll
    for (int j = 0; j < WP; ++j)
      if (j >= lo && j < hi)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(ws + (j * RPP + wrow0) * ROWB), 16, (int)vw[j], (int)wso, 0, 0);
  };

  f32x16 acc[TN][TM];
  zero_acc(acc);

  unsigned fwo[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    const int rw_ = wn * WTN + l31;
    fwo[kk] = rw_ * ROWB + (((kk * 2 + lhi) ^ swz<BK>(rw_)) << 4);
  }
  const int xrow0 = wm * WTM + l31;     // halo row of this lane's first pixel at the shift (-1, -1)
  // byte offsets (inside a halo buffer) of this lane's activation fragments for loop tap t, k-substep 0; the swizzle is
  // keyed on the halo row (+32 rows keep it), an out-of-image tap reads the zero row
  unsigned xbv[TM];
  auto set_tap = [&](const int t) {
    const int dr = p.tsign * (t / 3 - 1), ds = p.tsign * (t % 3 - 1);
    const int row = xrow0 + (dr + 1) * Wd + (ds + 1);
    const unsigned xb = (unsigned)row * ROWB + ((unsigned)(lhi ^ swz<BK>(row)) << 4);
#pragma unroll
    for (int b = 0; b < TM; ++b) xbv[b] = ((vmask[b] >> t) & 1u) ? xb + (unsigned)(b * 32 * ROWB) : ZERO_ROW;
  };
  bf16x8 fwb[2][TN], fxb[2][TM];
  auto load_frags = [&](int hb, int stage, const int kk, const int buf) {
    const unsigned char* ws = wring + stage * WST;
    const unsigned char* hs = smem + hb * HALO;
#pragma unroll
    for (int a = 0; a < TN; ++a) fwb[buf][a] = *reinterpret_cast<const bf16x8*>(ws + fwo[kk] + a * 32 * ROWB);
#pragma unroll
    for (int b = 0; b < TM; ++b) fxb[buf][b] = *reinterpret_cast<const bf16x8*>(hs + (xbv[b] ^ (unsigned)(kk << 5)));
  };
  auto mma = [&](const int buf) {
#pragma unroll
    for (int a = 0; a < TN; ++a)
#pragma unroll
      for (int b = 0; b < TM; ++b)
        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fwb[buf][a], fxb[buf][b], acc[a][b], 0, 0, 0);
  };
  auto tap_off = [&](const int t) -> unsigned { return (unsigned)(p.wt0 + (t / 3) * p.wtr + (t % 3) * p.wts) * tapw; };

  {
    // ---- chunk 0's rows + the first filter tile; then one barrier per (chunk, tap) step.  A step opens with the barrier
    // that publishes its filter tile, issues the NEXT step's DMA at once (a whole step of MFMAs to land under: with only
    // 4 + 1 pieces per wave, spreading them over the step as igemm2 does leaves the last ones ~200 cycles before the wait)
    // and runs the previous step's last MFMA group under its own first fragment reads ----
#pragma unroll
    for (int j = 0; j < HP; ++j) issue_halo(0, 0u, j);
    issue_w(0, tap_off(0), 0, WP);
#pragma unroll
    for (int a = 0; a < TN; ++a) fwb[(KK - 1) & 1][a] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};   // the first "previous group" adds 0
#pragma unroll
    for (int b = 0; b < TM; ++b) fxb[(KK - 1) & 1][b] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    int cur = 0, hb = 0;
    unsigned kcb = 0;
#pragma unroll 1
    for (int kc = 0; kc < p.kchunks; ++kc) {
      const bool has_next = kc + 1 < p.kchunks;
#pragma unroll
      for (int t = 0; t < NTAP; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                         // this step's filter tile (at tap 0: this chunk's rows) visible; the
                                                 // stage / rows the DMA below overwrites have been read by every wave
        set_tap(t);
        load_frags(hb, cur, 0, 0);
        mma((KK - 1) & 1);
        const bool more = (t + 1 < NTAP) || has_next;
        const int tn = (t + 1 < NTAP) ? t + 1 : 0;           // compile time after unrolling
        if constexpr (NHB == 2) {
          if (has_next && t < HP) issue_halo(hb ^ 1, kcb + BK * 2, t);
        }
        if (more) issue_w(cur ^ 1, (t + 1 < NTAP ? kcb : kcb + BK * 2) + tap_off(tn), 0, WP);
#pragma unroll
        for (int kk = 0; kk + 1 < KK; ++kk) {
          load_frags(hb, cur, kk + 1, (kk + 1) & 1);
          mma(kk & 1);
        }
        cur ^= 1;
      }
      kcb += BK * 2;
      if constexpr (NHB == 2) hb ^= 1;
    }
    mma((KK - 1) & 1);
  }
  __syncthreads();   // every wave's fragment reads are done: the epilogue reuses the region
  igemm_epilogue<C, BM, BN, WTM, WTN, TM, TN, false, STATS, PFA, false, false, BNRED, 8>(p, acc, smem, tile_m, tile_n, tid, wm, wn, l31, lhi);
}

template <int BN, bool STATS, bool PFA, int HR = 192, int NHB = 2, bool BNRED = false>
int launch3_one(const IGemmArgs& a, hipStream_t st) {
  using C = Cfg<128, BN, 64, 2, 2, false, STATS>;
  constexpr int LDS = cmax(cmax(NHB * HR * 128 + 2 * BN * 128, C::EPI), C::RED);
  static_assert(LDS <= 80 * 1024, "two workgroups per CU");
  return asm_launch_dyn_lds<igemm3_kernel<BN, STATS, PFA, HR, NHB, BNRED>>("igemm3_kernel", dim3(a.n_blocks), dim3(256), LDS, st, a);
}

template <int HR, int NHB>
int launch3(const ConvLaunch& L, const IGemmArgs& a, hipStream_t st) {
  switch (L.epi) {
    case EPI_BNRED: return launch3_one<128, true, false, HR, NHB, true>(a, st);
    case EPI_STATS: return launch3_one<128, true, false, HR, NHB>(a, st);
    case EPI_PFA: return launch3_one<128, false, true, HR, NHB>(a, st);
    case EPI_PLAIN: return launch3_one<128, false, false, HR, NHB>(a, st);
  }
  return conv_no_variant("igemm3_kernel", L.epi);
}

// is the layer one igemm3_kernel covers?
bool igemm3_covers(const IGemmArgs& a, bool out_f32) {
  if (out_f32 || a.R != 3 || a.S != 3 || a.so != 1 || a.sd != 1 || a.y_strided || a.pool_dy) return false;
  if (!pad1_window(a) || !whole_3x3_filter(a)) return false;
  const bool one_chunk = a.Ci == 64;      // asm_tuning.igemm3 >= 2: also the single-chunk layers (one halo buffer)
  if (one_chunk && asm_tune().igemm3 == 1) return false;
  if (a.Ci % 64 || a.Co <= 64 || a.Wi > ((one_chunk ? 256 : 192) - 1 - 128 - 2) / 2) return false;
  if (a.HoWo != a.Hi * a.Wi || a.Wo != a.Wi || a.M % a.HoWo) return false;
  return packed_input(a);
}

// ------------------------------------------------------------------------------------------------------------
// conv_halo_kernel: stride-1 3x3 convolution (and its input gradient) for the NARROW high-resolution layers
// (Ci in {32, 64}, 112 x 112 maps: the BigLittle module-0 / ResNet-D stem convolutions).
// The gather-GEMM stages one activation tile PER TAP, so the 9 taps of a 3x3 read (almost) the same pixels 9 times
// through L2 -> LDS: these layers need ~0.6 GB of HBM traffic but ~5 GB of L2 -> LDS traffic and ran at 2.0-3.0 TB/s
// of HBM-equivalent rate (L2-bound, 14-20 % of the MFMA peak).  Here a workgroup owns an 8 x 16 pixel patch of one
// image: the 10 x 18 halo of the patch is staged in LDS ONCE (rows padded by 16 bytes: conflict-free ds_read_b128 at
// any tap offset), the whole 9-tap filter slice for the workgroup's output channels is LDS-DMA'd once, and the tap loop
// runs entirely out of LDS with compile-time tap offsets and NO barriers.  Epilogue (bf16 pack, coalesced stores, fused
// BN statistics / gradient fan-in addend) is the shared one.
// Requires H % 8 == 0, W % 16 == 0, stride 1, pad 1 (so tiles == M / 128 and the statistics partials keep their layout).
template <int KO, int CI>
struct HaloCfg {
  static constexpr int RB = CI * 2 + 16;                    // padded halo row (bytes)
  static constexpr int HALO = 10 * 18 * RB;
  static constexpr int FILT = 9 * KO * CI * 2;              // the whole 3x3 filter slice of the workgroup's KO rows
  static constexpr int EPI = 128 * (KO * 2 + 16);           // Cfg::EPI
  static constexpr int RED = (256 / (KO / 8)) * KO * 2 * 4; // Cfg::RED
  static constexpr int WORK = cmax(cmax(HALO, EPI), RED);   // halo, then output tile / statistics scratch
  static constexpr int LDS = FILT + WORK;
  static constexpr int PER_CU = (160 * 1024) / LDS < 4 ? (160 * 1024) / LDS : 4;
};

// PERSISTENT and weight-stationary: a workgroup loads its filter slice ONCE and then walks a contiguous run of patches
// (vertical / horizontal neighbours back to back: shared halo rows come from this XCD's L2).  The halo of patch i+1 is
// prefetched into registers while patch i is multiplied and stored, so a workgroup hides its own HBM latency.
template <int KO, int CI, int WGM, int WGN, bool STATS>
__global__ __launch_bounds__(256) void conv_halo_kernel(IGemmArgs p) {
  using C = Cfg<128, KO, CI, WGM, WGN, false, STATS>;
  using H = HaloCfg<KO, CI>;
  constexpr int TM = C::TM, TN = C::TN, WTM = C::WTM, WTN = C::WTN;
  constexpr int HW_ = 18;                           // halo width in pixels (height 10)
  constexpr int RB = H::RB;
  constexpr int CPR = CI / 8;                       // 16-byte chunks per pixel / per filter row
  constexpr int WROWB = CI * 2;                     // filter tile row bytes (XOR-swizzled, as in igemm2)
  constexpr int WTAP = KO * WROWB;                  // one tap's filter tile
  constexpr int KK = CI / 16;
  constexpr int NV = 10 * HW_ * CPR;                // 16-byte vectors of one halo
  constexpr int HP = (NV + 255) / 256;              // halo vectors per thread
  static_assert(H::EPI == C::EPI && H::RED >= C::RED, "epilogue scratch size");
  typedef __attribute__((address_space(3))) void* lptr_t;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* ws = smem;                         // filter (resident)
  unsigned char* xs = smem + H::FILT;               // halo of the current patch; reused by the epilogue

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  const int l31 = lane & 31, lhi = lane >> 5;

  // this workgroup's run of (row-tile) patches; block b runs on XCD b % 8, so give XCD x the x-th eighth of the patches
  const int n_m = p.M >> 7;
  int t_begin, t_end;
  even_run(xcd_contiguous(blockIdx.x, gridDim.x), gridDim.x, n_m, t_begin, t_end);
  const int tiles_x = p.Wi >> 4, tpi = tiles_x * (p.Hi >> 3);

  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w, p.w_bytes);

  // ---- filter: all 9 taps of the KO rows by LDS-DMA (lane-linear destination, swizzle on the source), once ----
  {
    const int chunk = tid % CPR, r0 = tid / CPR;
    constexpr int RPP = 256 / CPR;
    const int csw = (chunk ^ swz<CI>(r0)) << 3;
    const int wrow0 = wave * (64 / CPR);
#pragma unroll
    for (int j = 0; j < (KO + RPP - 1) / RPP; ++j) {
      const int row = r0 + j * RPP;
      const unsigned vw = (row < KO && row < p.Co) ? ((unsigned)row * (unsigned)p.w_row_pitch + (unsigned)csw) * 2u : ASM_OOB;
      if (j * RPP + wrow0 < KO) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(ws + t * WTAP + (j * RPP + wrow0) * WROWB), 16, (int)vw,
                                                   (int)((unsigned)t * (unsigned)p.Ci * 2u), 0, 0);
      }
    }
  }

  // halo vector i of a thread: pixel hp = i / CPR of the 10 x 18 halo, chunk ck
  auto load_halo = [&](int tile, u32x4 (&hv)[HP]) {
    const int img = tile / tpi, trem = tile - img * tpi;
    const int ty = trem / tiles_x, tx = trem - ty * tiles_x;
    const int y0 = ty * 8, x0 = tx * 16;
    const unsigned img_off = (unsigned)img * (unsigned)p.x_img_pitch;
#pragma unroll
    for (int k = 0; k < HP; ++k) {
      const int i = k * 256 + tid;
      const int hp = i / CPR, ck = i - hp * CPR;
      const int hy = hp / HW_, hx = hp - hy * HW_;
      const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
      const bool ok = (i < NV) && ((unsigned)gy < (unsigned)p.Hi) && ((unsigned)gx < (unsigned)p.Wi);
      const unsigned off = (img_off + (unsigned)gy * (unsigned)p.x_row_pitch + (unsigned)gx * (unsigned)p.x_pix_pitch +
                            (unsigned)ck * 8u) * 2u;
      hv[k] = __builtin_amdgcn_raw_buffer_load_b128(rx, ok ? off : ASM_OOB, 0, 0);
    }
  };
  auto store_halo = [&](const u32x4 (&hv)[HP]) {
#pragma unroll
    for (int k = 0; k < HP; ++k) {
      const int i = k * 256 + tid;
      const int hp = i / CPR, ck = i - hp * CPR;
      if (i < NV) *reinterpret_cast<u32x4*>(xs + hp * RB + ck * 16) = hv[k];
    }
  };

  // per-lane fragment bases: activation pixel (py, px) of row m_local -> halo index py * 18 + px (top-left of its window)
  unsigned fxo[TM], fwo[TN];
#pragma unroll
  for (int b = 0; b < TM; ++b) {
    const int row = wm * WTM + b * 32 + l31;
    fxo[b] = (unsigned)(((row >> 4) * HW_ + (row & 15)) * RB + lhi * 16);
  }
#pragma unroll
  for (int a = 0; a < TN; ++a) fwo[a] = (unsigned)((wn * WTN + a * 32 + l31) * WROWB);
  const int wsw = swz<CI>(wn * WTN + l31);   // rows 32 apart share the swizzle term

  u32x4 hv[HP];
  if (t_begin < t_end) load_halo(t_begin, hv);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the filter DMA (and the first halo) have landed

#pragma unroll 1
  for (int tile = t_begin; tile < t_end; ++tile) {
    __syncthreads();                 // the previous patch's epilogue is done with the scratch region (1st trip: filter visible)
    store_halo(hv);
    __syncthreads();
    if (tile + 1 < t_end) load_halo(tile + 1, hv);   // in flight under the MFMAs and the stores of this patch

    f32x16 acc[TN][TM];
    zero_acc(acc);
    // tap loop: fprop (tsign > 0) reads halo (py + r, px + s) with filter tap (r, s); the input gradient (tsign < 0)
    // reads halo (py + 2 - r, px + 2 - s) with the same filter tap (dx(h, w) = sum dy(h + 1 - r, w + 1 - s) . w(r, s))
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int r = t / 3, q = t - r * 3;
      const int hoff = (p.tsign > 0 ? (r * HW_ + q) : ((2 - r) * HW_ + (2 - q))) * RB;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        bf16x8 fw[TN], fx[TM];
#pragma unroll
        for (int a = 0; a < TN; ++a)
          fw[a] = *reinterpret_cast<const bf16x8*>(ws + t * WTAP + fwo[a] + (((kk * 2 + lhi) ^ wsw) << 4));
#pragma unroll
        for (int b = 0; b < TM; ++b) fx[b] = *reinterpret_cast<const bf16x8*>(xs + fxo[b] + hoff + kk * 32);
#pragma unroll
        for (int a = 0; a < TN; ++a)
#pragma unroll
          for (int b = 0; b < TM; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[a], fx[b], acc[a][b], 0, 0, 0);
      }
    }
    __syncthreads();   // every wave is done reading the halo: the epilogue reuses the region for the output tile
    const int img = tile / tpi, trem = tile - img * tpi;
    const int ty = trem / tiles_x, tx = trem - ty * tiles_x;
    const int patch_base = (img * p.Hi + ty * 8) * p.Wi + tx * 16;
    igemm_epilogue<C, 128, KO, WTM, WTN, TM, TN, false, STATS>(p, acc, xs, tile, 0, tid, wm, wn, l31, lhi, patch_base);
  }
}

template <int KO, int CI, int WGM, int WGN, bool STATS>
int launch_halo_one(const IGemmArgs& a, hipStream_t st) {
  using H = HaloCfg<KO, CI>;
  return asm_launch_dyn_lds<conv_halo_kernel<KO, CI, WGM, WGN, STATS>>("conv_halo_kernel", dim3(a.n_blocks), dim3(256), H::LDS, st, a);
}

template <int KO, int CI, int WGM, int WGN>
int launch_halo(const ConvLaunch& L, const IGemmArgs& a, hipStream_t st) {
  return L.epi == EPI_STATS ? launch_halo_one<KO, CI, WGM, WGN, true>(a, st) : launch_halo_one<KO, CI, WGM, WGN, false>(a, st);
}

// is the layer one the halo kernel covers?
bool halo_covers(const IGemmArgs& a, bool out_f32) {
  if (out_f32 || a.R != 3 || a.S != 3 || a.so != 1 || a.sd != 1 || a.y_strided || a.bn_scale) return false;
  if (a.Hi % 8 || a.Wi % 16 || a.M != (a.HoWo / a.Wo) * a.Wo * (a.M / a.HoWo) || a.HoWo != a.Hi * a.Wi) return false;
  if (!packed_input(a) || !pad1_window(a) || !whole_3x3_filter(a)) return false;
  return (a.Ci == 32 || a.Ci == 64) && (a.Co == 32 || a.Co == 64);
}

template <int BM, int BN, int BK, int WGM, int WGN, bool OUT_F32, bool STATS, int R, int S, int NS = 2, bool PFA = false, bool POOL = false,
          int SCHED = 0, bool BNRED = false>
int launch2_one(const IGemmArgs& a, hipStream_t st) {
  using C = Cfg2<BM, BN, BK, WGM, WGN, OUT_F32, STATS, NS>;
  constexpr int NTHR = 64 * WGM * WGN;
  // measured (tools/conv_bench.py, same box, round 3): spreading the DMA issue is +2..4 % on the 3x3 layers (7 of 8 shapes,
  // fprop and dgrad) and -3..6 % on the deep 1x1 layers (their steps are short: the last pieces land too late), hence the
  // per-layer choice
  if constexpr (SCHED == 0 && BK == 64 && BN >= 128 && !OUT_F32 && !POOL && ((R == 3 && S == 3) || (R == 1 && S == 1))) {
    if (R == 3) return launch2_one<BM, BN, BK, WGM, WGN, OUT_F32, STATS, R, S, NS, PFA, POOL, 1>(a, st);
  }
  return asm_launch_dyn_lds<igemm2_kernel<BM, BN, BK, WGM, WGN, OUT_F32, STATS, R, S, NS, PFA, POOL, SCHED, BNRED>>(
      "igemm2_kernel", dim3(a.n_blocks), dim3(NTHR), C::LDS, st, a);
}

// the epilogue variants igemm2_kernel is instantiated with (launch2) for an R x S tap shape on a BM x BN x BK tile: every one
// for the 1x1 layers; the 3x3 layers without f32 output, pooled gradient or batch-norm backward sums; the parity classes of a
// stride-2 3x3 input gradient (1x2, 2x1, 2x2) plain; the two stems (7x1, 3x1 over the 4-channel halo buffer) on the small tiles
constexpr unsigned igemm2_variants(int R, int S, int BM, int BN, int BK) {
  if (R == 1 && S == 1)
    return epi_bit(EPI_F32) | epi_bit(EPI_BNRED) | epi_bit(EPI_STATS) | epi_bit(EPI_POOL) | epi_bit(EPI_PFA) | epi_bit(EPI_PLAIN);
  if (R == 3 && S == 3) return epi_bit(EPI_STATS) | epi_bit(EPI_PFA) | epi_bit(EPI_PLAIN);
  if ((R == 1 && S == 2) || (R == 2 && S == 1) || (R == 2 && S == 2)) return epi_bit(EPI_PLAIN);
  if ((R == 7 || R == 3) && S == 1 && BK == 32 && BM == 128 && BN <= 64) return epi_bit(EPI_STATS) | epi_bit(EPI_PLAIN);
  return 0;
}

template <int BM, int BN, int BK, int WGM, int WGN, int R, int S>
int launch2_rs(const ConvLaunch& L, const IGemmArgs& a, hipStream_t st) {
  constexpr unsigned has = igemm2_variants(R, S, BM, BN, BK);
  if constexpr ((has >> EPI_F32) & 1)
    if (L.epi == EPI_F32) return launch2_one<BM, BN, BK, WGM, WGN, true, false, R, S>(a, st);
  if constexpr ((has >> EPI_BNRED) & 1)
    if (L.epi == EPI_BNRED) return launch2_one<BM, BN, BK, WGM, WGN, false, true, R, S, 2, false, false, 0, true>(a, st);
  if constexpr ((has >> EPI_STATS) & 1)
    if (L.epi == EPI_STATS) return launch2_one<BM, BN, BK, WGM, WGN, false, true, R, S>(a, st);
  if constexpr ((has >> EPI_POOL) & 1)
    if (L.epi == EPI_POOL) return launch2_one<BM, BN, BK, WGM, WGN, false, false, R, S, 2, false, true>(a, st);
  if constexpr ((has >> EPI_PFA) & 1)
    if (L.epi == EPI_PFA) return launch2_one<BM, BN, BK, WGM, WGN, false, false, R, S, 2, true>(a, st);
  if constexpr ((has >> EPI_PLAIN) & 1)
    if (L.epi == EPI_PLAIN) return launch2_one<BM, BN, BK, WGM, WGN, false, false, R, S>(a, st);
  return conv_no_variant("igemm2_kernel", L.epi);
}

template <int BM, int BN, int BK, int WGM, int WGN>
struct Launch2 {
  static int run(const ConvLaunch& L, const IGemmArgs& a, hipStream_t st) {
    if (a.R == 1 && a.S == 1) return launch2_rs<BM, BN, BK, WGM, WGN, 1, 1>(L, a, st);
    if (a.R == 3 && a.S == 3) return launch2_rs<BM, BN, BK, WGM, WGN, 3, 3>(L, a, st);
    if (a.R == 1 && a.S == 2) return launch2_rs<BM, BN, BK, WGM, WGN, 1, 2>(L, a, st);
    if (a.R == 2 && a.S == 1) return launch2_rs<BM, BN, BK, WGM, WGN, 2, 1>(L, a, st);
    if (a.R == 2 && a.S == 2) return launch2_rs<BM, BN, BK, WGM, WGN, 2, 2>(L, a, st);
    if (a.R == 7 && a.S == 1) return launch2_rs<BM, BN, BK, WGM, WGN, 7, 1>(L, a, st);
    if (a.R == 3 && a.S == 1) return launch2_rs<BM, BN, BK, WGM, WGN, 3, 1>(L, a, st);
    return conv_no_variant("igemm2_kernel", L.epi);
  }
};

template <int BM, int BN, int BK, int WGM, int WGN, bool OUT_F32, bool STATS, bool BNRED = false>
int launch_one(const IGemmArgs& a, hipStream_t st) {
  using C = Cfg<BM, BN, BK, WGM, WGN, OUT_F32, STATS>;
  return asm_launch_dyn_lds<igemm_kernel<BM, BN, BK, WGM, WGN, OUT_F32, STATS, BNRED>>("igemm_kernel", dim3(a.n_blocks), dim3(C::NT),
                                                                                   C::LDS, st, a);
}

template <int BM, int BN, int BK, int WGM, int WGN>
struct LaunchGeneral {
  static int run(const ConvLaunch& L, const IGemmArgs& a, hipStream_t st) {
    switch (L.epi) {
      case EPI_F32: return launch_one<BM, BN, BK, WGM, WGN, true, false>(a, st);
      case EPI_BNRED: return launch_one<BM, BN, BK, WGM, WGN, false, true, true>(a, st);
      case EPI_STATS: return launch_one<BM, BN, BK, WGM, WGN, false, true>(a, st);
      case EPI_PLAIN: return launch_one<BM, BN, BK, WGM, WGN, false, false>(a, st);
    }
    return conv_no_variant("igemm_kernel", L.epi);
  }
};

// the plan's tile as template arguments (the seven tiles of pick_tile)
template <template <int, int, int, int, int> class F>
int on_tile(const ConvLaunch& L, const IGemmArgs& a, hipStream_t st) {
  const ConvTile& t = L.t;
  if (t.bm == 256) return F<256, 256, 64, 4, 2>::run(L, a, st);
  if (t.bn == 32) return t.bk == 64 ? F<128, 32, 64, 4, 1>::run(L, a, st) : F<128, 32, 32, 4, 1>::run(L, a, st);
  if (t.bn == 64) return t.bk == 64 ? F<128, 64, 64, 2, 2>::run(L, a, st) : F<128, 64, 32, 2, 2>::run(L, a, st);
  return t.bk == 64 ? F<128, 128, 64, 2, 2>::run(L, a, st) : F<128, 128, 32, 2, 2>::run(L, a, st);
}

// ---- the plan ----
// what a launch writes: bf16, f32, bf16 + the batch-norm statistics, bf16 + the batch-norm backward sums (IGemmArgs::red_y)
enum class ConvOut { bf16, f32, stats, bnred };

// The MFMA-bound layers (K = R*S*C >= 512) go on 256 x 256 / 8 waves once there are >= 192 such tiles (C >= 256 outputs);
// asm_tuning.igemm_tile = 1 / 3 forces 128-row tiles / 256 x 256 (where Ci % 64 == 0).
bool tile256(const IGemmArgs& a) {
  const int ftile = asm_tune().igemm_tile;
  if (ftile == 1) return false;
  if (ftile == 3 && a.Ci % 64 == 0) return true;
  const long long b256 = (long long)cdiv(a.M, 256) * cdiv(a.Co, 256);
  return a.Ci % 64 == 0 && (long long)a.R * a.S * a.Ci >= 512 && a.Co >= 256 && b256 >= 192;
}

// The tile of igemm2 and of the general kernel.  Measured on MI355X (tools/conv_bench.py, Assemble-ResNet-50 shapes, batch 256):
//  * HBM-bound layers (1x1, and everything at 112x112): LDS-DMA staging + the smallest footprint wins
//    (3-8 workgroups per CU hide the load round trip of the very short K loops);
//  * MFMA-bound layers: tile256.
// 1x1 layers stage 32 channels per step (smallest footprint: the bandwidth-bound ones want many workgroups per CU) --
// except deep reductions on few tiles (7x7 / 14x14 / 28x28 maps), where each of the K / 32 steps is an exposed DMA
// round trip behind a barrier: up to 4000 tiles of 128 x 128 they take 64-channel steps (tools/conv_bench.py, all 1x1
// shapes of the network: fprop 2.36 -> 2.31 ms, input gradients 2.11 -> 2.03 ms per step).
ConvTile pick_tile(const IGemmArgs& a) {
  const long long t128 = (long long)cdiv(a.M, 128) * cdiv(a.Co, 128);
  const bool bk64 = a.Ci % 64 == 0 && (a.R * a.S > 1 || (a.Ci >= 256 && t128 <= 4000));
  if (a.Co <= 32) return bk64 ? ConvTile{128, 32, 64, 4, 1} : ConvTile{128, 32, 32, 4, 1};
  if (a.Co <= 64) return bk64 ? ConvTile{128, 64, 64, 2, 2} : ConvTile{128, 64, 32, 2, 2};
  if (tile256(a)) return ConvTile{256, 256, 64, 4, 2};
  return bk64 ? ConvTile{128, 128, 64, 2, 2} : ConvTile{128, 128, 32, 2, 2};
}

unsigned family_variants(int family, const IGemmArgs& a, const ConvTile& t) {
  switch (family) {
    case FAM_GENERAL: return epi_bit(EPI_F32) | epi_bit(EPI_BNRED) | epi_bit(EPI_STATS) | epi_bit(EPI_PLAIN);
    case FAM_IGEMM2: return igemm2_variants(a.R, a.S, t.bm, t.bn, t.bk);
    case FAM_HALO: return epi_bit(EPI_STATS) | epi_bit(EPI_PLAIN);
    case FAM_DENSE: return epi_bit(EPI_F32) | epi_bit(EPI_PLAIN);
    case FAM_GEMM1: return epi_bit(EPI_BNRED) | epi_bit(EPI_STATS) | epi_bit(EPI_POOL) | epi_bit(EPI_PFA) | epi_bit(EPI_PLAIN);
    default: return epi_bit(EPI_BNRED) | epi_bit(EPI_STATS) | epi_bit(EPI_PFA) | epi_bit(EPI_PLAIN);   // igemm3, igemm8
  }
}

// One launch of `family` on tile t over row tiles m_tile0 .. cdiv(M, BM) - 1, with its epilogue variant.  The addend-prefetching
// epilogue (PFA, see igemm_epilogue) goes where a launch is one round of few workgroups (<= 1024), on every 256-row tile (one
// workgroup per CU anyway: igemm8, igemm2's 256 x 256) and never on a strided output (parity classes); asm_tuning.igemm_pfa =
// 0 / 1 forces it off / on wherever the family has the variant.
ConvLaunch tiled(int family, ConvTile t, const IGemmArgs& a, ConvOut out, int M, int m_tile0) {
  ConvLaunch L = {};
  L.family = family; L.t = t; L.M = M; L.m_tile0 = m_tile0;
  L.n_tiles_n = cdiv(a.Co, t.bn);
  L.n_blocks = (cdiv(M, t.bm) - m_tile0) * L.n_tiles_n;
  L.kchunks = cdiv(a.Ci, t.bk);
  const unsigned has = family_variants(family, a, t);
  const int pfa_env = asm_tune().igemm_pfa;
  const bool pfa = (has & epi_bit(EPI_PFA)) && a.addend != nullptr && !a.y_strided &&
                   (pfa_env >= 0 ? pfa_env != 0 : (t.bm == 256 || L.n_blocks <= 1024));
  const int want = out == ConvOut::f32 ? EPI_F32 : out == ConvOut::bnred ? EPI_BNRED : out == ConvOut::stats ? EPI_STATS
                   : a.pool_dy ? EPI_POOL : pfa ? EPI_PFA : EPI_PLAIN;
  L.epi = (has & epi_bit(want)) ? want : -1;
  if (family == FAM_IGEMM3) {   // a layer with one 64-channel chunk has one halo buffer, of 192 rows up to 30 pixels wide
    L.nhb = a.Ci == 64 ? 1 : 2;
    L.hr = a.Ci == 64 && a.Wi > 30 ? 256 : 192;
  }
  return L;
}

ConvPlan single(const ConvLaunch& L) { return ConvPlan{1, {L, {}}, nullptr}; }
ConvPlan no_plan(const char* why) { return ConvPlan{0, {}, why}; }

// asm_dense_shaped (igemm_common.h: why there are two, and that they must agree) on the argument block of the launch
bool dense_shaped(const IGemmArgs& a) {
  return a.Hi == 1 && a.Wi == 1 && a.HoWo == 1 && a.R == 1 && a.S == 1 && a.x_img_pitch == a.Ci && a.x_row_pitch == a.Ci &&
         a.x_pix_pitch == a.Ci;
}
// Does dense_small_kernel take the launch?  Forward and input gradient alike (dgrad_args maps dy / wt / dx onto x / w / y): a
// dense-shaped layer that writes the plain product (+ an unmasked addend) to rows asm_dense_small accepts, from 16-byte aligned
// operands (an absent one counts as aligned); asm_tuning.dense_small = 0: never.
bool dense_covers(const IGemmArgs& a, ConvOut out) {
  if (!asm_tune().dense_small || !dense_shaped(a) || a.Ci % 16 || (out != ConvOut::bf16 && out != ConvOut::f32)) return false;
  if (a.addend_mask || a.pool_dy || a.bn_scale || a.y_strided) return false;
  if (a.ldy % 4 || a.ldy > cdiv(a.Co, 32) * 32) return false;   // the pad columns end inside the last 32-column tile
  return asm_aligned16(a.x) && asm_aligned16(a.w) && asm_aligned16(a.y) && asm_aligned16(a.addend);
}

// The kernel of a forward / input-gradient layer: family, tile, epilogue variant, grid.  Pure: reads the arguments,
// asm_tuning and the CU count only.  Where a family's coverage predicate accepts the layer, it takes it, in this order:
// dense_small (the [N,1,1,C] layers, whatever igemm_mode / igemm_tile say), conv_halo (the narrow 112-wide 3x3 layers), igemm1
// (the 1x1 layers of conv_gemm1.hip's table), igemm8 / igemm3 (3x3 stride 1), igemm2 (the gather-free general form), the general kernel.  asm_tuning.igemm_mode = 1 sends every layer to the general kernel,
// igemm_tile != 0 keeps the specialised families out.
ConvPlan plan_conv(const IGemmArgs& a, ConvOut out) {
  const asm_tuning& tu = asm_tune();
  const bool f32 = out == ConvOut::f32, stats = out == ConvOut::stats || out == ConvOut::bnred;
  const bool k1 = a.R == 1 && a.S == 1;
  // the batch-norm backward sums of a 3x3 input gradient: only igemm8 and igemm3 have that instantiation (in the bandwidth-bound
  // halo kernel of the 112-wide maps the y reads cost 0.22 ms per step and saved 0.09 of reduce passes: measured, removed)
  const bool bnred3 = out == ConvOut::bnred && !k1;
  // (32 x 32 output tiles, 16-channel steps split over the workgroup's four waves)
  if (dense_covers(a, out)) return single(tiled(FAM_DENSE, ConvTile{32, 32, 16, 1, 1}, a, out, a.M, 0));
  if (dense_shaped(a) && (a.pool_dy || out == ConvOut::bnred))
    return no_plan("conv dgrad: the fused input-gradient forms do not take a [N,1,1,C] layer");
  if (a.pool_dy && (tu.igemm_mode != 0 || out != ConvOut::bf16 || !k1 || a.y_strided))
    return no_plan("conv dgrad_pooled: only the 1x1 stride-1 igemm2 path folds an average-pool backward in");
  if (tu.igemm_mode == 0 && tu.igemm_tile == 0) {
    if (halo_covers(a, f32)) {
      if (bnred3) return no_plan("conv dgrad_bnred: no kernel with the batch-norm sums for this 3x3 layer");
      const int ko = a.Co, ci = a.Ci;
      ConvLaunch L = tiled(FAM_HALO, ConvTile{128, ko, ci, ko == 32 ? 4 : 2, ko == 32 ? 1 : 2}, a, out, a.M, 0);
      const int per_cu = ko == 32 ? (ci == 32 ? HaloCfg<32, 32>::PER_CU : HaloCfg<32, 64>::PER_CU)
                                  : (ci == 32 ? HaloCfg<64, 32>::PER_CU : HaloCfg<64, 64>::PER_CU);
      L.n_blocks = a.M / 128 < per_cu * 256 ? a.M / 128 : per_cu * 256;    // persistent: at most per_cu rounds of the chip
      return single(L);
    }
    ConvTile t1;
    if (const int code = asm_gemm1_config(a, f32, stats, &t1)) {   // the ring-pipelined GEMM form of the 1x1 layers
      ConvLaunch L = tiled(FAM_GEMM1, t1, a, out, a.M, 0);
      L.gemm1 = code;
      return single(L);
    }
    // igemm3_kernel (128 x 128 tiles, activation rows resident across the taps, two workgroups per CU) against igemm2
    // (tools/conv_bench.py --iters 50, same box, steady state): it wins wherever igemm2 would run 128-row tiles
    // (28x28x128 -> 256 input gradient 124 -> 112 us, 7x7x256 -> 512 37 -> 35 / 48.6 -> 40, 7x7x512 -> 1024 input gradient
    // 114 -> 108, 14x14x128 -> 256 input gradient 35.8 -> 33.2) and on the 784-tile short-reduction forward layer
    // (28x28x128 -> 256: 131 -> 117.5); against the 256 x 256 tile it loses 3 - 15 % where that tile fills the chip
    // (its 8-wave loop reads 0.75 instead of 1 LDS fragment per MFMA and has half the barriers), so those stay -- on
    // igemm8_kernel, the 256 x 256 tile on the wave-staggered multi-phase loop (bit-identical results).
    // asm_tuning.igemm3 = 2 forces igemm3 wherever the shape allows, igemm8 = 2 igemm8.
    const int h3 = tu.igemm3, h8 = tu.igemm8;
    const ConvTile t128 = {128, 128, 64, 2, 2};           // igemm3's tile
    const bool big = tile256(a);
    const long long b256 = (long long)cdiv(a.M, 256) * cdiv(a.Co, 256);
    // (the short-reduction layers on >= 768 tiles stay on igemm3: 28x28x128 -> 256 forward 127 us there, 131 us on igemm8)
    const bool to_igemm3 = h3 && b256 >= 768 && a.Ci <= 128;
    const bool cov3 = h3 && igemm3_covers(a, f32);
    if (((h8 == 1 && big && !to_igemm3) || h8 == 2) && asm_igemm8_covers(a, f32)) {
      const ConvTile t8 = {256, 256, 64, 2, 4};
      // The ragged last round.  One 128 KB workgroup per CU: n tiles take ceil(n / CUs) rounds, and 784 tiles on 256 CUs
      // (14x14x512 -> 1024 and 28x28x128 -> 256 at batch 256) spend a whole round on their last 16.  When the tail is short,
      // the row tiles of the full rounds go to igemm8 and the remaining rows to the 128 x 128 kernels (igemm3, else igemm2's
      // 128 x 128 x 64: four times the workgroups, two per CU, the same accumulation order -- the tensor stays bit-identical):
      // 3 rounds + one small round (~0.3 of a big one when there is at most one small tile per CU, ~0.5 per round of two)
      // instead of 4.  Measured (14x14x512 -> 1024 forward, same box): 490.2 us igemm2, 455.5 us split (three igemm8 rounds
      // ~355 us + ~100 us for the 64 small tiles, which run one per CU and are latency-bound: 72 lock-step steps).  The batch-norm
      // backward sums need igemm3 for the rest.
      const int cus = asm_num_cus();
      const int nt8 = cdiv(a.Co, 256), mt8 = cdiv(a.M, 256);
      const long long n8 = (long long)nt8 * mt8;
      const int m_full = (int)((n8 / cus) * cus / nt8);                 // row tiles of the full rounds
      const long long rem = n8 - (long long)m_full * nt8;              // 256 x 256 tiles left over
      const double small = 4 * rem <= cus ? 0.3 : 0.5 * (double)((4 * rem + 2 * cus - 1) / (2 * cus));
      const double split_cost = (double)((long long)m_full * nt8 / cus) + small, whole_cost = (double)((n8 + cus - 1) / cus);
      if (h8 == 1 && m_full > 0 && rem > 0 && split_cost < whole_cost - 0.15 && (cov3 || !bnred3)) {
        // (the head's gather is bounded by the tensor, not by M)
        return ConvPlan{2, {tiled(FAM_IGEMM8, t8, a, out, m_full * 256, 0),
                            tiled(cov3 ? FAM_IGEMM3 : FAM_IGEMM2, t128, a, out, a.M, m_full * 2)},
                        nullptr};
      }
      return single(tiled(FAM_IGEMM8, t8, a, out, a.M, 0));
    }
    if (cov3 && (h3 == 2 || !big || to_igemm3)) return single(tiled(FAM_IGEMM3, t128, a, out, a.M, 0));
  }
  if (bnred3) return no_plan("conv dgrad_bnred: no kernel with the batch-norm sums for this 3x3 layer");
  const ConvTile t = pick_tile(a);
  if (tu.igemm_mode == 0) {
    const ConvLaunch L = tiled(FAM_IGEMM2, t, a, out, a.M, 0);
    if (L.epi >= 0 && (a.Ci % t.bk == 0 || a.Ci <= t.bk)) return single(L);
    if (a.pool_dy) return no_plan("conv dgrad_pooled: no igemm2 instantiation for this shape");
  }
  return single(tiled(FAM_GENERAL, t, a, out, a.M, 0));
}

// the dispatcher: each launch of the plan on its template instantiation
int run_plan(const ConvPlan& p, IGemmArgs a, hipStream_t st) {
  if (p.n == 0) ASM_FAIL(ASM_ENOTSUP, "%s", p.why);
  a.fd_howo = make_fastdiv((unsigned)a.HoWo);
  a.fd_wo = make_fastdiv((unsigned)a.Wo);
  for (int i = 0; i < p.n; ++i) {
    const ConvLaunch& L = p.l[i];
    a.M = L.M; a.m_tile0 = L.m_tile0; a.n_tiles_n = L.n_tiles_n; a.n_blocks = L.n_blocks; a.kchunks = L.kchunks;
    a.fd_ntn = make_fastdiv((unsigned)L.n_tiles_n);
    int rc;
    switch (L.family) {
      case FAM_GENERAL: rc = on_tile<LaunchGeneral>(L, a, st); break;
      case FAM_GEMM1: rc = asm_gemm1_launch(L, a, st); break;
      case FAM_IGEMM2: rc = on_tile<Launch2>(L, a, st); break;
      case FAM_IGEMM3: rc = L.nhb == 2 ? launch3<192, 2>(L, a, st) : L.hr == 192 ? launch3<192, 1>(L, a, st) : launch3<256, 1>(L, a, st); break;
      case FAM_HALO:   // KO = BN output, CI = BK input channels
        rc = L.t.bn == 32 ? (L.t.bk == 64 ? launch_halo<32, 64, 4, 1>(L, a, st) : launch_halo<32, 32, 4, 1>(L, a, st))
                          : (L.t.bk == 64 ? launch_halo<64, 64, 2, 2>(L, a, st) : launch_halo<64, 32, 2, 2>(L, a, st));
        break;
      case FAM_IGEMM8: rc = asm_igemm8_launch(L, a, st); break;
      case FAM_DENSE:
        rc = asm_dense_small_launch(a.x, a.Ci, a.w, a.Ci, a.M, a.Co, a.Ci, a.y, a.ldy, L.epi == EPI_F32, a.addend, st);
        break;
      default: ASM_FAIL(ASM_EINVAL, "conv: no kernel family %d", L.family);
    }
    if (rc != ASM_OK) return rc;
  }
  asm_last_conv_kernel = p.l[p.n - 1].family;
  return ASM_OK;
}

int check_desc(const asm_conv_desc* d) {
  ASM_REQUIRE(d != nullptr, "conv: null descriptor");
  ASM_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->K > 0 && d->R > 0 && d->S > 0,
              "conv: non-positive dimension");
  ASM_REQUIRE(d->C % 8 == 0, "conv: C=%d must be a multiple of 8", d->C);
  ASM_REQUIRE(d->stride == 1 || d->stride == 2, "conv: stride %d not supported", d->stride);
  ASM_REQUIRE(d->Ho > 0 && d->Wo > 0, "conv: bad output size");
  ASM_REQUIRE(d->pad >= 0 && d->pad < 64, "conv: bad pad");
  return ASM_OK;
}

}  // namespace

static inline int64_t img_pitch(const asm_conv_desc* d) {
  return d->x_img_pitch ? d->x_img_pitch : (int64_t)d->H * d->W * d->C;
}
static inline int row_pitch(const asm_conv_desc* d) { return d->x_row_pitch ? d->x_row_pitch : d->W * d->C; }
static inline int pix_pitch(const asm_conv_desc* d) { return d->x_pix_pitch ? d->x_pix_pitch : d->C; }

extern "C" int asm_debug_last_conv_kernel(void) { return asm_last_conv_kernel; }

extern "C" int asm_conv2d_stats_blocks(const asm_conv_desc* d) {
  if (!d) return ASM_EINVAL;
  return cdiv(d->N * d->Ho * d->Wo, STATS_BM);
}

static int fprop_impl(const asm_conv_desc* d, const void* x, const void* w, void* y, float* stats_partial,
                      const float* bn_scale, const float* bn_shift, const void* residual, int relu, void* stream) {
  if (int e = check_desc(d)) return e;
  ASM_REQUIRE(x && w && y, "conv fprop: null pointer");
  const int64_t xelems = (int64_t)d->N * img_pitch(d);
  ASM_REQUIRE(xelems * 2 < (int64_t)ASM_OOB, "conv fprop: input larger than 2 GiB");
  const int ldy = d->ldy ? d->ldy : d->K;
  ASM_REQUIRE(ldy % (d->out_f32 ? 4 : 8) == 0 && ldy >= d->K, "conv fprop: bad ldy %d", ldy);
  ASM_REQUIRE(!(stats_partial && d->out_f32), "conv fprop: fused statistics need bf16 output");
  IGemmArgs a = {};
  a.x = x; a.w = w; a.y = y; a.addend = residual; a.stats = stats_partial;
  a.x_bytes = (unsigned)(xelems * 2);
  a.w_bytes = (unsigned)((int64_t)d->K * d->R * d->S * d->C * 2);
  a.M = d->N * d->Ho * d->Wo;
  a.Hi = d->H; a.Wi = d->W; a.Ci = d->C;
  a.Wo = d->Wo; a.HoWo = d->Ho * d->Wo;
  a.Co = d->K; a.ldy = ldy;
  a.R = d->R; a.S = d->S;
  a.so = d->stride; a.sd = 1; a.tsign = 1; a.pad = d->pad;
  a.pad_w = a.pad; a.wt0 = 0; a.wtr = a.S; a.wts = 1;
  a.bn_scale = bn_scale; a.bn_shift = bn_shift; a.bn_relu = relu;
  a.x_img_pitch = (int)img_pitch(d); a.x_row_pitch = row_pitch(d); a.x_pix_pitch = pix_pitch(d);
  a.w_row_pitch = d->R * d->S * d->C;
  const ConvOut out = d->out_f32 ? ConvOut::f32 : stats_partial ? ConvOut::stats : ConvOut::bf16;
  return run_plan(plan_conv(a, out), a, (hipStream_t)stream);
}

extern "C" int asm_conv2d_fprop(const asm_conv_desc* d, const void* x, const void* w, void* y,
                                float* stats_partial, void* stream) {
  return fprop_impl(d, x, w, y, stats_partial, nullptr, nullptr, nullptr, 0, stream);
}

extern "C" int asm_conv2d_fprop_bn(const asm_conv_desc* d, const void* x, const void* w, void* y, const float* scale,
                                   const float* shift, const void* residual, int relu, void* stream) {
  ASM_REQUIRE(d && scale && shift, "conv fprop_bn: null pointer");
  ASM_REQUIRE(!d->out_f32 && d->K % 8 == 0, "conv fprop_bn: needs bf16 output and K %% 8 == 0 (K=%d)", d->K);
  ASM_REQUIRE(d->ldy == 0 || d->ldy == d->K, "conv fprop_bn: padded output rows not supported");
  return fprop_impl(d, x, w, y, nullptr, scale, shift, residual, relu ? 1 : 0, stream);
}

struct PoolAdd {
  const void* dy;
  int k, stride, pad, Hp, Wp, cv;
};
struct BnRed {      // asm_conv2d_dgrad_bnred: batch-norm backward sums of the gradient this launch writes
  const void* y;
  const uint8_t* mask;
  float* partial;
};
static int dgrad_impl(const asm_conv_desc* d, const void* dy, const void* wt, const void* addend,
                      const uint8_t* addend_mask, void* dx, void* stream, const PoolAdd* pool = nullptr,
                      const BnRed* red = nullptr);
// the input gradient as the generic gather over dy (p = (h + pad - r) / stride when divisible), without its tensors:
// M = N*H*W rows of dx, N = C, the reduction over K*R*S
static IGemmArgs dgrad_args(const asm_conv_desc* d) {
  IGemmArgs a = {};
  a.x_bytes = (unsigned)((int64_t)d->N * d->Ho * d->Wo * d->K * 2);
  a.w_bytes = (unsigned)((int64_t)d->K * d->R * d->S * d->C * 2);
  a.M = d->N * d->H * d->W;
  a.Hi = d->Ho; a.Wi = d->Wo; a.Ci = d->K;
  a.Wo = d->W; a.HoWo = d->H * d->W;
  a.Co = d->C; a.ldy = d->C;
  a.R = d->R; a.S = d->S;
  a.so = 1; a.sd = d->stride; a.tsign = -1; a.pad = -d->pad; a.pad_w = a.pad;
  a.x_img_pitch = d->Ho * d->Wo * d->K; a.x_row_pitch = d->Wo * d->K; a.x_pix_pitch = d->K;
  a.w_row_pitch = d->R * d->S * d->K;
  a.wt0 = 0; a.wtr = a.S; a.wts = 1;
  return a;
}
// the descriptor checks of every input-gradient entry point
static int dgrad_check(const asm_conv_desc* d) {
  if (int e = check_desc(d)) return e;
  ASM_REQUIRE(d->K % 8 == 0, "conv dgrad: K=%d must be a multiple of 8 (pad dy)", d->K);
  ASM_REQUIRE(d->x_img_pitch == 0 && d->x_row_pitch == 0 && d->x_pix_pitch == 0 && !d->out_f32,
              "conv dgrad: custom pitches / f32 output not supported");
  const int64_t dyelems = (int64_t)d->N * d->Ho * d->Wo * d->K;
  ASM_REQUIRE(dyelems * 2 < (int64_t)ASM_OOB, "conv dgrad: dy larger than 2 GiB");
  return ASM_OK;
}
// conv_dgrad_s2.hip: the one-launch 3x3 / stride-2 input gradient
bool asm_dgrad_s2_covers(const asm_conv_desc* d);
int asm_dgrad_s2_launch(const asm_conv_desc* d, const void* dy, const void* wt, const void* addend, const uint8_t* addend_mask,
                        void* dx, void* stream);

// The kernels of an input gradient, all chosen before the first launch: dense_small_kernel (through plan_conv, whatever the
// stride of the [N,1,1,C] layer), dgrad_s2_kernel, the parity classes of a stride-2 layer, or the plan_conv plan of the generic
// gather (which also carries an ASM_ENOTSUP).
enum class DgradForm { conv, parity, s2 };
struct DgradPlan {
  DgradForm form;
  int nc;                     // parity: classes, each a dense stride-1 gather over dy (cls[i]) on its plan (cp[i])
  IGemmArgs cls[4];
  ConvPlan cp[4];
  bool fill;                  // parity of a 1x1 layer: fill dx (zeros or the addend) before its one class writes
  ConvPlan conv;              // conv
};

// Pure: reads the descriptor, which operands `a` has, asm_tuning and the CU count.  aligned: dy, wt, dx and the addend are
// 16-byte aligned (dgrad_s2_kernel's vector accesses).
static DgradPlan plan_dgrad(const asm_conv_desc* d, const IGemmArgs& a, ConvOut out, bool aligned) {
  DgradPlan p = {};
  const asm_tuning& tu = asm_tune();
  const bool k3 = d->R == 3 && d->S == 3, k1 = d->R == 1 && d->S == 1 && d->pad == 0;
  if (dense_covers(a, out)) {
    p.conv = plan_conv(a, out);
    return p;
  }
  if (aligned && !a.pool_dy && asm_dgrad_s2_covers(d)) {   // all four parity classes in one launch
    p.form = DgradForm::s2;
    return p;
  }
  // Stride-2 3x3: three quarters of the (pixel, tap) pairs of the generic gather are parity misses (multiplied as
  // zeros).  Split dx into its four (h % 2, w % 2) classes instead: within a class every pixel uses the same
  // 1 / 2 / 2 / 4 taps, so each class is a dense stride-1 gather over dy with a 1x1 / 1x2 / 2x1 / 2x2 sub-filter
  //   dx(2hh+ph, 2ww+pw) = sum_{i,j} dy(hh + dh0 - i, ww + dw0 - j) . w(r0 + 2i, s0 + 2j),
  //   r0 = (ph + pad) & 1, dh0 = (ph + pad - r0) / 2   (same for columns)
  // written through the strided-output epilogue: 9/4 instead of 9 tap passes.  A 1x1 / 2 projection touches only the
  // (even, even) class.  Taken only if every class has a gather-free kernel; otherwise the whole layer is the generic gather.
  if (tu.dgrad_parity && d->stride == 2 && (k3 || k1) && tu.igemm_mode == 0) {
    if (k1 && a.addend_mask) {
      p.conv = no_plan("conv dgrad_masked: a masked addend is not supported for the 1x1 stride-2 input gradient");
      return p;
    }
    for (int cls = 0; cls < 4; ++cls) {
      const int ph = cls >> 1, pw = cls & 1;
      const int Hc = (d->H - ph + 1) / 2, Wc = (d->W - pw + 1) / 2;
      const int r0 = (ph + d->pad) & 1, s0 = (pw + d->pad) & 1;
      const int Rc = (d->R - r0 + 1) / 2, Sc = (d->S - s0 + 1) / 2;   // taps r0, r0 + 2, ... (< R)
      if (Hc <= 0 || Wc <= 0 || Rc <= 0 || Sc <= 0) continue;
      IGemmArgs& c = p.cls[p.nc];
      c = a;
      c.R = Rc; c.S = Sc;
      c.M = d->N * Hc * Wc;
      c.Wo = Wc; c.HoWo = Hc * Wc;
      c.so = 1; c.sd = 1; c.tsign = -1;
      c.pad = -((ph + d->pad - r0) / 2); c.pad_w = -((pw + d->pad - s0) / 2);
      c.wt0 = r0 * d->S + s0; c.wtr = 2 * d->S; c.wts = 2;
      c.y_strided = 1;
      c.y_base = (ph * d->W + pw) * d->C;
      c.y_img_pitch = d->H * d->W * d->C; c.y_row_pitch = 2 * d->W * d->C; c.y_pix_pitch = 2 * d->C;
      p.cp[p.nc] = plan_conv(c, ConvOut::bf16);
      if (p.cp[p.nc].n > 0 && p.cp[p.nc].l[0].family == FAM_GENERAL) {   // no gather-free kernel for this class
        p.nc = 0;
        break;
      }
      ++p.nc;
    }
    if (p.nc > 0) {
      p.form = DgradForm::parity;
      p.fill = k1;
      return p;
    }
  }
  p.conv = plan_conv(a, out);
  return p;
}

extern "C" int asm_conv2d_dgrad(const asm_conv_desc* d, const void* dy, const void* wt, const void* addend,
                                void* dx, void* stream) {
  return dgrad_impl(d, dy, wt, addend, nullptr, dx, stream);
}

extern "C" int asm_conv2d_dgrad_masked(const asm_conv_desc* d, const void* dy, const void* wt, const void* addend,
                                       const uint8_t* addend_mask, void* dx, void* stream) {
  ASM_REQUIRE(addend && addend_mask, "conv dgrad_masked: needs the addend and its mask");
  ASM_REQUIRE(d && d->C % 8 == 0, "conv dgrad_masked: C must be a multiple of 8");
  return dgrad_impl(d, dy, wt, addend, addend_mask, dx, stream);
}

extern "C" int asm_conv2d_dgrad_pooled(const asm_conv_desc* d, const void* dy, const void* wt, const void* addend,
                                       const uint8_t* addend_mask, const void* pool_dy, int pool_k, int pool_stride,
                                       int pool_pad, int pool_Ho, int pool_Wo, int count_valid, void* dx, void* stream) {
  ASM_REQUIRE(d && pool_dy, "conv dgrad_pooled: null pointer");
  ASM_REQUIRE(d->R == 1 && d->S == 1 && d->stride == 1 && d->pad == 0 && d->C % 8 == 0,
              "conv dgrad_pooled: needs a 1x1 stride-1 convolution with C %% 8 == 0");
  ASM_REQUIRE(pool_k >= 1 && (pool_stride == 1 || pool_stride == 2) && pool_pad >= 0 && pool_Ho > 0 && pool_Wo > 0,
              "conv dgrad_pooled: bad pooling geometry");
  if (pool_k > 2 * pool_stride || pool_k < pool_stride)
    ASM_FAIL(ASM_ENOTSUP, "conv dgrad_pooled: window %d / stride %d puts a pixel in more than two windows per dimension",
             pool_k, pool_stride);
  ASM_REQUIRE(!addend_mask || addend, "conv dgrad_pooled: a mask needs its addend");
  const PoolAdd pa = {pool_dy, pool_k, pool_stride, pool_pad, pool_Ho, pool_Wo, count_valid ? 1 : 0};
  return dgrad_impl(d, dy, wt, addend, addend_mask, dx, stream, &pa);
}

// does asm_conv2d_dgrad_bnred cover this layer?  1x1 / stride 1 / no padding and 3x3 / stride 1 / pad 1 layers whose plan has
// the batch-norm backward sums in every launch (all 1x1 kernels have them; of the 3x3 ones igemm8 and igemm3)
static bool dgrad_bnred_covers(const asm_conv_desc* d) {
  if (!d || d->C % 8 || d->K % 8 || d->stride != 1 || d->x_img_pitch || d->x_row_pitch || d->x_pix_pitch || d->out_f32) return false;
  if (!(d->R == 1 && d->S == 1 && d->pad == 0) && !(d->R == 3 && d->S == 3 && d->pad == 1 && d->Ho == d->H && d->Wo == d->W))
    return false;
  const ConvPlan p = plan_conv(dgrad_args(d), ConvOut::bnred);
  for (int i = 0; i < p.n; ++i)
    if (p.l[i].epi != EPI_BNRED) return false;
  return p.n > 0;
}

// partial rows of asm_conv2d_dgrad_bnred for this layer; 0: the layer is not one it covers
extern "C" int asm_conv2d_dgrad_bnred_blocks(const asm_conv_desc* d) {
  if (!d) return ASM_EINVAL;
  if (!dgrad_bnred_covers(d)) return 0;
  return cdiv(d->N * d->H * d->W, STATS_BM);
}

extern "C" int asm_conv2d_dgrad_bnred(const asm_conv_desc* d, const void* dy, const void* wt, const void* addend,
                                      const uint8_t* addend_mask, const void* bn_y, const uint8_t* bn_relu_mask,
                                      float* partial, void* dx, void* stream) {
  ASM_REQUIRE(d && bn_y && partial, "conv dgrad_bnred: null pointer");
  ASM_REQUIRE(!addend_mask || addend, "conv dgrad_bnred: a mask needs its addend");
  if (!dgrad_bnred_covers(d))
    ASM_FAIL(ASM_ENOTSUP, "conv dgrad_bnred: 1x1 stride-1 layers, and the 3x3 stride-1 layers of the igemm8 / igemm3 kernels, with "
             "C %% 8 == 0 only (%dx%d, stride %d, C %d)", d->R, d->S, d->stride, d->C);
  const BnRed r = {bn_y, bn_relu_mask, partial};
  return dgrad_impl(d, dy, wt, addend, addend_mask, dx, stream, nullptr, &r);
}

extern "C" int asm_conv2d_dgrad_kernel(const asm_conv_desc* d, int variant) {
  if (int e = dgrad_check(d)) return e;
  ASM_REQUIRE(!(variant & ~(ASM_DGRAD_MASKED | ASM_DGRAD_POOLED | ASM_DGRAD_BNRED)), "conv dgrad_kernel: bad variant %d", variant);
  const bool pooled = variant & ASM_DGRAD_POOLED, bnred = variant & ASM_DGRAD_BNRED;
  if (pooled && (bnred || d->R != 1 || d->S != 1 || d->stride != 1 || d->pad != 0))
    ASM_FAIL(ASM_ENOTSUP, "conv dgrad_kernel: the pooled input gradient is a 1x1 stride-1 one without the batch-norm sums");
  if (bnred && !dgrad_bnred_covers(d)) ASM_FAIL(ASM_ENOTSUP, "conv dgrad_kernel: no batch-norm sums for this layer");
  alignas(16) static const unsigned char operand[16] = {};   // stands in for the tensors: the plan asks only which are there
  IGemmArgs a = dgrad_args(d);
  if (variant & ASM_DGRAD_MASKED) {
    a.addend = operand;
    a.addend_mask = operand;
  }
  if (pooled) a.pool_dy = operand;
  const DgradPlan p = plan_dgrad(d, a, bnred ? ConvOut::bnred : ConvOut::bf16, true);
  if (p.form == DgradForm::s2) return FAM_DGRAD_S2;
  const ConvPlan& last = p.form == DgradForm::parity ? p.cp[p.nc - 1] : p.conv;   // what asm_last_conv_kernel reports
  if (last.n == 0) ASM_FAIL(ASM_ENOTSUP, "%s", last.why);
  return last.l[last.n - 1].family;
}

static int dgrad_impl(const asm_conv_desc* d, const void* dy, const void* wt, const void* addend,
                      const uint8_t* addend_mask, void* dx, void* stream, const PoolAdd* pool, const BnRed* red) {
  if (int e = dgrad_check(d)) return e;
  ASM_REQUIRE(dy && wt && dx, "conv dgrad: null pointer");
  IGemmArgs a = dgrad_args(d);
  a.x = dy; a.w = wt; a.y = dx; a.addend = addend; a.addend_mask = addend_mask;
  if (red) {
    a.stats = red->partial; a.red_y = red->y; a.red_mask = red->mask;
  }
  if (pool) {
    a.pool_dy = pool->dy; a.pool_k = pool->k; a.pool_stride = pool->stride; a.pool_pad = pool->pad;
    a.pool_Hp = pool->Hp; a.pool_Wp = pool->Wp; a.pool_cv = pool->cv; a.pool_H = d->H;
  }
  const bool aligned = ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(wt) | reinterpret_cast<uintptr_t>(dx) |
                         reinterpret_cast<uintptr_t>(addend)) & 15) == 0;
  const DgradPlan p = plan_dgrad(d, a, red ? ConvOut::bnred : ConvOut::bf16, aligned);
  const hipStream_t st = (hipStream_t)stream;
  switch (p.form) {
    case DgradForm::s2:
      if (const int rc = asm_dgrad_s2_launch(d, dy, wt, addend, addend_mask, dx, stream)) return rc;
      asm_last_conv_kernel = FAM_DGRAD_S2;
      return ASM_OK;
    case DgradForm::parity:
      if (p.fill) {   // the classes the one launch does not write are zero, or just the addend
        const size_t bytes = (size_t)a.M * d->C * 2;
        hipError_t e = (addend && addend != dx) ? asm_fill_async(dx, addend, 0, bytes, st)
                     : addend ? hipSuccess
                              : asm_fill_async(dx, nullptr, 0, bytes, st);
        if (e != hipSuccess) ASM_FAIL(ASM_EHIP, "conv dgrad: fill: %s", hipGetErrorString(e));
      }
      for (int i = 0; i < p.nc; ++i)
        if (const int rc = run_plan(p.cp[i], p.cls[i], st)) return rc;
      return ASM_OK;
    case DgradForm::conv: break;
  }
  return run_plan(p.conv, a, st);
}
