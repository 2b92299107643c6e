// Recall@K retrieval evaluation (metric/recall_metric.py): similarity of every query embedding with every index embedding and
// the K most similar index rows per query, WITHOUT the similarity matrix ever reaching memory.
//
//   reference (:98-110)    sim = l2_normalize(q) . l2_normalize(x)^T   or   -(|q|^2 + |x|^2 - 2 q.x)      [Q, N] fp32, stored
//                          top_k(sim, k = max(k_list) + 1, sorted=True)                                     reads it again
//   here                   retrieval_topk_kernel: one MFMA GEMM whose epilogue keeps a sorted list of K (value, index) pairs per
//                          query row; it moves O((Q + N) D) bytes where the reference moves O(Q N)
//
// Tiling.  A workgroup of four waves owns 128 query rows (wave w: rows 32 w .. 32 w + 31) and walks a contiguous range of
// 128-row index tiles in ascending order.  Per 64-channel step both tiles go global -> registers -> LDS (the next step's loads
// are in flight under this step's MFMAs), and every wave multiplies its 32 queries (B operand: the query is the LANE, l & 31)
// with the 128 index rows (A operand: four 32 x 32 x 16 bf16 MFMA tiles, the index row is the accumulator REGISTER).  So a lane
// sees 64 similarities of ONE query per tile, and that query's state -- the list, [K][128] in LDS, and its K-th entry, the
// threshold, in a register -- belongs to one wave.  Once the list is warm a tile costs one compare per element; the few
// survivors are inserted by the two lanes of a query in turn.
//
// Order.  A list is ordered by (value descending, index ascending) and an entry is inserted only where it is strictly better
// in that order, which is tf.nn.top_k's "of equal values the lower index first" whatever order the candidates arrive in.
//
// Splits.  The index range is cut into S contiguous runs of tiles (retrieval_splits: a pure function of Q, N) so that a small
// Q still fills the chip; every (query tile, split) writes its list to the workspace and topk_merge_kernel combines the S
// lists of a row in the same order.  Nothing depends on timing: the result is identical from run to run.
//
// Accuracy.  The dot products accumulate the RAW bf16 embeddings in fp32 on the matrix pipe; the normalisation is applied to
// the accumulator in fp32 (acc * rsqrt(max(|q|^2, 1e-12)) * rsqrt(max(|x|^2, 1e-12)), tf.nn.l2_normalize's epsilon; or
// -(|q|^2 + |x|^2 - 2 acc)).  The model emits its embedding in bf16, so no operand is rounded a second time: at least as
// exact as the reference's fp16 placeholders with an fp16 normalise before the matmul (:72-73, :99-104).
#include "common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int PITCH = BK * 2 + 16;          // bytes per LDS tile row: the 16-byte pad spreads the ds_read_b128 row reads over the banks
constexpr int TOPK_MAX = 64;                // lists are insertion-sorted: past this a selection scheme of another kind is due
constexpr int SPLIT_MAX = 64, SPLIT_TARGET = 512;   // workgroups wanted (two per CU) / most splits of one query tile
constexpr int EMPTY = 0x7fffffff;           // index of an unused list slot while lists are being built (-1 once stored)

__device__ __forceinline__ bool better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

struct TopkArgs {
  const bf16_t* q;
  const bf16_t* x;
  const float* sqq;
  const float* sqx;
  float* out_val;       // [Q][S][K]
  int* out_idx;
  int Q, N, D, ldq, ldi, K, sim, index_base, S, tiles_per_split, n_tiles;
};

// 8 channels [e, e + 8) of one row; zero beyond the row count or D.  e % 8 == 0 and ld % 8 == 0 keep the 16 bytes inside the row
__device__ __forceinline__ u32x4 load_chunk(const bf16_t* base, int row, int nrows, int ld, int e, int D) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (row < nrows && e < D) {
    v = *reinterpret_cast<const u32x4*>(base + (size_t)row * ld + e);
    const int rem = D - e;
    if (rem < 8) {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const unsigned m = (2 * w < rem ? 0x0000ffffu : 0u) | (2 * w + 1 < rem ? 0xffff0000u : 0u);
        v[w] &= m;
      }
    }
  }
  return v;
}

__global__ __launch_bounds__(256, 2) void retrieval_topk_kernel(TopkArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* qs = smem;
  unsigned char* xs = smem + BM * PITCH;
  float* xn = reinterpret_cast<float*>(smem + (BM + BN) * PITCH);     // per index row of the tile: |x|^2 or rsqrt(max(|x|^2, eps))
  float* lv = xn + BN;                                                 // [K][BM] list values
  int* li = reinterpret_cast<int*>(lv + p.K * BM);                     // [K][BM] list indices (local to this index)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int K = p.K;
  const int q0 = blockIdx.x * BM;
  const int split = blockIdx.y;
  const int t0 = split * p.tiles_per_split;
  const int t1 = min(p.n_tiles, t0 + p.tiles_per_split);
  const int ksteps = (p.D + BK - 1) / BK;

  for (int i = tid; i < K * BM; i += 256) {
    lv[i] = -INFINITY;
    li[i] = EMPTY;
  }

  const int row = wave * 32 + l31;            // the query row of this lane inside the tile
  float qn = 0.f;
  if (q0 + row < p.Q) {
    const float s = p.sqq[q0 + row];
    qn = p.sim == 0 ? rsqrtf(fmaxf(s, 1e-12f)) : s;
  }

  const int chunk = tid & 7, r0 = tid >> 3;
  u32x4 gq[4], gx[4];
  auto gload = [&](int tile, int kc) {
    const int e = kc * BK + chunk * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      gq[j] = load_chunk(p.q, q0 + r0 + 32 * j, p.Q, p.ldq, e, p.D);
      gx[j] = load_chunk(p.x, tile * BN + r0 + 32 * j, p.N, p.ldi, e, p.D);
    }
  };

  f32x16 acc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[a][i] = 0.f;

  int tile = t0, kc = 0;
  if (t0 < t1) gload(t0, 0);
  const int total = (t1 - t0) * ksteps;
#pragma unroll 1
  for (int s = 0; s < total; ++s) {
    __syncthreads();                          // the previous step's fragment reads (and the list initialisation) are done
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      *reinterpret_cast<u32x4*>(qs + (r0 + 32 * j) * PITCH + chunk * 16) = gq[j];
      *reinterpret_cast<u32x4*>(xs + (r0 + 32 * j) * PITCH + chunk * 16) = gx[j];
    }
    if (kc == 0 && tid < BN) {
      const int n = tile * BN + tid;
      float v = 0.f;
      if (n < p.N) {
        v = p.sqx[n];
        if (p.sim == 0) v = rsqrtf(fmaxf(v, 1e-12f));
      }
      xn[tid] = v;
    }
    __syncthreads();
    if (s + 1 < total) {
      const bool wrap = kc + 1 == ksteps;
      gload(wrap ? tile + 1 : tile, wrap ? 0 : kc + 1);
    }
    const int kleft = p.D - kc * BK;          // channels of this step (> 0)
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      if (kk * 16 < kleft) {
        const int off = (kk * 2 + lhi) * 16;
        const bf16x8 fq = *reinterpret_cast<const bf16x8*>(qs + row * PITCH + off);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const bf16x8 fx = *reinterpret_cast<const bf16x8*>(xs + (a * 32 + l31) * PITCH + off);
          acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fx, fq, acc[a], 0, 0, 0);
        }
      }
    }
    if (kc + 1 < ksteps) {
      ++kc;
      continue;
    }
    // ---- epilogue of one index tile: acc[a][i] is (query l31, index row a*32 + (i&3) + 8*(i>>2) + 4*lhi) ----
    const int nb = tile * BN;
    float thr = lv[(K - 1) * BM + row];        // written by this wave before the barriers above
    unsigned long long cand = 0ull;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int nl = a * 32 + (i & 3) + 8 * (i >> 2) + 4 * lhi;
        const float xv = xn[nl];
        const float sv = p.sim == 0 ? (acc[a][i] * qn) * xv : -((qn + xv) - 2.0f * acc[a][i]);
        acc[a][i] = sv;
        if (nb + nl < p.N && sv >= thr) cand |= 1ull << (a * 16 + i);
      }
    // the two lanes of a query insert in turn; a lane re-reads the threshold its partner may have raised
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      if (lhi == half && cand != 0ull) {
        thr = lv[(K - 1) * BM + row];
        int thi = li[(K - 1) * BM + row];
        unsigned long long left = cand;
        while (left != 0ull) {                 // ascending index order; rare once the list is warm
          const int b = __builtin_ctzll(left);
          left &= left - 1ull;
          float sv = 0.f;                      // acc[b >> 4][b & 15]: registers cannot be indexed, a select chain can
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int i = 0; i < 16; ++i) sv = b == a * 16 + i ? acc[a][i] : sv;
          const int n = nb + (b >> 4) * 32 + (b & 3) + 8 * ((b & 15) >> 2) + 4 * lhi;
          if (better(sv, n, thr, thi)) {
            int j = K - 1;
            while (j > 0) {
              const float pv = lv[(j - 1) * BM + row];
              const int pi = li[(j - 1) * BM + row];
              if (!better(sv, n, pv, pi)) break;
              lv[j * BM + row] = pv;
              li[j * BM + row] = pi;
              --j;
            }
            lv[j * BM + row] = sv;
            li[j * BM + row] = n;
            thr = lv[(K - 1) * BM + row];
            thi = li[(K - 1) * BM + row];
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][i] = 0.f;
    kc = 0;
    ++tile;
  }
  __syncthreads();
  if (tid < BM && q0 + tid < p.Q) {
    const size_t o = ((size_t)(q0 + tid) * p.S + split) * K;
    for (int j = 0; j < K; ++j) {
      const int n = li[j * BM + tid];
      p.out_val[o + j] = lv[j * BM + tid];
      p.out_idx[o + j] = n == EMPTY ? -1 : n + p.index_base;
    }
  }
}

// P sorted lists of K per row -> one; one thread per row, the output row itself is the insertion-sorted list
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ in_val, const int* __restrict__ in_idx,
                                                         int rows, int P, int K, float* __restrict__ out_val,
                                                         int* __restrict__ out_idx) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  float* ov = out_val + (size_t)r * K;
  int* oi = out_idx + (size_t)r * K;
  for (int j = 0; j < K; ++j) {
    ov[j] = -INFINITY;
    oi[j] = EMPTY;
  }
  float thr = -INFINITY;
  int thi = EMPTY;
  for (int l = 0; l < P; ++l) {
    const float* iv = in_val + ((size_t)r * P + l) * K;
    const int* ii = in_idx + ((size_t)r * P + l) * K;
    for (int e = 0; e < K; ++e) {
      const float sv = iv[e];
      const int n = ii[e];
      if (n < 0 || !better(sv, n, thr, thi)) break;     // the list is sorted: what follows is no better
      int j = K - 1;
      while (j > 0 && better(sv, n, ov[j - 1], oi[j - 1])) {
        ov[j] = ov[j - 1];
        oi[j] = oi[j - 1];
        --j;
      }
      ov[j] = sv;
      oi[j] = n;
      thr = ov[K - 1];
      thi = oi[K - 1];
    }
  }
  for (int j = 0; j < K; ++j)
    if (oi[j] == EMPTY) oi[j] = -1;
}

// sq[n] = sum_d x[n][d]^2: one wave per row, lanes take 16-byte pieces, fixed summation order
__global__ __launch_bounds__(256) void embed_sqnorm_kernel(const bf16_t* __restrict__ x, int N, int D, int ld,
                                                           float* __restrict__ sq) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;
  float s = 0.f;
  for (int e = lane * 8; e < D; e += 512) {
    float f[8];
    unpack8(load_chunk(x, n, N, ld, e, D), f);
#pragma unroll
    for (int i = 0; i < 8; ++i) s += f[i] * f[i];
  }
  s = wave_sum(s);
  if (lane == 0) sq[n] = s;
}

// metric/recall_metric.py:217-228 for one query per thread; integer atomics: exact and order-independent
__global__ __launch_bounds__(256) void recall_accumulate_kernel(const int* __restrict__ top_idx, int Q, int K,
                                                                const int* __restrict__ qlab, const int* __restrict__ ilab,
                                                                int N, int query_base, const int* __restrict__ k_list, int nk,
                                                                int* __restrict__ hits) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  int first = 0x7fffffff;                      // position of the first entry with the query's label, self entries dropped
  if (r < Q) {
    const int qi = query_base + r, lab = qlab[r];
    int pos = 0;
    for (int j = 0; j < K; ++j) {
      const int n = top_idx[(size_t)r * K + j];
      if (n == qi) continue;                   // filter(lambda x: x != query_idx, top_k): compared with the position in the QUERY list
      if ((unsigned)n < (unsigned)N && ilab[n] == lab) {
        first = pos;
        break;
      }
      ++pos;
    }
  }
  for (int i = 0; i < nk; ++i) {
    const unsigned long long m = __ballot(first < k_list[i]);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(hits + i, (int)__popcll(m));
  }
}

inline int retrieval_splits(int Q, int N, int* tiles_per_split) {
  const int qt = cdiv(Q, BM), nt = cdiv(N, BN);
  int S = cdiv(SPLIT_TARGET, qt);
  if (S > SPLIT_MAX) S = SPLIT_MAX;
  if (S > nt) S = nt;
  const int tps = cdiv(nt, S);
  *tiles_per_split = tps;
  return cdiv(nt, tps);                        // no empty split
}

}  // namespace

// An upper bound of Q * S * K * 8 that grows with each of Q, N, K (S itself shrinks as Q grows)
extern "C" size_t asm_retrieval_topk_workspace_bytes(int Q, int N, int K) {
  if (Q <= 0 || N <= 0 || K <= 0) return 0;
  const size_t qt = cdivz((size_t)Q, BM), nt = cdivz((size_t)N, BN);
  size_t lists = qt * nt;                      // S <= nt, and qt * S <= SPLIT_TARGET + qt, and S <= SPLIT_MAX
  if (lists > SPLIT_TARGET + qt) lists = SPLIT_TARGET + qt;
  if (lists > SPLIT_MAX * qt) lists = SPLIT_MAX * qt;
  return lists * BM * (size_t)K * 8;
}

extern "C" int asm_embed_sqnorm(const void* x, int N, int D, int ld, float* sq, void* stream) {
  ASM_REQUIRE(x && sq && N > 0 && D > 0 && ld >= D && ld % 8 == 0, "embed_sqnorm: bad arguments (N=%d D=%d ld=%d)", N, D, ld);
  ASM_LAUNCH(embed_sqnorm_kernel, dim3(cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, N, D, ld, sq);
  ASM_CHECK_LAUNCH("embed_sqnorm");
  return ASM_OK;
}

extern "C" int asm_topk_merge(const float* in_val, const int32_t* in_idx, int rows, int P, int K, float* out_val,
                              int32_t* out_idx, void* stream) {
  ASM_REQUIRE(in_val && in_idx && out_val && out_idx && rows > 0 && P > 0 && K > 0,
              "topk_merge: bad arguments (rows=%d P=%d K=%d)", rows, P, K);
  ASM_REQUIRE((const void*)in_val != (const void*)out_val && (const void*)in_idx != (const void*)out_idx,
              "topk_merge: the output must not alias the input");
  if (K > TOPK_MAX) ASM_FAIL(ASM_ENOTSUP, "topk_merge: K = %d is above the cap of %d", K, TOPK_MAX);
  ASM_LAUNCH(topk_merge_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, (hipStream_t)stream, in_val, in_idx, rows, P, K, out_val,
             out_idx);
  ASM_CHECK_LAUNCH("topk_merge");
  return ASM_OK;
}

extern "C" int asm_retrieval_topk(const void* queries, int ldq, const void* index, int ldi, const float* sq_queries,
                                  const float* sq_index, int Q, int N, int D, int similarity, int K, int index_base,
                                  float* top_val, int32_t* top_idx, void* workspace, size_t workspace_bytes, void* stream) {
  ASM_REQUIRE(queries && index && sq_queries && sq_index && top_val && top_idx, "retrieval_topk: null operand");
  ASM_REQUIRE(Q > 0 && N > 0 && D > 0 && K > 0, "retrieval_topk: sizes must be positive (Q=%d N=%d D=%d K=%d)", Q, N, D, K);
  ASM_REQUIRE(ldq >= D && ldi >= D && ldq % 8 == 0 && ldi % 8 == 0,
              "retrieval_topk: rows must be 16-byte multiples of at least D channels (ldq=%d ldi=%d D=%d)", ldq, ldi, D);
  ASM_REQUIRE(index_base >= 0 && (long long)index_base + N <= 0x7fffffffLL, "retrieval_topk: index_base + N exceeds int32");
  if (similarity != 0 && similarity != 1)
    ASM_FAIL(ASM_ENOTSUP, "retrieval_topk: similarity %d (0 cosine, 1 euclidean)", similarity);
  if (K > TOPK_MAX) ASM_FAIL(ASM_ENOTSUP, "retrieval_topk: K = %d is above the cap of %d", K, TOPK_MAX);
  ASM_REQUIRE(workspace && workspace_bytes >= asm_retrieval_topk_workspace_bytes(Q, N, K),
              "retrieval_topk: workspace of %zu bytes, %zu needed", workspace_bytes, asm_retrieval_topk_workspace_bytes(Q, N, K));
  hipStream_t st = (hipStream_t)stream;
  TopkArgs a;
  a.q = (const bf16_t*)queries;
  a.x = (const bf16_t*)index;
  a.sqq = sq_queries;
  a.sqx = sq_index;
  a.Q = Q; a.N = N; a.D = D; a.ldq = ldq; a.ldi = ldi; a.K = K; a.sim = similarity; a.index_base = index_base;
  a.n_tiles = cdiv(N, BN);
  a.S = retrieval_splits(Q, N, &a.tiles_per_split);
  float* ws_val = (float*)workspace;
  int* ws_idx = (int*)workspace + (size_t)Q * a.S * K;
  a.out_val = a.S == 1 ? top_val : ws_val;     // one split: its list IS the result
  a.out_idx = a.S == 1 ? top_idx : ws_idx;
  const int lds = (BM + BN) * PITCH + BN * 4 + K * BM * 8;
  static bool attr_done[ASM_MAX_DEVICES] = {};
  if (hipError_t e = asm_ensure_dyn_lds(retrieval_topk_kernel, lds, attr_done); e != hipSuccess)
    ASM_FAIL(ASM_EHIP, "retrieval_topk: dynamic LDS opt-in: %s", hipGetErrorString(e));
  ASM_LAUNCH(retrieval_topk_kernel, dim3(cdiv(Q, BM), a.S), dim3(256), lds, st, a);
  if (a.S > 1)
    ASM_LAUNCH(topk_merge_kernel, dim3(cdiv(Q, 256)), dim3(256), 0, st, ws_val, ws_idx, Q, a.S, K, top_val, top_idx);
  ASM_CHECK_LAUNCH("retrieval_topk");
  return ASM_OK;
}

extern "C" int asm_recall_accumulate(const int32_t* top_idx, int Q, int K, const int32_t* query_labels,
                                     const int32_t* index_labels, int N, int query_base, const int32_t* k_list, int nk,
                                     int32_t* hits, void* stream) {
  ASM_REQUIRE(top_idx && query_labels && index_labels && k_list && hits && Q > 0 && K > 0 && N > 0 && nk > 0 && query_base >= 0,
              "recall_accumulate: bad arguments (Q=%d K=%d N=%d nk=%d query_base=%d)", Q, K, N, nk, query_base);
  ASM_LAUNCH(recall_accumulate_kernel, dim3(cdiv(Q, 256)), dim3(256), 0, (hipStream_t)stream, top_idx, Q, K, query_labels,
             index_labels, N, query_base, k_list, nk, hits);
  ASM_CHECK_LAUNCH("recall_accumulate");
  return ASM_OK;
}
