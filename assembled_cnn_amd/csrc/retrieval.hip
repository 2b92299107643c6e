// Recall@K retrieval evaluation (metric/recall_metric.py): similarity of every query embedding with every index embedding and
// the K most similar index rows per query, WITHOUT the similarity matrix ever reaching memory.
//
//   reference (:98-110)    sim = l2_normalize(q) . l2_normalize(x)^T   or   -(|q|^2 + |x|^2 - 2 q.x)      [Q, N] fp32, stored
//                          top_k(sim, k = max(k_list) + 1, sorted=True)                                     reads it again
//   here                   retrieval_topk_kernel: one MFMA GEMM whose epilogue keeps a sorted list of K (value, index) pairs per
//                          query row; it moves O((Q + N) D) bytes where the reference moves O(Q N)
//                          retrieval_topk_wide_kernel (64 < K <= 1024): the same GEMM and epilogue (retrieval_walk), whose
//                          survivors go unsorted into a per-query candidate buffer that a radix select cuts back to K
//                          topk_merge_kernel / topk_merge_wide_kernel: the lists or buffers of a query's splits -> its K best
//
// Shared by the two selections: the walk (retrieval_walk, tile_row), the sorted insertion (list_insert: lists in LDS, the merge's
// output row), the radix select (radix_select: one wave over registers in WideSel::compact, a workgroup over memory in
// topk_merge_wide_kernel) and, on the host, the plan of a call (RetrievalPlan), the workspace bound and the launcher.
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
// Splits.  The index range is cut into S contiguous runs of tiles (RetrievalPlan: a pure function of the sizes) so that a small
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
constexpr int TOPK_MAX = 64;                // lists are insertion-sorted: past this the wide selection below
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
  int B;                // wide selection only: capacity of a (query, run) candidate buffer
  unsigned long long* counters;   // wide selection, test builds of the call only (else null): {survivors appended,
                                  // compactions during the walk, compactions at the end of a run}
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

// accumulator element acc[a][i] of a lane in half lhi of its wave -> index row of the tile (the 32 x 32 x 16 MFMA's layout)
__device__ __forceinline__ int tile_row(int a, int i, int lhi) { return a * 32 + (i & 3) + 8 * (i >> 2) + 4 * lhi; }

// The walk both selection kernels share: the 128 x 128 x 64 GEMM over this workgroup's run of index tiles and the scale
// epilogue.  At the end of every index tile a lane holds the 64 similarities of its query in acc (acc[a][i]: index row
// nb + tile_row(a, i, lhi)) and the bit mask `cand` (bit a*16 + i) of those that reach sel.threshold(row); sel.insert takes them.
// One instantiation per selection scheme, so every similarity is the same bits whichever scheme looks at it.
template <class Sel>
__device__ __forceinline__ void retrieval_walk(const TopkArgs& p, unsigned char* smem, Sel& sel) {
  unsigned char* qs = smem;
  unsigned char* xs = smem + BM * PITCH;
  float* xn = reinterpret_cast<float*>(smem + (BM + BN) * PITCH);     // per index row of the tile: |x|^2 or rsqrt(max(|x|^2, eps))

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int q0 = blockIdx.x * BM;
  const int split = blockIdx.y;
  const int t0 = split * p.tiles_per_split;
  const int t1 = min(p.n_tiles, t0 + p.tiles_per_split);
  const int ksteps = (p.D + BK - 1) / BK;

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
    __syncthreads();                          // the previous step's fragment reads (and the selection's initialisation) are done
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
    // ---- epilogue of one index tile: acc[a][i] is (query l31, index row tile_row(a, i, lhi)) ----
    const int nb = tile * BN;
    const float thr = sel.threshold(row);
    unsigned long long cand = 0ull;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int nl = tile_row(a, i, lhi);
        const float xv = xn[nl];
        const float sv = p.sim == 0 ? (acc[a][i] * qn) * xv : -((qn + xv) - 2.0f * acc[a][i]);
        acc[a][i] = sv;
        if (nb + nl < p.N && sv >= thr) cand |= 1ull << (a * 16 + i);
      }
    sel.insert(acc, cand, nb, row, lhi);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][i] = 0.f;
    kc = 0;
    ++tile;
  }
}

// acc[b >> 4][b & 15]: registers cannot be indexed, a select chain can
__device__ __forceinline__ float pick(const f32x16 (&acc)[4], int b) {
  float sv = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int i = 0; i < 16; ++i) sv = b == a * 16 + i ? acc[a][i] : sv;
  return sv;
}

// (sv, n) into the sorted list of K entries whose entry j is v[j * STRIDE], ix[j * STRIDE] and whose last entry is (thr, thi):
// false, and nothing done, unless it is strictly better than that one; else the entries it beats move down one place, the last
// one drops out, and (thr, thi) is the new last entry.  Inlined: the list kernel's list is in LDS, the merge's in memory.
template <int STRIDE>
__device__ __forceinline__ bool list_insert(float* v, int* ix, int K, float sv, int n, float& thr, int& thi) {
  if (!better(sv, n, thr, thi)) return false;
  int j = K - 1;
  while (j > 0) {
    const float pv = v[(j - 1) * STRIDE];
    const int pi = ix[(j - 1) * STRIDE];
    if (!better(sv, n, pv, pi)) break;
    v[j * STRIDE] = pv;
    ix[j * STRIDE] = pi;
    --j;
  }
  v[j * STRIDE] = sv;
  ix[j * STRIDE] = n;
  thr = v[(K - 1) * STRIDE];
  thi = ix[(K - 1) * STRIDE];
  return true;
}

// K <= 64: a sorted list per query, [K][BM] in LDS, whose K-th entry is the threshold
struct ListSel {
  float* lv;
  int* li;
  int K;
  __device__ __forceinline__ float threshold(int row) const { return lv[(K - 1) * BM + row]; }   // written by this wave before the barriers of the step
  // the two lanes of a query insert in turn; a lane re-reads the threshold its partner may have raised
  __device__ __forceinline__ void insert(const f32x16 (&acc)[4], unsigned long long cand, int nb, int row, int lhi) {
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      if (lhi == half && cand != 0ull) {
        float thr = lv[(K - 1) * BM + row];
        int thi = li[(K - 1) * BM + row];
        unsigned long long left = cand;
        while (left != 0ull) {                 // ascending index order; rare once the list is warm
          const int b = __builtin_ctzll(left);
          left &= left - 1ull;
          list_insert<BM>(lv + row, li + row, K, pick(acc, b), nb + tile_row(b >> 4, b & 15, lhi), thr, thi);
        }
      }
      __syncthreads();
    }
  }
};

__global__ __launch_bounds__(256, 2) void retrieval_topk_kernel(TopkArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* lv = reinterpret_cast<float*>(smem + (BM + BN) * PITCH) + BN;      // [K][BM] list values, behind the tiles and the |x|^2 row
  int* li = reinterpret_cast<int*>(lv + p.K * BM);                          // [K][BM] list indices (local to this index)
  const int tid = threadIdx.x, K = p.K;
  for (int i = tid; i < K * BM; i += 256) {
    lv[i] = -INFINITY;
    li[i] = EMPTY;
  }
  ListSel sel{lv, li, K};
  retrieval_walk(p, smem, sel);
  __syncthreads();
  const int q0 = blockIdx.x * BM, split = blockIdx.y;
  if (tid < BM && q0 + tid < p.Q) {
    const size_t o = ((size_t)(q0 + tid) * p.S + split) * K;
    for (int j = 0; j < K; ++j) {
      const int n = li[j * BM + tid];
      p.out_val[o + j] = lv[j * BM + tid];
      p.out_idx[o + j] = n == EMPTY ? -1 : n + p.index_base;
    }
  }
}

// ---- wide selection (64 < K <= 1024; legal from K = 1) -------------------------------------------------------------------------
// A (value, index) pair is ranked by one 64-bit key, larger = better: the value's bits mapped so that unsigned order is float
// order (-0 counts as +0, as the float compare of the list path has it) above the complement of the index, so of equal values
// the lower index wins.  Keys of distinct index rows are distinct: the K best are one set, whatever order they arrived in.
// Key 0 is an unused slot (index -1).
typedef unsigned long long u64;
constexpr int WIDE_MAX = 1024;
constexpr int WIDE_ROOM_MIN = 256, WIDE_ROOM_MAX = 448;   // room above K in a candidate buffer: K itself, within these bounds (the
                                                          // trigger sits BN below the capacity, so BN of it is never filled)
constexpr int WIDE_NCH = 23;                  // 64-key register chunks that hold the largest buffer: wide_capacity(WIDE_MAX) / 64
constexpr int WIDE_TARGET = 256;              // workgroups wanted: one per CU, the buffers of two would not meet the workspace bound

inline int wide_capacity(int K) {             // B: K + its room, whole 64-key chunks; non-decreasing in K
  int room = K < WIDE_ROOM_MIN ? WIDE_ROOM_MIN : K;
  if (room > WIDE_ROOM_MAX) room = WIDE_ROOM_MAX;
  return (K + room + 63) / 64 * 64;
}
static_assert(WIDE_NCH * 64 == (WIDE_MAX + WIDE_ROOM_MAX + 63) / 64 * 64, "the register copy of a buffer holds the largest one");

__device__ __forceinline__ u64 make_key(float v, int idx) {
  if (idx < 0) return 0ull;
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
  return ((u64)u << 32) | (unsigned)~idx;
}
__device__ __forceinline__ float key_value(u64 k) {
  const unsigned u = (unsigned)(k >> 32);
  return __uint_as_float((u >> 31) ? u ^ 0x80000000u : ~u);
}
__device__ __forceinline__ int key_index(u64 k) { return (int)~(unsigned)k; }

__device__ __forceinline__ void wave_sync() {             // LDS traffic between the lanes of one wave
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One step of a radix select, by one whole wave: hist holds the counts of 256 digit values; the digit d in which the need-th
// largest element lies (1 <= need <= sum of hist), how many elements have a larger digit, and how many have d itself.
__device__ __forceinline__ void select_digit(const unsigned* hist, int need, int lane, int& d, int& above, int& binc) {
  unsigned c[4], s = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c[j] = hist[255 - (4 * lane + j)];        // lanes walk the digits downwards
    s += c[j];
  }
  unsigned incl = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  unsigned run = incl - s;
  int fd = -1, fa = 0, fb = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (fd < 0 && run < (unsigned)need && (unsigned)need <= run + c[j]) {
      fd = 255 - (4 * lane + j);
      fa = (int)run;
      fb = (int)c[j];
    }
    run += c[j];
  }
  const u64 found = __ballot(fd >= 0);
  const int src = found ? __builtin_ctzll(found) : 0;
  d = max(__shfl(fd, src), 0);
  above = __shfl(fa, src);
  binc = __shfl(fb, src);
}

// Who runs a radix select together: how these threads clear the 256 counts they share, the barrier between two phases, and
// how the digit select_digit picks reaches every one of them (pick ends behind a barrier: hist may be cleared again).
struct WaveScope {                            // one wave, hist in LDS
  unsigned* hist; int lane;
  __device__ __forceinline__ void clear() const {
#pragma unroll
    for (int j = 0; j < 4; ++j) hist[lane + 64 * j] = 0u;
  }
  __device__ __forceinline__ void sync() const { wave_sync(); }
  __device__ __forceinline__ void pick(int need, int& d, int& above, int& binc) const {
    select_digit(hist, need, lane, d, above, binc);       // every lane gets the result
    wave_sync();
  }
};
struct GroupScope {                           // a workgroup of 256 threads, hist and the three picked numbers in LDS
  unsigned* hist; int* picked; int tid;
  __device__ __forceinline__ void clear() const { hist[tid] = 0u; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ void pick(int need, int& d, int& above, int& binc) const {
    if (tid < 64) {
      select_digit(hist, need, tid, d, above, binc);
      if (tid == 0) { picked[0] = d; picked[1] = above; picked[2] = binc; }
    }
    __syncthreads();
    d = picked[0]; above = picked[1]; binc = picked[2];
  }
};

// The radix select over 64-bit keys, 8-bit digits from the top: the prefix (low bits zero) at or above which the need best keys
// lie, 1 <= need <= number of keys.  each_key(add) calls add(k) for every key of this thread that takes part, once per pass.
// It stops as soon as a whole digit bin is taken: every key >= prefix is then one of the need best.
template <class Scope, class EachKey>
__device__ __forceinline__ u64 radix_select(const Scope& sc, int need, EachKey each_key) {
  u64 prefix = 0ull;
#pragma unroll 1
  for (int shift = 56;; shift -= 8) {
    sc.clear();
    sc.sync();
    const u64 mask = shift == 56 ? 0ull : ~0ull << (shift + 8);
    each_key([&](u64 k) {
      if ((k & mask) == prefix) atomicAdd(&sc.hist[(unsigned)(k >> shift) & 255u], 1u);
    });
    sc.sync();
    int d, above, binc;
    sc.pick(need, d, above, binc);
    prefix |= (u64)d << shift;
    need -= above;
    if (need == binc || shift == 0) return prefix;
  }
}

// K <= 1024: per (query, run) an unsorted buffer of B candidates in the workspace, the count and the threshold in registers
struct WideSel {
  float* wv;            // this wave's first query, this run: row r of the wave is at r * rstride
  int* wi;
  unsigned* hist;       // this wave's 256 digit counts in LDS
  size_t rstride;       // S * B
  int K, B, index_base, l31;
  unsigned long long* counters;
  bool valid;           // this lane's query exists
  float thr;            // a lower bound of the K-th best value of this lane's query so far
  int cnt;              // entries in its buffer (the two lanes of a query agree)

  __device__ __forceinline__ float threshold(int) const { return thr; }

  // The wave keeps the K best of the n > K entries of row r's buffer, in place, and returns the new threshold.  The buffer is
  // read once into registers; every digit pass counts from there.
  __device__ float compact(int r, int n) {
    float* v = wv + (size_t)r * rstride;
    int* ix = wi + (size_t)r * rstride;
    const int lane = threadIdx.x & 63;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the appends of this wave's other lanes: one CU, one vector cache --
                                                             // a wider scope would write the L2 back at every compaction
    u64 key[WIDE_NCH];
#pragma unroll
    for (int c = 0; c < WIDE_NCH; ++c) {
      const int e = c * 64 + lane;
      key[c] = 0ull;
      if (c * 64 < n && e < n) key[c] = make_key(v[e], ix[e]);
    }
    const u64 prefix = radix_select(WaveScope{hist, lane}, K, [&](auto add) {   // the n > K used slots; an unused one is no key
#pragma unroll
      for (int c = 0; c < WIDE_NCH; ++c)
        if (c * 64 < n && key[c] != 0ull) add(key[c]);
    });
    int out = 0;
#pragma unroll
    for (int c = 0; c < WIDE_NCH; ++c)
      if (c * 64 < n) {
        const bool keep = key[c] != 0ull && key[c] >= prefix;
        const u64 b = __ballot(keep);
        const int pos = out + __popcll(b & ((1ull << lane) - 1ull));
        if (keep && pos < B) {
          v[pos] = key_value(key[c]);
          ix[pos] = key_index(key[c]);
        }
        out += __popcll(b);
      }
    const float t = key_value(prefix);        // the low bits of an early exit are zero: at or below every kept value
    return t != t ? -INFINITY : t;
  }

  __device__ __forceinline__ void insert(const f32x16 (&acc)[4], unsigned long long cand, int nb, int row, int lhi) {
    if (!valid) cand = 0ull;
    const int c = __popcll(cand), cp = __shfl_xor(c, 32);
    if (counters && c) atomicAdd(counters, (unsigned long long)c);
    int pos = cnt + (lhi ? cp : 0);           // the low lane's survivors first: no turn-taking, the order never shows
    float* v = wv + (size_t)l31 * rstride;
    int* ix = wi + (size_t)l31 * rstride;
    while (cand != 0ull) {
      const int b = __builtin_ctzll(cand);
      cand &= cand - 1ull;
      const float sv = pick(acc, b);
      const int n = nb + tile_row(b >> 4, b & 15, lhi);
      if (pos < B) {                         // always: a tile adds at most BN to a count of at most B - BN
        v[pos] = sv;
        ix[pos] = n + index_base;
      }
      ++pos;
    }
    cnt += c + cp;
    // a query whose buffer could overflow on the next tile is compacted now, by the whole wave; the other waves wait at the step barrier
    u64 full = __ballot(cnt > B - BN) & 0xffffffffull;
    while (full != 0ull) {
      const int r = __builtin_ctzll(full);
      full &= full - 1ull;
      const float t = compact(r, __shfl(cnt, r));
      if (counters && (threadIdx.x & 63) == 0) atomicAdd(counters + 1, 1ull);
      if (l31 == r) {
        cnt = K;
        thr = t;
      }
    }
  }
};

// one workgroup per CU (WIDE_TARGET): no second one to leave registers for
__global__ __launch_bounds__(256) void retrieval_topk_wide_kernel(TopkArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qw = blockIdx.x * BM + wave * 32;                // the wave's first query
  const size_t o = ((size_t)qw * p.S + blockIdx.y) * p.B;
  WideSel sel;
  sel.wv = p.out_val + o;
  sel.wi = p.out_idx + o;
  sel.hist = reinterpret_cast<unsigned*>(smem + (BM + BN) * PITCH + BN * 4) + wave * 256;
  sel.rstride = (size_t)p.S * p.B;
  sel.K = p.K; sel.B = p.B; sel.index_base = p.index_base; sel.l31 = lane & 31;
  sel.counters = p.counters;
  sel.valid = qw + sel.l31 < p.Q;
  sel.thr = -INFINITY;
  sel.cnt = 0;
  retrieval_walk(p, smem, sel);
  // what the run leaves: at most K entries per query, the rest of the first K slots unused
  const int nvalid = min(32, p.Q - qw);
#pragma unroll 1
  for (int r = 0; r < 32; ++r) {
    int n = __shfl(sel.cnt, r);
    if (r >= nvalid) break;
    if (n > p.K) {
      sel.compact(r, n);
      if (p.counters && lane == 0) atomicAdd(p.counters + 2, 1ull);
      n = p.K;
    }
    for (int e = n + lane; e < p.K; e += 64) {
      sel.wv[(size_t)r * sel.rstride + e] = -INFINITY;
      sel.wi[(size_t)r * sel.rstride + e] = -1;
    }
  }
}

// The K best of P lists per row, sorted: one workgroup per row.  List l of row r holds K entries from (r * P + l) * stride on, in
// any order, index -1 = unused.  A radix select over the keys finds the K-th best, the keys at or above it are gathered into LDS
// (slots by atomic counter: the bitonic sort that follows removes the order they landed in) and sorted.
__global__ __launch_bounds__(256) void topk_merge_wide_kernel(const float* __restrict__ in_val, const int* __restrict__ in_idx, int P,
                                                              int K, size_t stride, float* __restrict__ out_val,
                                                              int* __restrict__ out_idx) {
  __shared__ unsigned hist[256];
  __shared__ u64 keys[WIDE_MAX];
  __shared__ int picked[3], nsel;
  const int tid = threadIdx.x;
  const size_t r = blockIdx.x;
  const float* iv = in_val + r * P * stride;
  const int* ii = in_idx + r * P * stride;
  // all P * K >= K slots, unused ones (key 0) counted: the K-th may be an unused one
  const u64 prefix = radix_select(GroupScope{hist, picked, tid}, K, [&](auto add) {
    for (int l = 0; l < P; ++l)
      for (int j = tid; j < K; j += 256) add(make_key(iv[l * stride + j], ii[l * stride + j]));
  });
  int n2 = 2;
  while (n2 < K) n2 <<= 1;
  for (int j = tid; j < n2; j += 256) keys[j] = 0ull;
  if (tid == 0) nsel = 0;
  __syncthreads();
  for (int l = 0; l < P; ++l)
    for (int j = tid; j < K; j += 256) {
      const u64 k = make_key(iv[l * stride + j], ii[l * stride + j]);
      if (k != 0ull && k >= prefix) {
        const int s = atomicAdd(&nsel, 1);
        if (s < n2) keys[s] = k;              // always, for lists of distinct index rows
      }
    }
  __syncthreads();
  for (int k2 = 2; k2 <= n2; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += 256) {
        const int x = i ^ j;
        if (x > i) {
          const u64 a = keys[i], b = keys[x];
          if ((i & k2) == 0 ? a < b : a > b) {
            keys[i] = b;
            keys[x] = a;
          }
        }
      }
      __syncthreads();
    }
  for (int j = tid; j < K; j += 256) {
    const u64 k = keys[j];
    out_val[r * K + j] = k ? key_value(k) : -INFINITY;
    out_idx[r * K + j] = k ? key_index(k) : -1;
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
      const int n = ii[e];
      if (n < 0 || !list_insert<1>(ov, oi, K, iv[e], n, thr, thi)) break;     // the list is sorted: what follows is no better
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

// Everything the two selections decide differently on the host, and the split plan of one call: a pure function of
// (Q, N, K, wide).  For sizes no call may have (one not positive, K above the cap) only name and cap are filled, to refuse with.
struct RetrievalPlan {
  const char* name;     // the entry point's, in messages
  int cap, target;      // largest K; workgroups wanted
  int B;                // wide selection: capacity of a (query, split) candidate buffer; else 0
  int lds;              // dynamic LDS of the selection kernel: tiles, |x|^2 row and the lists / the four waves' digit counts
  int entries;          // (value, index) pairs per (query, split) in the workspace: K or B
  int S, tiles_per_split, n_tiles;
};
inline RetrievalPlan retrieval_plan(int Q, int N, int K, bool wide) {
  RetrievalPlan p = wide ? RetrievalPlan{"retrieval_topk_wide", WIDE_MAX, WIDE_TARGET}
                         : RetrievalPlan{"retrieval_topk", TOPK_MAX, SPLIT_TARGET};      // the other members: 0
  if (Q <= 0 || N <= 0 || K <= 0 || K > p.cap) return p;
  p.B = wide ? wide_capacity(K) : 0;
  p.entries = wide ? p.B : K;
  p.lds = (BM + BN) * PITCH + BN * 4 + (wide ? 4 * 256 * 4 : K * BM * 8);
  p.n_tiles = cdiv(N, BN);
  int S = cdiv(p.target, cdiv(Q, BM));         // the splits of one query tile that make `target` workgroups
  if (S > SPLIT_MAX) S = SPLIT_MAX;
  if (S > p.n_tiles) S = p.n_tiles;
  p.tiles_per_split = cdiv(p.n_tiles, S);
  p.S = cdiv(p.n_tiles, p.tiles_per_split);    // no empty split
  return p;
}

// An upper bound of the plan's Q * S * entries * 8 that grows with each of Q, N, entries, so that a workspace sized for the
// largest call holds every smaller one; the plan's own product does not, S itself shrinks as Q grows
inline size_t retrieval_workspace_bound(int Q, int N, size_t target, size_t entries) {
  const size_t qt = cdivz((size_t)Q, BM), nt = cdivz((size_t)N, BN);
  size_t lists = qt * nt;                      // S <= nt, and qt * S <= target + qt, and S <= SPLIT_MAX
  if (lists > target + qt) lists = target + qt;
  if (lists > SPLIT_MAX * qt) lists = SPLIT_MAX * qt;
  return lists * BM * entries * 8;
}

}  // namespace

extern "C" size_t asm_retrieval_topk_workspace_bytes(int Q, int N, int K) {
  return Q <= 0 || N <= 0 || K <= 0 ? 0 : retrieval_workspace_bound(Q, N, SPLIT_TARGET, K);
}

extern "C" size_t asm_retrieval_topk_wide_workspace_bytes(int Q, int N, int K) {
  return Q <= 0 || N <= 0 || K <= 0 ? 0 : retrieval_workspace_bound(Q, N, WIDE_TARGET, wide_capacity(K));
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

extern "C" int asm_topk_merge_wide(const float* in_val, const int32_t* in_idx, int rows, int P, int K, float* out_val,
                                   int32_t* out_idx, void* stream) {
  ASM_REQUIRE(in_val && in_idx && out_val && out_idx && rows > 0 && P > 0 && K > 0,
              "topk_merge_wide: bad arguments (rows=%d P=%d K=%d)", rows, P, K);
  ASM_REQUIRE((const void*)in_val != (const void*)out_val && (const void*)in_idx != (const void*)out_idx,
              "topk_merge_wide: the output must not alias the input");
  if (K > WIDE_MAX) ASM_FAIL(ASM_ENOTSUP, "topk_merge_wide: K = %d is above the cap of %d", K, WIDE_MAX);
  ASM_LAUNCH(topk_merge_wide_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, in_val, in_idx, P, K, (size_t)K, out_val,
             out_idx);
  ASM_CHECK_LAUNCH("topk_merge_wide");
  return ASM_OK;
}

// The launcher of both selections: the checks, the plan, the selection kernel and the merge of its S lists per query
static int retrieval_launch(const void* queries, int ldq, const void* index, int ldi, const float* sq_queries,
                            const float* sq_index, int Q, int N, int D, int similarity, int K, int index_base, float* top_val,
                            int32_t* top_idx, void* workspace, size_t workspace_bytes, void* stream, bool wide,
                            unsigned long long* counters) {
  const RetrievalPlan pl = retrieval_plan(Q, N, K, wide);
  ASM_REQUIRE(queries && index && sq_queries && sq_index && top_val && top_idx, "%s: null operand", pl.name);
  ASM_REQUIRE(Q > 0 && N > 0 && D > 0 && K > 0, "%s: sizes must be positive (Q=%d N=%d D=%d K=%d)", pl.name, Q, N, D, K);
  ASM_REQUIRE(ldq >= D && ldi >= D && ldq % 8 == 0 && ldi % 8 == 0,
              "%s: rows must be 16-byte multiples of at least D channels (ldq=%d ldi=%d D=%d)", pl.name, ldq, ldi, D);
  ASM_REQUIRE(index_base >= 0 && (long long)index_base + N <= 0x7fffffffLL, "%s: index_base + N exceeds int32", pl.name);
  if (similarity != 0 && similarity != 1) ASM_FAIL(ASM_ENOTSUP, "%s: similarity %d (0 cosine, 1 euclidean)", pl.name, similarity);
  if (K > pl.cap) ASM_FAIL(ASM_ENOTSUP, "%s: K = %d is above the cap of %d", pl.name, K, pl.cap);
  const size_t need = retrieval_workspace_bound(Q, N, pl.target, pl.entries);
  ASM_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", pl.name, workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  float* ws_val = (float*)workspace;           // [Q][S][entries] values, then as many indices
  int* ws_idx = (int*)workspace + (size_t)Q * pl.S * pl.entries;
  const bool direct = !wide && pl.S == 1;      // one split of sorted lists: its list IS the result
  TopkArgs a;
  a.q = (const bf16_t*)queries; a.x = (const bf16_t*)index; a.sqq = sq_queries; a.sqx = sq_index;
  a.out_val = direct ? top_val : ws_val; a.out_idx = direct ? top_idx : ws_idx;
  a.Q = Q; a.N = N; a.D = D; a.ldq = ldq; a.ldi = ldi; a.K = K; a.sim = similarity; a.index_base = index_base;
  a.S = pl.S; a.tiles_per_split = pl.tiles_per_split; a.n_tiles = pl.n_tiles; a.B = pl.B;
  a.counters = counters;
  const dim3 grid(cdiv(Q, BM), pl.S);
  const int rc = wide ? asm_launch_dyn_lds<retrieval_topk_wide_kernel>(pl.name, grid, dim3(256), pl.lds, st, a)
                      : asm_launch_dyn_lds<retrieval_topk_kernel>(pl.name, grid, dim3(256), pl.lds, st, a);
  if (rc != ASM_OK || direct) return rc;
  if (wide)
    ASM_LAUNCH(topk_merge_wide_kernel, dim3(Q), dim3(256), 0, st, ws_val, ws_idx, pl.S, K, (size_t)pl.B, top_val, top_idx);
  else
    ASM_LAUNCH(topk_merge_kernel, dim3(cdiv(Q, 256)), dim3(256), 0, st, ws_val, ws_idx, Q, pl.S, K, top_val, top_idx);
  ASM_CHECK_LAUNCH(pl.name);
  return ASM_OK;
}

extern "C" int asm_retrieval_topk(const void* queries, int ldq, const void* index, int ldi, const float* sq_queries,
                                  const float* sq_index, int Q, int N, int D, int similarity, int K, int index_base,
                                  float* top_val, int32_t* top_idx, void* workspace, size_t workspace_bytes, void* stream) {
  return retrieval_launch(queries, ldq, index, ldi, sq_queries, sq_index, Q, N, D, similarity, K, index_base, top_val, top_idx,
                          workspace, workspace_bytes, stream, false, nullptr);
}

extern "C" int asm_retrieval_topk_wide(const void* queries, int ldq, const void* index, int ldi, const float* sq_queries,
                                       const float* sq_index, int Q, int N, int D, int similarity, int K, int index_base,
                                       float* top_val, int32_t* top_idx, void* workspace, size_t workspace_bytes, void* stream) {
  return retrieval_launch(queries, ldq, index, ldi, sq_queries, sq_index, Q, N, D, similarity, K, index_base, top_val, top_idx,
                          workspace, workspace_bytes, stream, true, nullptr);
}

// test-only (asm_hip_debug.h): the same call, adding to three device counters
extern "C" int asm_debug_retrieval_topk_wide_counted(const void* queries, int ldq, const void* index, int ldi,
                                                     const float* sq_queries, const float* sq_index, int Q, int N, int D,
                                                     int similarity, int K, int index_base, float* top_val, int32_t* top_idx,
                                                     void* workspace, size_t workspace_bytes, void* stream,
                                                     unsigned long long* counters3) {
  ASM_REQUIRE(counters3, "retrieval_topk_wide_counted: null counters");
  return retrieval_launch(queries, ldq, index, ldi, sq_queries, sq_index, Q, N, D, similarity, K, index_base, top_val, top_idx,
                          workspace, workspace_bytes, stream, true, counters3);
}

// test-only (asm_hip_debug.h): the RetrievalPlan the launcher would act on; nothing is launched
extern "C" int asm_debug_retrieval_plan(int Q, int N, int K, int wide, int32_t plan[4]) {
  const RetrievalPlan pl = retrieval_plan(Q, N, K, wide != 0);
  ASM_REQUIRE(plan && Q > 0 && N > 0 && K > 0, "retrieval_plan: bad arguments (Q=%d N=%d K=%d)", Q, N, K);
  if (K > pl.cap) ASM_FAIL(ASM_ENOTSUP, "retrieval_plan: K = %d is above the cap of %d", K, pl.cap);
  plan[0] = pl.S; plan[1] = pl.tiles_per_split; plan[2] = pl.n_tiles; plan[3] = pl.B;
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
