// Classifier tails of the evaluations.  asm_eval_rows / asm_eval_accumulate: the per-row metrics and the running state of the
// classification run loop (nets/run_loop_classification.py:208-219, metric/ece_metric.py:171-298).  asm_eval_groups: the
// grouped tail of the corruption-robustness evaluation (mce/eval_robustness.py:186-226): per row the arg-max class, the top-1
// hit and the in_top_k(k=5) hit, added into the int32 counters of the row's group in the same launch.
#include "common.h"

namespace {

constexpr int kNoArg = 0x7fffffff;    // "no non-NaN logit seen yet"
constexpr int kRows = 4;              // rows (= waves) per workgroup

// running arg-max over the non-NaN values, visited in increasing index order: strictly larger replaces, so the lowest index
// of equal maxima stays (tf.nn.top_k / tf.argmax); `higher` counts the values strictly above the label's logit
__device__ __forceinline__ void take(float v, int c, float zl, float& mx, int& arg, int& higher) {
  if (v == v && (arg == kNoArg || v > mx)) {
    mx = v;
    arg = c;
  }
  higher += v > zl ? 1 : 0;
}
// the better of the partial result (mx, arg) and another one (ov, oa): the larger value, the lower index of equal ones; a side
// that has seen no non-NaN logit never wins
__device__ __forceinline__ void merge(float ov, int oa, float& mx, int& arg) {
  if (oa != kNoArg && (arg == kNoArg || ov > mx || (ov == mx && oa < arg))) {
    mx = ov;
    arg = oa;
  }
}

// One 256-thread block per row: arg-max, max softmax probability, top-1 hit, in_top_k(k=5) hit.  A second sweep sums the
// softmax's denominator.  A row without a non-NaN logit keeps arg = kNoArg.
__global__ __launch_bounds__(256) void eval_rows_kernel(const float* __restrict__ logits, int ld,
                                                        const int32_t* __restrict__ labels, int C,
                                                        int32_t* __restrict__ pred, float* __restrict__ conf,
                                                        float* __restrict__ top1, float* __restrict__ top5) {
  __shared__ float shv[4];
  __shared__ int shi[4];
  __shared__ float sh[4];
  const int b = blockIdx.x;
  const float* z = logits + (size_t)b * ld;
  const int lab = labels[b];
  // a label outside [0, C) can never be hit (tf.nn.in_top_k yields False for an out-of-range target): no stray read
  const bool lab_ok = (unsigned)lab < (unsigned)C;
  const float zl = lab_ok ? z[lab] : INFINITY;
  float mx = -INFINITY;
  int arg = kNoArg, higher = 0;
  for (int c = threadIdx.x; c < C; c += 256) take(z[c], c, zl, mx, arg, higher);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) merge(__shfl_xor(mx, o, 64), __shfl_xor(arg, o, 64), mx, arg);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    shv[w] = mx;
    shi[w] = arg;
  }
  __syncthreads();
  mx = shv[0];
  arg = shi[0];
  for (int i = 1; i < 4; ++i) merge(shv[i], shi[i], mx, arg);
  float se = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) se += __expf(z[c] - mx);
  se = block_reduce(se, false, sh);
  const float above = block_reduce((float)higher, false, sh);   // a count: exact in float32
  if (threadIdx.x == 0) {
    pred[b] = arg;
    conf[b] = 1.0f / se;                      // max of softmax
    top1[b] = arg == lab ? 1.f : 0.f;
    top5[b] = (lab_ok && above < 5.f) ? 1.f : 0.f;   // in the top k unless k others are strictly larger
  }
}
// state[0..2] = sum top1, sum top5, count ; state[3..12] correct per bin, [13..22] conf per bin, [23..32] count per bin
__global__ __launch_bounds__(64) void eval_accumulate_kernel(const float* __restrict__ conf,
                                                             const float* __restrict__ top1,
                                                             const float* __restrict__ top5, int B,
                                                             float* __restrict__ state) {
  const int t = threadIdx.x;
  if (t < 3) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += (t == 0) ? top1[b] : (t == 1 ? top5[b] : 1.f);
    state[t] += s;
  } else if (t < 13) {  // ECE bin t-3: (lo, hi] with the reference's epsilon-widened outer edges
    const int bin = t - 3;
    const float eps = 1e-7f;
    const float lo = bin == 0 ? -eps : (float)bin / 10.f;
    const float hi = bin == 9 ? 1.f + eps : (float)(bin + 1) / 10.f;
    float cor = 0.f, cs = 0.f, cnt = 0.f;
    for (int b = 0; b < B; ++b) {
      const float c = conf[b];
      if (c > lo && c <= hi) {
        cor += top1[b];
        cs += c;
        cnt += 1.f;
      }
    }
    state[3 + bin] += cor;
    state[13 + bin] += cs;
    state[23 + bin] += cnt;
  }
}

// One wave per row, four rows per workgroup.  The row is read once: the label's logit is one broadcast load in front of the
// sweep, so max, arg and the strictly-larger count share the sweep.  kVec: 16-byte loads (ld % 4 == 0 and a 16-byte aligned
// base, so every row starts on 16 bytes); the last partial quad of a row and the other case are scalar loads.  Columns
// C .. ld-1 are never read.  The four rows' outcomes meet in LDS and one lane adds them, rows of one group as one add per
// counter: an evaluation walks its files severity by severity, so a whole batch usually lands on three addresses, and one
// atomic per row was 2.7 x (B = 1024) to 8.8 x (B = 65536) the time of the same rows spread over 95 groups
// (profiles/robustness.md).
template <bool kVec>
__global__ __launch_bounds__(64 * kRows) void eval_groups_kernel(const float* __restrict__ logits, int ld,
                                                                 const int32_t* __restrict__ labels,
                                                                 const int32_t* __restrict__ groups, int B, int C, int G,
                                                                 int32_t* __restrict__ counts, int32_t* __restrict__ pred) {
  __shared__ int sh_group[kRows], sh_hits[kRows];       // counter row of the wave's image (-1: no image); bit 0 top-1, bit 1 top-5
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * kRows + w;
  int row = -1, hits = 0;
  if (b < B) {                                          // wave-uniform
    const float* z = logits + (size_t)b * ld;
    const int lab = labels[b];
    const bool lab_ok = (unsigned)lab < (unsigned)C;    // a label outside [0, C) is never read and never hit
    const float zl = lab_ok ? z[lab] : INFINITY;
    float mx = -INFINITY;
    int arg = kNoArg, higher = 0;
    if (kVec) {
      for (int c = lane * 4; c < C; c += 256) {
        if (c + 4 <= C) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(z + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) take(v[e], c + e, zl, mx, arg, higher);
        } else {
          for (int e = c; e < C; ++e) take(z[e], e, zl, mx, arg, higher);
        }
      }
    } else {
      for (int c = lane; c < C; c += 64) take(z[c], c, zl, mx, arg, higher);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(mx, o, 64);
      const int oa = __shfl_xor(arg, o, 64);
      higher += __shfl_xor(higher, o, 64);
      merge(ov, oa, mx, arg);
    }
    const int p = arg == kNoArg ? -1 : arg;             // a row of NaNs predicts nothing
    if (lane == 0 && pred) pred[b] = p;
    const int g = groups[b];
    if ((unsigned)g >= (unsigned)G) {                    // a stray group id: an image of row G, never a hit
      row = G;
    } else {
      row = g;
      // tf.nn.in_top_k: false for a non-finite target, true unless k others are strictly larger
      hits = (lab_ok && p == lab ? 1 : 0) | (lab_ok && fabsf(zl) < INFINITY && higher < 5 ? 2 : 0);
    }
  }
  if (lane == 0) {
    sh_group[w] = row;
    sh_hits[w] = hits;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    const int gi = sh_group[i];
    if (gi < 0) continue;
    int n = 0, h1 = 0, h5 = 0;
#pragma unroll
    for (int j = i; j < kRows; ++j)                     // this image and the later ones of its group
      if (sh_group[j] == gi) {
        n += 1;
        h1 += sh_hits[j] & 1;
        h5 += sh_hits[j] >> 1;
        sh_group[j] = -1;
      }
    int32_t* dst = counts + (size_t)gi * 3;
    atomicAdd(dst, n);
    if (h1) atomicAdd(dst + 1, h1);
    if (h5) atomicAdd(dst + 2, h5);
  }
}

}  // namespace

extern "C" int asm_eval_rows(const float* logits, int ld, const int32_t* labels, int B, int C, int32_t* pred,
                             float* conf, float* top1, float* top5, void* stream) {
  ASM_REQUIRE(logits && labels && pred && conf && top1 && top5 && B > 0 && C > 0 && ld >= C, "eval_rows: bad arguments");
  return asm_launch_checked<eval_rows_kernel>("eval_rows", B, 256, (hipStream_t)stream, logits, ld, labels, C, pred, conf,
                                              top1, top5);
}
extern "C" int asm_eval_accumulate(const float* conf, const float* top1, const float* top5, int B, float* state33,
                                   void* stream) {
  ASM_REQUIRE(conf && top1 && top5 && state33 && B > 0, "eval_accumulate: bad arguments");
  return asm_launch_checked<eval_accumulate_kernel>("eval_accumulate", 1, 64, (hipStream_t)stream, conf, top1, top5, B,
                                                    state33);
}

extern "C" int asm_eval_groups(const float* logits, int ld, const int32_t* labels, const int32_t* groups, int B, int C,
                               int G, int32_t* counts, int32_t* pred, void* stream) {
  ASM_REQUIRE(logits && labels && groups && counts && B > 0 && C > 0 && G > 0 && ld >= C,
              "eval_groups: bad arguments (B=%d C=%d G=%d ld=%d)", B, C, G, ld);
  const bool vec = ld % 4 == 0 && ((uintptr_t)logits & 15) == 0;
  const dim3 grid((unsigned)((B - 1) / kRows + 1)), block(64 * kRows);
  if (vec)
    return asm_launch_checked<eval_groups_kernel<true>>("eval_groups", grid, block, (hipStream_t)stream, logits, ld, labels,
                                                        groups, B, C, G, counts, pred);
  return asm_launch_checked<eval_groups_kernel<false>>("eval_groups", grid, block, (hipStream_t)stream, logits, ld, labels,
                                                       groups, B, C, G, counts, pred);
}
