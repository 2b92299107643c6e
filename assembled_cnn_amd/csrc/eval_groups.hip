// Grouped classifier tail of the corruption-robustness evaluation (mce/eval_robustness.py:186-226): per row the arg-max
// class, the top-1 hit and the in_top_k(k=5) hit, added into the int32 counters of the row's group in the same launch.
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
      if (oa != kNoArg && (arg == kNoArg || ov > mx || (ov == mx && oa < arg))) {
        mx = ov;
        arg = oa;
      }
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

extern "C" int asm_eval_groups(const float* logits, int ld, const int32_t* labels, const int32_t* groups, int B, int C,
                               int G, int32_t* counts, int32_t* pred, void* stream) {
  ASM_REQUIRE(logits && labels && groups && counts && B > 0 && C > 0 && G > 0 && ld >= C,
              "eval_groups: bad arguments (B=%d C=%d G=%d ld=%d)", B, C, G, ld);
  const bool vec = ld % 4 == 0 && ((uintptr_t)logits & 15) == 0;
  const dim3 grid((unsigned)((B - 1) / kRows + 1)), block(64 * kRows);
  if (vec)
    ASM_LAUNCH(eval_groups_kernel<true>, grid, block, 0, (hipStream_t)stream, logits, ld, labels, groups, B, C, G, counts,
               pred);
  else
    ASM_LAUNCH(eval_groups_kernel<false>, grid, block, 0, (hipStream_t)stream, logits, ld, labels, groups, B, C, G, counts,
               pred);
  ASM_CHECK_LAUNCH("eval_groups");
  return ASM_OK;
}
