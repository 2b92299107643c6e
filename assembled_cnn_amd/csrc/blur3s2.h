// Blur-pool arithmetic shared by the pooling kernels (pool.hip) and the selective-kernel passes that fold the blur pool of a
// strided unit into themselves (sk_fused.hip): the binomial coefficients, the REFLECT index and the adjoint of the
// workload's case (3 taps, stride 2, even extents) for one input pixel.  Both users add the same terms in the same order,
// which is what keeps the folded passes bit-identical to the two-kernel chains.
#pragma once
#include "common.h"

struct BlurCoef {
  float a[8];  // normalised 1-D binomial; 2-D weight = a[r]*a[s] (exact: all factors are dyadic)
};
inline BlurCoef blur_coef(int k) {
  static const int tri[8][7] = {{0}, {1}, {1, 1}, {1, 2, 1}, {1, 3, 3, 1}, {1, 4, 6, 4, 1}, {1, 5, 10, 10, 5, 1},
                                {1, 6, 15, 20, 15, 6, 1}};
  BlurCoef c;
  int sum = 0;
  for (int i = 0; i < k; ++i) sum += tri[k][i];
  for (int i = 0; i < 8; ++i) c.a[i] = i < k ? (float)tri[k][i] / (float)sum : 0.f;
  return c;
}
__device__ __forceinline__ int reflect(int i, int L) {
  if (i < 0) i = -i;
  if (i >= L) i = 2 * (L - 1) - i;
  return i;
}

// 3 taps (a0 a1 a2), stride 2, even H and W: the input gradient of pixel (h, w) = (2i + u, 2j + v) draws on the 2 x 2
// neighbourhood g[a][b] = dy[i + a][j + b] only.  Per dimension (h = 2i + u):
//   u = 0: tap 1 of output i                                      -> a1 g[i]
//   u = 1: tap 0 of output i + 1 (if it exists), tap 2 of output i -> a0 g[i+1] + a2 g[i]
//          h = 1 is also what the REFLECT pad shows at padded position 0 (tap 0 of output 0) -> + a0 g[0]
// (the far-end reflection lands on tap positions no stride-2 output uses when the extent is even).  The terms are
// added in the generic gather's order (blur_bwd_kernel), so the result is the same bits.
// hv / wv: output i + 1 / j + 1 exists (g[1][.] / g[.][1] are read only then); h0 / w0: i == 0 / j == 0.
// get(a, b, t): the 8 channels of g[a][b] as floats (a, b are constants after unrolling: the caller may keep the four
// vectors packed and unpack the one a term uses).
template <class Get>
__device__ __forceinline__ void blur3s2_bwd_pixel(Get get, bool u, bool v, bool hv, bool wv, bool h0, bool w0, float a0,
                                                  float a1, float a2, float* acc) {
  const int src[3] = {1, 0, 0};
  const float wh[3] = {a0, u ? a2 : a1, a0}, ww[3] = {a0, v ? a2 : a1, a0};
  const bool okh[3] = {u && hv, true, u && h0}, okw[3] = {v && wv, true, v && w0};
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
  for (int th = 0; th < 3; ++th) {
    if (!okh[th]) continue;
#pragma unroll
    for (int tw = 0; tw < 3; ++tw) {
      if (!okw[tw]) continue;
      const float wgt = wh[th] * ww[tw];
      float t[8];
      get(src[th], src[tw], t);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += t[e] * wgt;
    }
  }
}
