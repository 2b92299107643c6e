// AutoAugment on the device: the two ops of one sub-policy applied to every image of a batch in ONE launch.
// Reference: preprocessing/autoaugment.py:316-679 (the op bodies), :682-699 (NAME_TO_FUNC: the op ids 1..16 are its names
// in that order), applied between _resize_image and the mean subtraction (preprocessing/imagenet_preprocessing.py:280-289)
// on clip(image, 0, 255) cast to uint8.  All randomness (sub-policy, whether a slot fires, signs, cutout centre) and all
// transcendental math (the rotation matrix) is resolved on the host into the descriptor; see include/asm_hip.h.
//
// One workgroup per image.  The image lives as uint8 in one of two workspace planes (150 KB at 224 x 224: L2-resident);
// a slot is a statistics phase where the op needs one (AutoContrast: per-channel min / max; Equalize: per-channel 256-bin
// integer histogram in LDS, then the LUT by a 256-wide scan) followed by a map phase.  Point ops work in place; Sharpness
// and the geometric ops read neighbours / arbitrary pixels and go out of place to the other plane.  Phases are separated
// by __syncthreads(): an image never leaves its workgroup, so no output bit depends on the rest of the batch or on timing
// (the only atomics are integer LDS add / min / max, which commute exactly).  One code path serves every size.
// Float arithmetic is float32 without fused multiply-add, in the order written, so tests/autoaugment_ref.py matches it
// bit for bit.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AA_THREADS = 1024;
enum {
  AA_NONE = 0, AA_AUTOCONTRAST, AA_EQUALIZE, AA_INVERT, AA_ROTATE, AA_POSTERIZE, AA_SOLARIZE, AA_SOLARIZE_ADD, AA_COLOR,
  AA_CONTRAST, AA_BRIGHTNESS, AA_SHARPNESS, AA_SHEAR_X, AA_SHEAR_Y, AA_TRANSLATE_X, AA_TRANSLATE_Y, AA_CUTOUT
};
constexpr int AA_REPLACE = 128;   // replace_value of build_and_apply_nas_policy (:836), all three channels

__device__ __forceinline__ float clip255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }

// blend (:334-356): factor 0 -> image1, 1 -> image2, inside (0, 1) truncate without clipping, else clip then truncate
__device__ __forceinline__ int blend_u8(int i1, int i2, float factor) {
  if (factor == 0.f) return i1;
  if (factor == 1.f) return i2;
  const float a = (float)i1, b = (float)i2;
  const float difference = b - a;
  const float scaled = factor * difference;
  const float temp = a + scaled;
  if (factor > 0.f && factor < 1.f) return (int)temp & 255;
  return (int)clip255(temp);
}

// tf.image.rgb_to_grayscale on uint8: * (1/255), weighted sum in channel order, * 255.5, truncate
__device__ __forceinline__ int gray_u8(int r, int g, int b) {
  const float k = 1.0f / 255.0f;
  const float fr = (float)r * k, fg = (float)g * k, fb = (float)b * k;
  float s = fr * 0.2989f;
  s = s + fg * 0.5870f;
  s = s + fb * 0.1140f;
  return (int)(s * 255.5f);
}

struct Lds {
  int hist[768];   // Equalize: per-channel histogram, then the LUT
  int scan[768];
  int stat[8];     // AutoContrast: lo[3], hi[3]; Equalize: highest non-empty bin[3]
};

__device__ void autocontrast(uint8_t* img, int HW, Lds& l) {   // :521-557
  const int tid = threadIdx.x;
  if (tid < 3) { l.stat[tid] = 255; l.stat[3 + tid] = 0; }
  __syncthreads();
  int lo[3] = {255, 255, 255}, hi[3] = {0, 0, 0};
  for (int p = tid; p < HW; p += AA_THREADS)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int v = img[(size_t)p * 3 + c];
      lo[c] = min(lo[c], v);
      hi[c] = max(hi[c], v);
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    atomicMin(&l.stat[c], lo[c]);
    atomicMax(&l.stat[3 + c], hi[c]);
  }
  __syncthreads();
  float scale[3], offset[3];
  bool on[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float flo = (float)l.stat[c], fhi = (float)l.stat[3 + c];
    on[c] = fhi > flo;
    scale[c] = on[c] ? 255.0f / (fhi - flo) : 1.f;
    offset[c] = -flo * scale[c];
  }
  for (int p = tid; p < HW; p += AA_THREADS)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (on[c]) {
        const float v = (float)img[(size_t)p * 3 + c] * scale[c] + offset[c];
        img[(size_t)p * 3 + c] = (uint8_t)(int)clip255(v);
      }
  __syncthreads();
}

__device__ void equalize(uint8_t* img, int HW, Lds& l) {   // :589-627
  const int tid = threadIdx.x;
  if (tid < 768) l.hist[tid] = 0;
  if (tid < 3) l.stat[tid] = 0;
  __syncthreads();
  for (int p = tid; p < HW; p += AA_THREADS)
#pragma unroll
    for (int c = 0; c < 3; ++c) atomicAdd(&l.hist[c * 256 + img[(size_t)p * 3 + c]], 1);
  __syncthreads();
  const int c = tid >> 8, v = tid & 255;
  int mine = 0;
  if (tid < 768) {
    mine = l.hist[tid];
    l.scan[tid] = mine;
    if (mine != 0) atomicMax(&l.stat[c], v);
  }
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {   // inclusive scan of each channel's 256 bins
    int add = 0;
    if (tid < 768 && v >= off) add = l.scan[tid - off];
    __syncthreads();
    if (tid < 768) l.scan[tid] += add;
    __syncthreads();
  }
  int lut = v;
  if (tid < 768) {
    // step from the non-zero bins: (their sum - the last of them) // 255; zero -> the channel is returned unchanged
    const int step = (HW - l.hist[c * 256 + l.stat[c]]) / 255;
    if (step != 0) lut = v == 0 ? 0 : min(max((l.scan[tid - 1] + step / 2) / step, 0), 255);
  }
  __syncthreads();
  if (tid < 768) l.hist[tid] = lut;
  __syncthreads();
  for (int p = tid; p < HW; p += AA_THREADS)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) img[(size_t)p * 3 + ch] = (uint8_t)l.hist[ch * 256 + img[(size_t)p * 3 + ch]];
  __syncthreads();
}

// one value in, one value out, no coordinates: Invert, Posterize, Solarize, SolarizeAdd, Contrast, Brightness
__device__ void point_op(uint8_t* img, int HW, const asm_augment_op& o) {
  const int degenerate = (int)clip255((float)HW / 256.0f);   // contrast (:442-446): the pixel COUNT over 256
  for (int i = threadIdx.x; i < HW * 3; i += AA_THREADS) {
    const int v = img[i];
    int r = v;
    switch (o.op) {
      case AA_INVERT: r = 255 - v; break;
      case AA_POSTERIZE: r = o.a >= 8 ? 0 : ((v >> o.a) << o.a); break;      // a = 8 - bits; bits = 0 is defined as 0
      case AA_SOLARIZE: r = v < o.a ? v : 255 - v; break;                    // int compare: threshold 256 keeps all
      case AA_SOLARIZE_ADD: r = v < o.b ? min(max(v + o.a, 0), 255) : v; break;
      case AA_CONTRAST: r = blend_u8(degenerate, v, o.f[0]); break;
      case AA_BRIGHTNESS: r = blend_u8(0, v, o.f[0]); break;
    }
    img[i] = (uint8_t)r;
  }
  __syncthreads();
}

__device__ void color(uint8_t* img, int HW, float factor) {   // :427-430
  for (int p = threadIdx.x; p < HW; p += AA_THREADS) {
    uint8_t* px = img + (size_t)p * 3;
    const int r = px[0], g = px[1], b = px[2];
    const int gray = gray_u8(r, g, b);
    px[0] = (uint8_t)blend_u8(gray, r, factor);
    px[1] = (uint8_t)blend_u8(gray, g, factor);
    px[2] = (uint8_t)blend_u8(gray, b, factor);
  }
  __syncthreads();
}

__device__ void cutout(uint8_t* img, int H, int W, int pad, int cy, int cx) {   // :359-407
  const int y0 = max(0, cy - pad), y1 = min(H, cy + pad), x0 = max(0, cx - pad), x1 = min(W, cx + pad);
  for (int p = threadIdx.x; p < H * W; p += AA_THREADS) {
    const int y = p / W, x = p - y * W;
    if (y >= y0 && y < y1 && x >= x0 && x < x1) {
      uint8_t* px = img + (size_t)p * 3;
      px[0] = px[1] = px[2] = AA_REPLACE;
    }
  }
  __syncthreads();
}

__device__ void sharpness(const uint8_t* src, uint8_t* dst, int H, int W, float factor) {   // :560-586
  const float w1 = 1.0f / 13.0f, w5 = 5.0f / 13.0f;
  for (int p = threadIdx.x; p < H * W; p += AA_THREADS) {
    const int y = p / W, x = p - y * W;
    const bool inner = y >= 1 && y <= H - 2 && x >= 1 && x <= W - 2;   // the border ring keeps the original
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int orig = src[(size_t)p * 3 + c];
      int deg = orig;
      if (inner) {
        float acc = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {   // nine taps, row-major
            const float t = (float)src[((size_t)(y + dy) * W + (x + dx)) * 3 + c];
            acc = acc + t * ((dy == 0 && dx == 0) ? w5 : w1);
          }
        deg = (int)clip255(acc);
      }
      dst[(size_t)p * 3 + c] = (uint8_t)blend_u8(deg, orig, factor);
    }
  }
  __syncthreads();
}

// tf.contrib.image.transform, NEAREST: output (x, y) reads input (round(a0 x + a1 y + a2), round(b0 x + b1 y + b2)),
// half away from zero; a sample outside the image is `replace` after unwrap (:644-679)
__device__ void affine(const uint8_t* src, uint8_t* dst, int H, int W, const float* f) {
  for (int p = threadIdx.x; p < H * W; p += AA_THREADS) {
    const int y = p / W, x = p - y * W;
    const float fx = (float)x, fy = (float)y;
    const float sx = roundf(f[0] * fx + f[1] * fy + f[2]);
    const float sy = roundf(f[3] * fx + f[4] * fy + f[5]);
    uint8_t* px = dst + (size_t)p * 3;
    if (sx >= 0.f && sx < (float)W && sy >= 0.f && sy < (float)H) {   // false for NaN: never an out-of-range read
      const uint8_t* q = src + ((size_t)(int)sy * W + (int)sx) * 3;
      px[0] = q[0]; px[1] = q[1]; px[2] = q[2];
    } else {
      px[0] = px[1] = px[2] = AA_REPLACE;
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(AA_THREADS)
autoaugment_kernel(const float* __restrict__ in, const asm_augment_desc* __restrict__ descs, int H, int W, int subtract_mean,
                   float* __restrict__ out, uint8_t* ws, long long plane) {
  __shared__ Lds lds;
  const int n = blockIdx.x, tid = threadIdx.x, HW = H * W;
  const float* src = in + (size_t)n * HW * 3;
  uint8_t* cur = ws + (size_t)n * 2 * plane;
  uint8_t* alt = cur + plane;
  // imagenet_preprocessing.py:284-286: clip_by_value(image, 0, 255), cast to uint8 (truncation)
  for (int i = tid; i < HW * 3; i += AA_THREADS) cur[i] = (uint8_t)(int)clip255(src[i]);
  __syncthreads();
  for (int s = 0; s < 2; ++s) {
    const asm_augment_op o = descs[n].slot[s];   // the same for every thread of the workgroup: barriers below are uniform
    bool swapped = false;
    switch (o.op) {
      case AA_AUTOCONTRAST: autocontrast(cur, HW, lds); break;
      case AA_EQUALIZE: equalize(cur, HW, lds); break;
      case AA_POSTERIZE:
        if (o.a >= 0 && o.a <= 8) point_op(cur, HW, o);
        break;
      case AA_SOLARIZE:
        if (o.a >= 0 && o.a <= 256) point_op(cur, HW, o);
        break;
      case AA_SOLARIZE_ADD:
        if (o.a >= -255 && o.a <= 255 && o.b >= 0 && o.b <= 256) point_op(cur, HW, o);
        break;
      case AA_INVERT:
      case AA_CONTRAST:
      case AA_BRIGHTNESS: point_op(cur, HW, o); break;
      case AA_COLOR: color(cur, HW, o.f[0]); break;
      case AA_SHARPNESS: sharpness(cur, alt, H, W, o.f[0]); swapped = true; break;
      case AA_ROTATE:
      case AA_SHEAR_X:
      case AA_SHEAR_Y:
      case AA_TRANSLATE_X:
      case AA_TRANSLATE_Y: affine(cur, alt, H, W, o.f); swapped = true; break;
      case AA_CUTOUT:
        if (o.a >= 0 && o.b >= 0) cutout(cur, H, W, min(o.a, 1 << 15), o.b >> 16, o.b & 0xffff);
        break;
      default: break;   // 0 = not applied; anything unknown leaves the image unchanged (the host mirror raises)
    }
    if (swapped) { uint8_t* t = cur; cur = alt; alt = t; }
  }
  const float means[3] = ASM_CHANNEL_MEANS;
  float* dst = out + (size_t)n * HW * 3;
  for (int p = tid; p < HW; p += AA_THREADS)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = (float)cur[(size_t)p * 3 + c];
      if (subtract_mean) v = v - means[c];
      dst[(size_t)p * 3 + c] = v;
    }
}

long long aa_plane_bytes(int H, int W) { return ((long long)H * W * 3 + 255) / 256 * 256; }

}  // namespace

extern "C" int asm_autoaugment_workspace_bytes(int N, int H, int W, int64_t* bytes) {
  ASM_REQUIRE(bytes, "autoaugment_workspace_bytes: null pointer");
  ASM_REQUIRE(N >= 0 && H > 0 && W > 0 && H <= 32767 && W <= 32767 && (long long)H * W < (1ll << 24),
              "autoaugment: bad sizes (H, W <= 32767, H * W < 2^24)");
  *bytes = (int64_t)N * 2 * aa_plane_bytes(H, W);
  return ASM_OK;
}

extern "C" int asm_autoaugment(const float* in, const asm_augment_desc* descs, int N, int H, int W, int subtract_mean,
                               float* out, void* workspace, int64_t workspace_bytes, void* stream) {
  ASM_REQUIRE(N >= 0 && H > 0 && W > 0 && H <= 32767 && W <= 32767 && (long long)H * W < (1ll << 24),
              "autoaugment: bad sizes (H, W <= 32767, H * W < 2^24)");
  if (N == 0) return ASM_OK;
  ASM_REQUIRE(in && descs && out && workspace, "autoaugment: null pointer");
  const long long plane = aa_plane_bytes(H, W);
  ASM_REQUIRE(workspace_bytes >= (int64_t)N * 2 * plane, "autoaugment: workspace too small (asm_autoaugment_workspace_bytes)");
  ASM_LAUNCH(autoaugment_kernel, dim3(N), dim3(AA_THREADS), 0, (hipStream_t)stream, in, descs, H, W, subtract_mean ? 1 : 0, out,
             (uint8_t*)workspace, plane);
  ASM_CHECK_LAUNCH("autoaugment");
  return ASM_OK;
}
