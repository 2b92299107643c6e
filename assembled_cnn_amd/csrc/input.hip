// Input-pipeline tail on the GPU: crop window -> (flip) -> legacy-TF bilinear resize -> central-crop offset ->
// optional channel-mean subtraction, for a ragged batch of decoded uint8 images.
// Reference: preprocessing/imagenet_preprocessing.py:57-97 (crop + flip), :189-225 (_smallest_size_at_least,
// _aspect_preserving_resize, _resize_image = tf.image.resize_images(BILINEAR, align_corners=False)), :97-120
// (central_crop), :122-155 (mean_image_subtraction).  TF-1.14's resize has NO half-pixel centres:
// in = out_index * (in_size / out_size), lower = (int)in, upper = min(lower + 1, in_size - 1), lerp = in - lower,
// value = top + (bottom - top) * y_lerp with top = tl + (tr - tl) * x_lerp, all in float32, no fused multiply-add.
// HBM-bound byte work: one thread per output pixel, 12 source bytes gathered, 12 output bytes written.
// The same body serves the reference's other preprocessing types (asm_preprocess_window; utils/data_util.py:346-378):
// preprocessing/reid_preprocessing.py:489-540 and preprocessing/inception_preprocessing.py:117-144, :204-340 flip AFTER
// resize and crop -- not the same pixels, the resize above is not mirror-symmetric --, the Inception family converts to
// float32 in [0, 1] before it interpolates (tf.image.convert_image_dtype) and ends its training branch with a per-image
// colour offset and a clamp (distort_color_fast).
#include "common.h"

namespace {

// One body for both entry points.  kLegacy: asm_resize_crop_flip's descriptor rule (any non-zero flip mirrors the window
// before the resize); otherwise flip is one of ASM_FLIP_* and any other value counts as a window that does not fit.
// kUnit: the four taps are float(u8) * float32(1 / 255) (tf.image.convert_image_dtype) instead of float(u8).
// kTail: ASM_TAIL_*; `add` is read for ASM_TAIL_ADD_CLAMP only and may be null.
template <bool kLegacy, bool kUnit, int kTail>
__global__ void __launch_bounds__(256)
window_kernel(const uint8_t* __restrict__ src, long long src_bytes, const asm_image_desc* __restrict__ descs,
              int out_h, int out_w, const float* __restrict__ add, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= out_h * out_w) return;
  const asm_image_desc d = descs[n];
  const int i = p / out_w, j = p - i * out_w;
  float* o = out + ((size_t)n * out_h * out_w + p) * 3;
  // memory safety only (the host mirror validates and raises): a window outside the image or the buffer gives zeros
  const long long need = d.src_offset + (long long)d.Hs * d.Ws * 3;
  const bool ok = d.src_offset >= 0 && need <= src_bytes && d.crop_h > 0 && d.crop_w > 0 && d.crop_y >= 0 &&
                  d.crop_x >= 0 && d.crop_y + d.crop_h <= d.Hs && d.crop_x + d.crop_w <= d.Ws && d.resize_h > 0 &&
                  d.resize_w > 0 && d.out_y >= 0 && d.out_x >= 0 && d.out_y + out_h <= d.resize_h &&
                  d.out_x + out_w <= d.resize_w && (kLegacy || (d.flip >= ASM_FLIP_NONE && d.flip <= ASM_FLIP_AFTER));
  if (!ok) { o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; return; }
  const bool before = kLegacy ? d.flip != 0 : d.flip == ASM_FLIP_BEFORE;
  const int col = !kLegacy && d.flip == ASM_FLIP_AFTER ? out_w - 1 - j : j;     // column of the un-mirrored output
  const float hs = (float)d.crop_h / (float)d.resize_h;
  const float ws = (float)d.crop_w / (float)d.resize_w;
  const float in_y = (float)(d.out_y + i) * hs;
  const float in_x = (float)(d.out_x + col) * ws;
  const int ly = (int)in_y, lx = (int)in_x;
  const int uy = min(ly + 1, d.crop_h - 1), ux = min(lx + 1, d.crop_w - 1);
  const float fy = in_y - (float)ly, fx = in_x - (float)lx;
  const int cl = before ? d.crop_w - 1 - lx : lx;
  const int cu = before ? d.crop_w - 1 - ux : ux;
  const uint8_t* base = src + d.src_offset;
  const uint8_t* r0 = base + ((size_t)(d.crop_y + ly) * d.Ws + d.crop_x) * 3;
  const uint8_t* r1 = base + ((size_t)(d.crop_y + uy) * d.Ws + d.crop_x) * 3;
  const float means[3] = ASM_CHANNEL_MEANS;
  const float unit = (float)(1.0 / 255.0);
  // the per-image addend is read once, ahead of the pixel work: a load between the three stores keeps them from merging
  float plus[3] = {0.f, 0.f, 0.f};
  const bool adds = kTail == ASM_TAIL_ADD_CLAMP && add != nullptr;
  if (adds) { plus[0] = add[n * 3]; plus[1] = add[n * 3 + 1]; plus[2] = add[n * 3 + 2]; }
  float res[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float tl = (float)r0[cl * 3 + c], tr = (float)r0[cu * 3 + c];
    float bl = (float)r1[cl * 3 + c], br = (float)r1[cu * 3 + c];
    if (kUnit) { tl = tl * unit; tr = tr * unit; bl = bl * unit; br = br * unit; }
    const float top = tl + (tr - tl) * fx;
    const float bot = bl + (br - bl) * fx;
    float v = top + (bot - top) * fy;
    if (kTail == ASM_TAIL_MEANS) v = v - means[c];
    if (kTail == ASM_TAIL_ADD_CLAMP) {
      if (adds) v = v + plus[c];
      v = fminf(fmaxf(v, 0.f), 1.f);
    }
    res[c] = v;
  }
  o[0] = res[0]; o[1] = res[1]; o[2] = res[2];
}

template <bool kLegacy, bool kUnit, int kTail>
void launch_window(const uint8_t* src, int64_t src_bytes, const asm_image_desc* descs, int N, int out_h, int out_w,
                   const float* add, float* out, void* stream) {
  dim3 grid((out_h * out_w + 255) / 256, N);
  ASM_LAUNCH((window_kernel<kLegacy, kUnit, kTail>), grid, dim3(256), 0, (hipStream_t)stream, src, (long long)src_bytes,
             descs, out_h, out_w, add, out);
}

}  // namespace

extern "C" int asm_resize_crop_flip(const uint8_t* src, int64_t src_bytes, const asm_image_desc* descs, int N,
                                    int out_h, int out_w, int subtract_mean, float* out, void* stream) {
  ASM_REQUIRE(N >= 0 && out_h > 0 && out_w > 0 && src_bytes >= 0, "resize_crop_flip: bad sizes");
  ASM_REQUIRE((long long)out_h * out_w < (1ll << 30), "resize_crop_flip: output too large");
  if (N == 0) return ASM_OK;
  ASM_REQUIRE(src && descs && out, "resize_crop_flip: null pointer");
  if (subtract_mean) launch_window<true, false, ASM_TAIL_MEANS>(src, src_bytes, descs, N, out_h, out_w, nullptr, out, stream);
  else launch_window<true, false, ASM_TAIL_NONE>(src, src_bytes, descs, N, out_h, out_w, nullptr, out, stream);
  ASM_CHECK_LAUNCH("resize_crop_flip");
  return ASM_OK;
}

extern "C" int asm_preprocess_window(const uint8_t* src, int64_t src_bytes, const asm_image_desc* descs, int N,
                                     int out_h, int out_w, int source, int tail, const float* add, float* out,
                                     void* stream) {
  ASM_REQUIRE(N >= 0 && out_h > 0 && out_w > 0 && src_bytes >= 0, "preprocess_window: bad sizes");
  ASM_REQUIRE((long long)out_h * out_w < (1ll << 30), "preprocess_window: output too large");
  ASM_REQUIRE(source == ASM_SOURCE_BYTES || source == ASM_SOURCE_UNIT, "preprocess_window: unknown source mode %d", source);
  ASM_REQUIRE(tail == ASM_TAIL_NONE || tail == ASM_TAIL_MEANS || tail == ASM_TAIL_ADD_CLAMP,
              "preprocess_window: unknown tail mode %d", tail);
  ASM_REQUIRE(tail == ASM_TAIL_ADD_CLAMP || !add, "preprocess_window: an add table needs the add-and-clamp tail");
  if (N == 0) return ASM_OK;
  ASM_REQUIRE(src && descs && out, "preprocess_window: null pointer");
#define WINDOW_FORM(U, T)                                                                        \
  if ((source == ASM_SOURCE_UNIT) == U && tail == T)                                             \
    launch_window<false, U, T>(src, src_bytes, descs, N, out_h, out_w, add, out, stream)
  WINDOW_FORM(false, ASM_TAIL_NONE);
  WINDOW_FORM(false, ASM_TAIL_MEANS);
  WINDOW_FORM(false, ASM_TAIL_ADD_CLAMP);
  WINDOW_FORM(true, ASM_TAIL_NONE);
  WINDOW_FORM(true, ASM_TAIL_MEANS);
  WINDOW_FORM(true, ASM_TAIL_ADD_CLAMP);
#undef WINDOW_FORM
  ASM_CHECK_LAUNCH("preprocess_window");
  return ASM_OK;
}
