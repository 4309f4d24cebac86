// Per-pixel expressions shared by several translation units.  Kernels that must agree BIT FOR BIT - the float and the uint8 form of
// the network's last step, the PSNR kernel's and the output kernels' byte conversion - call these instead of restating them.
#pragma once
#include <hip/hip_runtime.h>

namespace edvr {

// tensor2img (basicsr/utils/img_util.py:36-98) of one value: clamp to [0, 1], x 255, np.round (half to even); an integer in [0, 255]
__device__ __forceinline__ float to_u8(float v) { return rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }

// byte / 255 in float32, correctly rounded (== numpy's float32 division for all 256 inputs, checked exhaustively by
// tests/test_gpu_data.py::test_division_is_numpy_division): q = u * fl(1/255), one Newton correction with the exact remainder.
// 3 VALU instructions instead of the ~10 of the IEEE division sequence.  Every kernel that turns input bytes into the floats the network
// reads (frames_u8_to_f32, crop_pad_frames_u8) calls this.
__device__ __forceinline__ float div255(unsigned u) {
  const float r = 1.f / 255.f, f = (float)u;
  const float q = __fmul_rn(f, r);
  return __fmaf_rn(__fmaf_rn(-q, 255.f, f), r, q);
}

// Y of one pixel as to_y_channel computes it (metric_util.py:34-47, matlab_functions.py:207-240), from the three bytes (integers in
// [0, 255] held as floats): float32 / 255, dot with the BT.601 row in double, + 16, / 255 -> float32, x 255 in float32.  NOT inlined:
// every image and every kernel (PSNR, SSIM, NIQE) must run the very same instruction sequence, or identical images stop giving a
// difference of exactly zero (PSNR = inf in the reference) and the float and byte entries of a metric stop agreeing bit for bit.
inline __device__ __noinline__ float y_of_bytes(float r8, float g8, float b8) {
  const float r = __fdiv_rn(r8, 255.f), g = __fdiv_rn(g8, 255.f), bl = __fdiv_rn(b8, 255.f);
  const double d = (double)bl * 24.966 + (double)g * 128.553 + (double)r * 65.481 + 16.0;
  return __fmul_rn((float)(d / 255.0), 255.f);
}

// The same for pixel `o` of a planar (3, h w) RGB float tensor: BGR image of the reference = channels (2, 1, 0) of the RGB tensor.
__device__ __forceinline__ float y_of_pixel(const float *__restrict__ p, int64_t o, int64_t hw) {
  return y_of_bytes(to_u8(p[o]), to_u8(p[hw + o]), to_u8(p[2 * hw + o]));
}

// ---- bilinear upsampling, align_corners=False: src = (dst + 0.5) / S - 0.5, clamped at 0
template <int S>
__device__ __forceinline__ void src_index(int dst, int in, int &i0, int &i1, float &l) {
  float s = ((float)dst + 0.5f) * (1.f / S) - 0.5f;
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  i1 = i0 + ((i0 < in - 1) ? 1 : 0);
  l = s - (float)i0;
}

// One bilinear sample with the rounding order written out (three fused multiply-adds on two products): every upsampling kernel
// calls this, so that their results are bit-identical whichever one a shape / alignment selects - left to -ffp-contract the
// compiler picks which product of `a * b + c * d` goes into the fma kernel by kernel.
__device__ __forceinline__ float bilerp(float v00, float v01, float v10, float v11, float lx, float ly) {
  const float top = __builtin_fmaf(lx, v01, (1.f - lx) * v00);
  const float bot = __builtin_fmaf(lx, v11, (1.f - lx) * v10);
  return __builtin_fmaf(ly, bot, (1.f - ly) * top);
}

// Output pixel (oy, ox) of the xS bilinear enlargement of one h x w plane (S = 4: the value edvr_upsample4x_add_f32 adds to y there).
template <int S>
__device__ __forceinline__ float upsample_at(const float *__restrict__ src, int h, int w, int oy, int ox) {
  int y0, y1, x0, x1;
  float ly, lx;
  src_index<S>(oy, h, y0, y1, ly);
  src_index<S>(ox, w, x0, x1, lx);
  return bilerp(src[y0 * w + x0], src[y0 * w + x1], src[y1 * w + x0], src[y1 * w + x1], lx, ly);
}

// 4 consecutive pixels of an interleaved (h, w, 3) byte row: v[c][i] = channel c of pixel i, already an integer in [0, 255] (to_u8); three
// dword stores where `o` is 4-byte aligned, twelve byte stores otherwise.  Shared by the byte tails of video.hip and resize.hip.
__device__ __forceinline__ void store_px4(uint8_t *__restrict__ o, const float (&v)[3][4], bool aligned) {
  uint8_t b[12];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) b[3 * i + c] = (uint8_t)(unsigned)v[c][i];
  if (aligned) {
    uint32_t *o32 = reinterpret_cast<uint32_t *>(o);
#pragma unroll
    for (int k = 0; k < 3; ++k) o32[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = b[k];
  }
}

}  // namespace edvr
