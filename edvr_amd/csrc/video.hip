// video.hip - glue of the whole-video path (edvr_amd/video.py) for gfx950: every frame's feature pyramid is computed once and kept
// in a bank; a window of `num_frame` neighbours per output frame is then a GATHER of bank images by an index table, and the
// restored frames leave the device as the bytes tensor2img would store.
//
//   edvr_gather_images_f32   dst[l][j] = src[l][table[j]] for up to three pyramid levels in one launch (pure bandwidth)
//   edvr_upsample4x_add_u8   to_u8(y + bilinear_x4(base)) -> interleaved HWC bytes  (edvr_arch.py:417-419 + img_util.py:36-98)
//   edvr_f32_to_u8_hwc       to_u8(x) -> interleaved HWC bytes
//
// The two byte kernels evaluate the very expressions of edvr_upsample4x_add_f32 and of the PSNR kernel's conversion (pixel.h), so
// the bytes equal to_u8 of what the float path stores.
#include <algorithm>

#include "common.h"
#include "pixel.h"

namespace edvr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct GatherArgs {
  const float *src[EDVR_GATHER_MAX_LEVELS];
  float *dst[EDVR_GATHER_MAX_LEVELS];
  int64_t src_img_stride[EDVR_GATHER_MAX_LEVELS];
  int64_t per_img[EDVR_GATHER_MAX_LEVELS];
  int vec[EDVR_GATHER_MAX_LEVELS];  // 16-byte accesses allowed (pointers, stride and image size are whole 16-byte groups)
  const int *table;
  int n_src;
};

// grid (blocks per image, n_out, levels): a workgroup copies a share of ONE image; its source index is one wave-uniform load.
// An index outside [0, n_src) never leaves the bank: the destination image is filled with NaN instead (visible, not a fault).
__global__ __launch_bounds__(256) void gather_images_kernel(const GatherArgs a) {
  const int lv = blockIdx.z, j = blockIdx.y;
  const int s = a.table[j];
  const bool ok = s >= 0 && s < a.n_src;
  const int64_t per = a.per_img[lv];
  const float *__restrict__ src = a.src[lv] + (ok ? (int64_t)s * a.src_img_stride[lv] : 0);
  float *__restrict__ dst = a.dst[lv] + (int64_t)j * per;
  const int64_t step = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const float bad = __builtin_nanf("");
  if (a.vec[lv]) {
    const int64_t nv = per >> 2;
    const f32x4 *__restrict__ s4 = reinterpret_cast<const f32x4 *>(src);
    f32x4 *__restrict__ d4 = reinterpret_cast<f32x4 *>(dst);
    const f32x4 bad4 = {bad, bad, bad, bad};
    for (int64_t i = first; i < nv; i += step) d4[i] = ok ? s4[i] : bad4;
  } else {
    for (int64_t i = first; i < per; i += step) dst[i] = ok ? src[i] : bad;
  }
}

// thread = 4 consecutive pixels of one output row (the output width 4w is always a multiple of 4): three 16-byte loads of y (one per
// channel) where it is aligned, twelve bilinear samples of base, twelve bytes = three dword stores where out is aligned.
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

__global__ __launch_bounds__(256) void upsample4x_add_u8_kernel(const float *__restrict__ y, const float *__restrict__ base, uint8_t *__restrict__ out,
                                                                int n, int h, int w, int aligned) {
  const int ho = 4 * h, wo = 4 * w;
  const int64_t plane = (int64_t)ho * wo, total = (int64_t)n * ho * w;  // w groups of 4 pixels per output row
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int g = (int)(idx % w);
    const int oy = (int)((idx / w) % ho);
    const int64_t img = idx / ((int64_t)w * ho);
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float *yp = y + (img * 3 + c) * plane + (int64_t)oy * wo + 4 * g;
      const float *bp = base + (img * 3 + c) * (int64_t)h * w;
      float yv[4];
      if (aligned) {
        const f32x4 q = *reinterpret_cast<const f32x4 *>(yp);
        yv[0] = q[0], yv[1] = q[1], yv[2] = q[2], yv[3] = q[3];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) yv[i] = yp[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) v[c][i] = to_u8(yv[i] + upsample_at<4>(bp, h, w, oy, 4 * g + i));  // = to_u8 of edvr_upsample4x_add_f32's y
    }
    store_px4(out + ((img * ho + oy) * (int64_t)wo + 4 * g) * 3, v, aligned);
  }
}

// FAST (w % 4 == 0, aligned pointers): thread = 4 pixels of a row as above; else thread = one pixel, three byte stores
template <bool FAST>
__global__ __launch_bounds__(256) void f32_to_u8_hwc_kernel(const float *__restrict__ x, uint8_t *__restrict__ out, int n, int h, int w,
                                                            int64_t x_img_stride) {
  const int64_t plane = (int64_t)h * w;
  if (FAST) {
    const int wq = w >> 2;
    const int64_t total = (int64_t)n * h * wq;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
      const int g = (int)(idx % wq);
      const int oy = (int)((idx / wq) % h);
      const int64_t img = idx / ((int64_t)wq * h);
      float v[3][4];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const f32x4 q = *reinterpret_cast<const f32x4 *>(x + img * x_img_stride + c * plane + (int64_t)oy * w + 4 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[c][i] = to_u8(q[i]);
      }
      store_px4(out + ((img * h + oy) * (int64_t)w + 4 * g) * 3, v, true);
    }
  } else {
    const int64_t total = (int64_t)n * plane;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
      const int64_t img = idx / plane, o = idx % plane;
#pragma unroll
      for (int c = 0; c < 3; ++c) out[idx * 3 + c] = (uint8_t)(unsigned)to_u8(x[img * x_img_stride + c * plane + o]);
    }
  }
}

static inline int grid_blocks(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>(cdiv64(n, 256), 1), 65536); }
static inline bool aligned_to(const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace edvr

extern "C" int edvr_gather_images_f32(const float *const *src, float *const *dst, const int64_t *src_img_stride, const int64_t *per_img,
                                      int levels, const int *table, int n_out, int n_src, edvr_stream_t stream) {
  using namespace edvr;
  EDVR_REQUIRE(src && dst && src_img_stride && per_img && table && levels >= 1 && levels <= EDVR_GATHER_MAX_LEVELS && n_out > 0 && n_out <= 65535 &&
                   n_src > 0,
               "gather_images: bad arguments");
  GatherArgs a;
  int64_t most = 0;
  for (int l = 0; l < EDVR_GATHER_MAX_LEVELS; ++l) {
    const int k = l < levels ? l : 0;  // (unused slots repeat level 0: never dereferenced, the grid has `levels` layers)
    EDVR_REQUIRE(src[k] && dst[k] && per_img[k] > 0 && (n_src == 1 || src_img_stride[k] >= per_img[k]), "gather_images: bad level %d", k);
    a.src[l] = src[k], a.dst[l] = dst[k], a.src_img_stride[l] = src_img_stride[k], a.per_img[l] = per_img[k];
    a.vec[l] = per_img[k] % 4 == 0 && src_img_stride[k] % 4 == 0 && aligned_to(src[k], 16) && aligned_to(dst[k], 16);
    most = std::max(most, a.vec[l] ? per_img[k] / 4 : per_img[k]);
  }
  a.table = table, a.n_src = n_src;
  const int per_image_blocks = (int)std::min<int64_t>(std::max<int64_t>(cdiv64(most, 256 * 8), 1), 256);  // ~8 accesses per lane on the largest level
  hipLaunchKernelGGL(gather_images_kernel, dim3(per_image_blocks, n_out, levels), dim3(256), 0, as_stream(stream), a);
  return check_launch("gather_images_kernel");
}

extern "C" int edvr_upsample4x_add_u8(const float *y, const float *base, uint8_t *out, int n, int h, int w, edvr_stream_t stream) {
  using namespace edvr;
  EDVR_REQUIRE(y && base && out && n > 0 && h > 0 && w > 0, "upsample4x_add_u8: bad arguments");
  const int aligned = aligned_to(y, 16) && aligned_to(out, 4);
  hipLaunchKernelGGL(upsample4x_add_u8_kernel, dim3(grid_blocks((int64_t)n * 4 * h * w)), dim3(256), 0, as_stream(stream), y, base, out, n, h, w, aligned);
  return check_launch("upsample4x_add_u8_kernel");
}

extern "C" int edvr_f32_to_u8_hwc(const float *x, uint8_t *out, int n, int h, int w, int64_t x_img_stride, edvr_stream_t stream) {
  using namespace edvr;
  EDVR_REQUIRE(x && out && n > 0 && h > 0 && w > 0 && (n == 1 || x_img_stride >= 3 * (int64_t)h * w), "f32_to_u8_hwc: bad arguments");
  if (w % 4 == 0 && x_img_stride % 4 == 0 && aligned_to(x, 16) && aligned_to(out, 4))
    hipLaunchKernelGGL(f32_to_u8_hwc_kernel<true>, dim3(grid_blocks((int64_t)n * h * (w / 4))), dim3(256), 0, as_stream(stream), x, out, n, h, w, x_img_stride);
  else
    hipLaunchKernelGGL(f32_to_u8_hwc_kernel<false>, dim3(grid_blocks((int64_t)n * h * w)), dim3(256), 0, as_stream(stream), x, out, n, h, w, x_img_stride);
  return check_launch("f32_to_u8_hwc_kernel");
}
