// video.hip - glue of the whole-video path (edvr_amd/video.py) for gfx950: every frame's feature pyramid is computed once and kept
// in a bank; a window of `num_frame` neighbours per output frame is then a GATHER of bank images by an index table, and the
// restored frames leave the device as the bytes tensor2img would store.
//
//   edvr_gather_images_f32   dst[l][j] = src[l][table[j]] for up to three pyramid levels in one launch (pure bandwidth)
//   edvr_upsample4x_add_u8   to_u8(y + bilinear_x4(base)) -> interleaved HWC bytes  (edvr_arch.py:417-419 + img_util.py:36-98)
//   edvr_f32_to_u8_hwc       to_u8(x) -> interleaved HWC bytes
//   edvr_crop_pad_frames_*   a rectangle of the bottom / right padded frames (uint8 HWC or float32 CHW) -> dense float32 tiles
//   edvr_*_rect_*            the three tails (and a copy) storing a kept rectangle of a tile's result into the full-frame output
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

// ---- frames of any size (edvr_amd/video.py: pad_mode / tile).  A TILE is a (th, tw) rectangle of the frame extended at the bottom and
// right to the network's size multiple; the per-frame stage reads tiles, the network's last kernel writes the KEPT part of a tile's
// result into the full-frame output.

// torch.nn.functional.pad's index rule for a coordinate beyond the last one (the host admits only j <= 2 (n - 1) under 'reflect')
__device__ __forceinline__ int pad_index(int j, int n, int reflect) { return j < n ? j : (reflect ? 2 * (n - 1) - j : n - 1); }

struct CropArgs {
  const void *src;
  float *dst;
  int64_t src_img_stride;  // float source: floats between images (the uint8 source is dense)
  int n, H, W, y0, x0, th, tw, reflect;
  int src_vec;             // source groups of 4 pixels that lie inside the frame may be read by aligned wide loads
};

// VEC (tw % 4 == 0, dst 16-byte aligned): thread = 4 consecutive pixels of one tile row, three 16-byte stores (one per channel).  A group
// wholly inside the frame at an aligned source address is read by three dword loads; the padded tail of a row (and every group of a
// frame whose rows do not start on dword boundaries) byte by byte through pad_index.  Generic: thread = one pixel.
template <bool VEC>
__global__ __launch_bounds__(256) void crop_pad_frames_u8_kernel(const CropArgs a) {
  const uint8_t *__restrict__ src = static_cast<const uint8_t *>(a.src);
  const int64_t plane = (int64_t)a.th * a.tw;
  if (VEC) {
    const int wq = a.tw >> 2;
    const int64_t total = (int64_t)a.n * a.th * wq;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
      const int g = (int)(idx % wq);
      const int r = (int)((idx / wq) % a.th);
      const int64_t img = idx / ((int64_t)wq * a.th);
      const int sy = pad_index(a.y0 + r, a.H, a.reflect), sx = a.x0 + 4 * g;
      const uint8_t *row = src + (img * a.H + sy) * (int64_t)a.W * 3;
      uint32_t px[4];  // px[i] = the three bytes of pixel 4 g + i
      if (a.src_vec && sx + 3 < a.W) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(row + (int64_t)sx * 3);
        const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
        px[0] = w0 & 0xffffffu, px[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8), px[2] = (w1 >> 16) | ((w2 & 0xffu) << 16), px[3] = w2 >> 8;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint8_t *p = row + (int64_t)pad_index(sx + i, a.W, a.reflect) * 3;
          px[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = div255((px[i] >> (8 * c)) & 0xffu);
        *reinterpret_cast<f32x4 *>(a.dst + (img * 3 + c) * plane + (int64_t)r * a.tw + 4 * g) = v;
      }
    }
  } else {
    const int64_t total = (int64_t)a.n * plane;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
      const int q = (int)(idx % a.tw);
      const int r = (int)((idx / a.tw) % a.th);
      const int64_t img = idx / plane;
      const uint8_t *p = src + ((img * a.H + pad_index(a.y0 + r, a.H, a.reflect)) * (int64_t)a.W + pad_index(a.x0 + q, a.W, a.reflect)) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) a.dst[(img * 3 + c) * plane + (int64_t)r * a.tw + q] = div255(p[c]);
    }
  }
}

// float source (n, 3, H, W), dense images src_img_stride apart: thread = 4 consecutive pixels of one row of one plane (VEC) or one element
template <bool VEC>
__global__ __launch_bounds__(256) void crop_pad_frames_f32_kernel(const CropArgs a) {
  const float *__restrict__ src = static_cast<const float *>(a.src);
  const int64_t plane = (int64_t)a.th * a.tw, splane = (int64_t)a.H * a.W;
  if (VEC) {
    const int wq = a.tw >> 2;
    const int64_t total = (int64_t)a.n * 3 * a.th * wq;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
      const int g = (int)(idx % wq);
      const int r = (int)((idx / wq) % a.th);
      const int64_t pl = idx / ((int64_t)wq * a.th);  // img * 3 + c
      const int sx = a.x0 + 4 * g;
      const float *row = src + (pl / 3) * a.src_img_stride + (pl % 3) * splane + (int64_t)pad_index(a.y0 + r, a.H, a.reflect) * a.W;
      f32x4 v;
      if (a.src_vec && sx + 3 < a.W) {
        v = *reinterpret_cast<const f32x4 *>(row + sx);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = row[pad_index(sx + i, a.W, a.reflect)];
      }
      *reinterpret_cast<f32x4 *>(a.dst + pl * plane + (int64_t)r * a.tw + 4 * g) = v;
    }
  } else {
    const int64_t total = (int64_t)a.n * 3 * plane;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
      const int q = (int)(idx % a.tw);
      const int r = (int)((idx / a.tw) % a.th);
      const int64_t pl = idx / plane;
      a.dst[idx] = src[(pl / 3) * a.src_img_stride + (pl % 3) * splane + (int64_t)pad_index(a.y0 + r, a.H, a.reflect) * a.W +
                       pad_index(a.x0 + q, a.W, a.reflect)];
    }
  }
}

// The three tails (and a plain copy) with a RECTANGLE store: the value of pixel (ky + r, kx + q) of a tile's result - the very expression
// the whole-tile kernel stores there, on the tile's own y and base - goes to (r, q) of a destination that has the row / plane / image
// strides of the full-frame output.  UP: + bilinear x4 of base (y is (n, 3, 4h, 4w) then, else (n, 3, h, w)); U8: interleaved bytes.
struct RectArgs {
  const float *y, *base;
  void *dst;
  int64_t y_img_stride, d_row, d_plane, d_img;  // destination strides in elements (d_plane: float destination only)
  int n, h, w, ky, kx, kh, kw;
  int d_vec;  // the destination takes aligned wide stores (16 bytes per channel in floats, three dwords in bytes)
};

// VEC (kx % 4 == 0, kw % 4 == 0, 16-byte aligned rows of y): thread = 4 consecutive pixels of a kept row, one 16-byte load of y per channel
template <bool UP, bool U8, bool VEC>
__global__ __launch_bounds__(256) void rect_store_kernel(const RectArgs a) {
  constexpr int P = VEC ? 4 : 1;
  const int hy = UP ? 4 * a.h : a.h, wy = UP ? 4 * a.w : a.w;
  const int wq = a.kw / P;
  const int64_t total = (int64_t)a.n * a.kh * wq, yplane = (int64_t)hy * wy;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int q = (int)(idx % wq) * P;
    const int r = (int)((idx / wq) % a.kh);
    const int64_t img = idx / ((int64_t)wq * a.kh);
    const int oy = a.ky + r, ox = a.kx + q;
    float v[3][P];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float *yp = a.y + img * a.y_img_stride + c * yplane + (int64_t)oy * wy + ox;
      if (VEC) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(yp);
#pragma unroll
        for (int i = 0; i < P; ++i) v[c][i] = t[i];
      } else {
        v[c][0] = yp[0];
      }
      if (UP) {
        const float *bp = a.base + (img * 3 + c) * (int64_t)a.h * a.w;
#pragma unroll
        for (int i = 0; i < P; ++i) v[c][i] = v[c][i] + upsample_at<4>(bp, a.h, a.w, oy, ox + i);
      }
      if (U8) {
#pragma unroll
        for (int i = 0; i < P; ++i) v[c][i] = to_u8(v[c][i]);
      }
    }
    if (U8) {
      uint8_t *o = static_cast<uint8_t *>(a.dst) + img * a.d_img + (int64_t)r * a.d_row + (int64_t)q * 3;
      if constexpr (VEC) {
        store_px4(o, v, a.d_vec);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (uint8_t)(unsigned)v[c][0];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float *o = static_cast<float *>(a.dst) + img * a.d_img + c * a.d_plane + (int64_t)r * a.d_row + q;
        if (VEC && a.d_vec) {
          f32x4 t;
#pragma unroll
          for (int i = 0; i < P; ++i) t[i] = v[c][i];
          *reinterpret_cast<f32x4 *>(o) = t;
        } else {
#pragma unroll
          for (int i = 0; i < P; ++i) o[i] = v[c][i];
        }
      }
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

namespace edvr {

static int crop_pad_launch(bool u8, const void *src, float *dst, int n, int H, int W, int64_t src_img_stride, int y0, int x0, int th, int tw,
                           int pad_mode, edvr_stream_t stream) {
  const char *name = u8 ? "crop_pad_frames_u8_kernel" : "crop_pad_frames_f32_kernel";
  EDVR_REQUIRE(src && dst && n > 0 && H > 0 && W > 0 && th > 0 && tw > 0 && y0 >= 0 && x0 >= 0 && y0 < H && x0 < W &&
                   (pad_mode == EDVR_PAD_REFLECT || pad_mode == EDVR_PAD_REPLICATE) && (u8 || n == 1 || src_img_stride >= 3 * (int64_t)H * W),
               "crop_pad_frames: bad arguments");
  // 'reflect' mirrors without repeating the edge: the last index it can produce is 2 (n - 1) (torch: padding < input size)
  EDVR_REQUIRE(pad_mode != EDVR_PAD_REFLECT || (y0 + th - 1 <= 2 * (H - 1) && x0 + tw - 1 <= 2 * (W - 1)),
               "crop_pad_frames: a %d x %d rectangle at (%d, %d) reaches beyond the reflection of a %d x %d frame", th, tw, y0, x0, H, W);
  CropArgs a;
  a.src = src, a.dst = dst, a.src_img_stride = src_img_stride, a.n = n, a.H = H, a.W = W, a.y0 = y0, a.x0 = x0, a.th = th, a.tw = tw;
  a.reflect = pad_mode == EDVR_PAD_REFLECT;
  const bool vec = tw % 4 == 0 && aligned_to(dst, 16);
  // a group of 4 pixels starts at pixel ((img * H + y) * W + x0 + 4 g): a whole number of 12-byte / 16-byte units from src
  a.src_vec = W % 4 == 0 && x0 % 4 == 0 && (u8 ? aligned_to(src, 4) : (aligned_to(src, 16) && src_img_stride % 4 == 0));
  const dim3 grid(grid_blocks((int64_t)n * (u8 ? 1 : 3) * th * (vec ? tw / 4 : tw)));
  if (u8) {
    if (vec) hipLaunchKernelGGL(crop_pad_frames_u8_kernel<true>, grid, dim3(256), 0, as_stream(stream), a);
    else hipLaunchKernelGGL(crop_pad_frames_u8_kernel<false>, grid, dim3(256), 0, as_stream(stream), a);
  } else {
    if (vec) hipLaunchKernelGGL(crop_pad_frames_f32_kernel<true>, grid, dim3(256), 0, as_stream(stream), a);
    else hipLaunchKernelGGL(crop_pad_frames_f32_kernel<false>, grid, dim3(256), 0, as_stream(stream), a);
  }
  return check_launch(name);
}

template <bool UP, bool U8>
static int rect_launch(const char *name, const float *y, const float *base, void *dst, int n, int h, int w, int64_t y_img_stride, int ky, int kx,
                       int kh, int kw, int64_t d_row, int64_t d_plane, int64_t d_img, edvr_stream_t stream) {
  const int hy = UP ? 4 * h : h, wy = UP ? 4 * w : w;
  EDVR_REQUIRE(y && (base || !UP) && dst && n > 0 && h > 0 && w > 0 && ky >= 0 && kx >= 0 && kh > 0 && kw > 0 && ky + kh <= hy && kx + kw <= wy &&
                   (n == 1 || y_img_stride >= 3 * (int64_t)hy * wy) && d_row >= (U8 ? 3 : 1) * (int64_t)kw &&
                   (U8 || d_plane >= (kh - 1) * d_row + kw) && (n == 1 || d_img >= (U8 ? 0 : 2 * d_plane) + (kh - 1) * d_row + (U8 ? 3 : 1) * (int64_t)kw),
               "%s: bad arguments", name);
  RectArgs a;
  a.y = y, a.base = base, a.dst = dst, a.y_img_stride = y_img_stride, a.d_row = d_row, a.d_plane = d_plane, a.d_img = d_img;
  a.n = n, a.h = h, a.w = w, a.ky = ky, a.kx = kx, a.kh = kh, a.kw = kw;
  const bool vec = kx % 4 == 0 && kw % 4 == 0 && wy % 4 == 0 && y_img_stride % 4 == 0 && aligned_to(y, 16);
  a.d_vec = U8 ? (aligned_to(dst, 4) && d_row % 4 == 0 && d_img % 4 == 0)
               : (aligned_to(dst, 16) && d_row % 4 == 0 && d_plane % 4 == 0 && d_img % 4 == 0);
  const dim3 grid(grid_blocks((int64_t)n * kh * (vec ? kw / 4 : kw)));
  if (vec) hipLaunchKernelGGL((rect_store_kernel<UP, U8, true>), grid, dim3(256), 0, as_stream(stream), a);
  else hipLaunchKernelGGL((rect_store_kernel<UP, U8, false>), grid, dim3(256), 0, as_stream(stream), a);
  return check_launch(name);
}

}  // namespace edvr

extern "C" int edvr_crop_pad_frames_u8(const uint8_t *src, float *dst, int n, int H, int W, int y0, int x0, int th, int tw, int pad_mode,
                                       edvr_stream_t stream) {
  return edvr::crop_pad_launch(true, src, dst, n, H, W, 0, y0, x0, th, tw, pad_mode, stream);
}

extern "C" int edvr_crop_pad_frames_f32(const float *src, float *dst, int n, int H, int W, int64_t src_img_stride, int y0, int x0, int th, int tw,
                                        int pad_mode, edvr_stream_t stream) {
  return edvr::crop_pad_launch(false, src, dst, n, H, W, src_img_stride, y0, x0, th, tw, pad_mode, stream);
}

extern "C" int edvr_upsample4x_add_rect_f32(const float *y, const float *base, float *dst, int n, int h, int w, int ky, int kx, int kh, int kw,
                                            int64_t dst_row_stride, int64_t dst_plane_stride, int64_t dst_img_stride, edvr_stream_t stream) {
  return edvr::rect_launch<true, false>("upsample4x_add_rect_f32", y, base, dst, n, h, w, 48 * (int64_t)h * w, ky, kx, kh, kw, dst_row_stride,
                                        dst_plane_stride, dst_img_stride, stream);
}

extern "C" int edvr_upsample4x_add_rect_u8(const float *y, const float *base, uint8_t *dst, int n, int h, int w, int ky, int kx, int kh, int kw,
                                           int64_t dst_row_stride, int64_t dst_img_stride, edvr_stream_t stream) {
  return edvr::rect_launch<true, true>("upsample4x_add_rect_u8", y, base, dst, n, h, w, 48 * (int64_t)h * w, ky, kx, kh, kw, dst_row_stride, 0,
                                       dst_img_stride, stream);
}

extern "C" int edvr_f32_to_u8_hwc_rect(const float *x, uint8_t *dst, int n, int h, int w, int64_t x_img_stride, int ky, int kx, int kh, int kw,
                                       int64_t dst_row_stride, int64_t dst_img_stride, edvr_stream_t stream) {
  return edvr::rect_launch<false, true>("f32_to_u8_hwc_rect", x, nullptr, dst, n, h, w, x_img_stride, ky, kx, kh, kw, dst_row_stride, 0,
                                        dst_img_stride, stream);
}

extern "C" int edvr_copy_rect_f32(const float *x, float *dst, int n, int h, int w, int64_t x_img_stride, int ky, int kx, int kh, int kw,
                                  int64_t dst_row_stride, int64_t dst_plane_stride, int64_t dst_img_stride, edvr_stream_t stream) {
  return edvr::rect_launch<false, false>("copy_rect_f32", x, nullptr, dst, n, h, w, x_img_stride, ky, kx, kh, kw, dst_row_stride, dst_plane_stride,
                                         dst_img_stride, stream);
}
