// resize.hip - MATLAB-style bicubic imresize on the device: the x4 LQ frames of a GT video ("BI x4") and the bicubic baseline of every
// SR table, next to the other kernels that turn the caller's bytes into network input (data.hip, video.hip).
//
// Reference: imresize / calculate_weights_indices (basicsr/utils/matlab_functions.py:88-170, 17-84) - a per-row, per-channel `mv` loop on
// the host that nothing calls; the datasets come from scripts/matlab_scripts/generate_bicubic_img.m.  Per axis, for the 1-based output x:
//   u = x / scale + 0.5 (1 - 1 / scale), support kw = 4 (4 / scale when antialiasing a reduction), first tap floor(u - kw / 2),
//   ceil(kw) + 2 taps of the Keys cubic (a = -0.5; scale * cubic(scale * d) when antialiasing), normalised to sum 1,
//   taps outside the frame read the symmetric extension (... 1 0 | 0 1 ...).  Rows first, then columns.
// (The reference drops first / last tap columns that are zero for every output; a zero weight changes no value.)
//
// ONE launch does both passes.  A workgroup owns a toh x tow OUTPUT tile of one frame, all three channels:
//   0. the tile's toh + tow weight rows and first-tap indices are computed in float64 (u reaches thousands: a float32 u would carry
//      1e-4 of a pixel at 4K) and kept in LDS as float32 - no table tensors, the call allocates nothing and waits for nothing;
//   1. vertical pass: thread = 16 contiguous source bytes (or 4 floats) of the tile's column window x one output row; per tap one
//      16-byte global load where the rows are 16-byte aligned, div255 per byte, one fma per sample; the result goes to LDS.  The rows a
//      tile reads again for its next output row come from L1 / L2: HBM sees the tile's window (with its halo) once;
//   2. horizontal pass: thread = one output sample, taps read from LDS, result to an LDS output tile;
//   3. store: float planes (16 bytes per lane) or tensor2img bytes (three dwords per 4 pixels) of the SAME float values - the byte
//      output is the rounding of the float output by construction, and the uint8 source differs from the float one in the load only.
// Tap loops have a runtime bound and accumulate into named unrolled registers (no dynamically indexed per-thread array: 0 scratch).
#include <algorithm>
#include <cmath>

#include "common.h"
#include "lq_window.h"
#include "pixel.h"

namespace edvr {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct ResizeArgs {
  const void *src;
  void *dst;
  int64_t src_img_stride;  // float source: floats between images (the uint8 source is dense)
  double scale;
  int H, W, ho, wo;
  int toh, tow;  // output tile (tow % 4 == 0)
  int taps;      // ceil(kw) + 2
  int ms;        // columns of one row of the vertical pass's result in LDS (>= the widest column window of a tile)
  int aa_down;   // scale < 1 with antialiasing: the stretched kernel
  int src_vec, dst_vec, out_u8;
  // the windowed form (WIN; lq_window.h): the source is n windows of wh rows of `pitch` bytes, H and W come from the table, ho = wo = p
  const int32_t *table;
  int wh, ww, pitch;
};

__device__ __forceinline__ double keys_cubic(double x) {
  const double a = fabs(x), a2 = a * a, a3 = a2 * a;
  return a <= 1.0 ? 1.5 * a3 - 2.5 * a2 + 1.0 : (a <= 2.0 ? -0.5 * a3 + 2.5 * a2 - 4.0 * a + 2.0 : 0.0);
}

// 0-based index of the symmetric extension; the host admits only frames one reflection reaches, the clamp keeps every read inside
// the frame whatever float32 / float64 rounding does to a tap of weight ~0 at the very edge
__device__ __forceinline__ int sym_index(int i, int n) {
  i = i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i);
  return min(max(i, 0), n - 1);
}

// weights of 1-based output x1 -> w[t * stride], t < taps; returns the 0-based index of tap 0
__device__ int axis_weights(int x1, const ResizeArgs &a, float *w, int stride) {
  const double s = a.scale, kw = a.aa_down ? 4.0 / s : 4.0;
  const double u = x1 / s + 0.5 * (1.0 - 1.0 / s);
  const double left = floor(u - kw / 2);
  double sum = 0.0;
  for (int t = 0; t < a.taps; ++t) {
    const double d = u - (left + t);
    sum += a.aa_down ? s * keys_cubic(d * s) : keys_cubic(d);
  }
  for (int t = 0; t < a.taps; ++t) {
    const double d = u - (left + t);
    w[t * stride] = (float)((a.aa_down ? s * keys_cubic(d * s) : keys_cubic(d)) / sum);
  }
  return (int)left - 1;
}

// WIN: output (oy, ox) of image `img` is sample (top + oy, left + ox) of the resized FRAME, and the source is a window of that frame
// (U8IN, byte output); every index is formed in frame coordinates and passes through view_index last
template <bool U8IN, bool WIN>
__global__ __launch_bounds__(256) void imresize_bicubic_kernel(const ResizeArgs a) {
  extern __shared__ float smem[];
  const int toh = a.toh, tow = a.tow, taps = a.taps, ms = a.ms, os = tow + 1;
  float *mid = smem;                    // [3][toh][ms]  vertical pass
  float *outt = mid + 3 * toh * ms;     // [3][toh][tow + 1]  both passes
  float *wy = outt + 3 * toh * os;      // [toh][taps]
  float *wx = wy + toh * taps;          // [taps][tow]
  int *ly = reinterpret_cast<int *>(wx + taps * tow);  // [toh] first tap (row) of each output row
  int *lx = ly + toh;                                  // [tow] first tap (column) of each output column
  int bx, by, img;
  xcd_block_index(bx, by, img);
  const int oy0 = by * toh, ox0 = bx * tow;
  const int nvy = min(toh, a.ho - oy0), nvx = min(tow, a.wo - ox0);
  const int tid = threadIdx.x;
  int H = a.H, W = a.W;
  int ay0 = 0, ax0 = 0;                // absolute index of output (0, 0)
  int vy0 = 0, vx0 = 0, vh = H, vw = W;  // the source view: rows [vy0, vy0 + vh) x columns [vx0, vx0 + vw) of the frame
  if (WIN) {
    const int32_t *rec = a.table + (int64_t)LQW_REC * img;
    vy0 = window_origin(rec[LQW_Y0]), vx0 = window_origin(rec[LQW_X0]), vh = a.wh, vw = a.ww;
    H = rec[LQW_H], W = rec[LQW_W], ay0 = rec[LQW_TOP], ax0 = rec[LQW_LEFT];
  }
  const int64_t pitch = WIN ? (int64_t)a.pitch : (int64_t)W * 3;  // bytes of a source row (U8IN)

  // ---- 0. weights (waves 0 and 1..3 take an axis each)
  if (tid < toh) ly[tid] = axis_weights(ay0 + oy0 + tid + 1, a, wy + tid * taps, 1);
  if (tid >= 64 && tid - 64 < tow) lx[tid - 64] = axis_weights(ax0 + ox0 + (tid - 64) + 1, a, wx + (tid - 64), tow);
  __syncthreads();

  // the tile's column window [lo, lo + ncols) of the source: what its taps reach, reflections included
  const int raw_lo = lx[0], raw_hi = lx[nvx - 1] + taps - 1;
  int lo = max(raw_lo, 0), hi = min(raw_hi, W - 1);
  if (raw_lo < 0) hi = max(hi, min(-raw_lo - 1, W - 1));
  if (raw_hi > W - 1) lo = min(lo, max(2 * W - 1 - raw_hi, 0));
  if (WIN) lo = min(max(lo, vx0), vx0 + vw - 1), hi = min(max(hi, lo), vx0 + vw - 1);  // taps of weight zero may leave the window
  const int ncols = min(hi - lo + 1, ms);
  const int llo = lo - vx0;  // first column of the tile's window inside the view

  // ---- 1. vertical pass: source -> mid
  if (U8IN) {
    const uint8_t *src = static_cast<const uint8_t *>(a.src) + (int64_t)img * vh * pitch;
    const int g_lo = (3 * llo) >> 4, ng = ((3 * (llo + ncols) - 1) >> 4) - g_lo + 1;  // 16-byte groups of a source row
    for (int item = tid; item < nvy * ng; item += 256) {
      const int oyl = item / ng, g = g_lo + item - oyl * ng;
      const int first = ly[oyl];
      float acc[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[k] = 0.f;
      for (int t = 0; t < taps; ++t) {
        const uint8_t *row = src + view_index<WIN>(sym_index(first + t, H), vy0, vh) * pitch;
        const float w = wy[oyl * taps + t];
        uint32_t q[4];
        if (a.src_vec) {
          const u32x4 v = *reinterpret_cast<const u32x4 *>(row + 16 * g);
          q[0] = v[0], q[1] = v[1], q[2] = v[2], q[3] = v[3];
        } else {
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            q[d] = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) q[d] |= (uint32_t)row[min(16 * g + 4 * d + e, 3 * W - 1)] << (8 * e);
          }
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = __builtin_fmaf(w, div255((q[k >> 2] >> (8 * (k & 3))) & 0xffu), acc[k]);
      }
      const int p0 = (16 * g) / 3, r0 = 16 * g - 3 * p0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int rel = p0 + (r0 + k) / 3 - llo, c = (r0 + k) % 3;
        if (rel >= 0 && rel < ncols) mid[(c * toh + oyl) * ms + rel] = acc[k];
      }
    }
  } else {
    const float *src = static_cast<const float *>(a.src) + (int64_t)img * a.src_img_stride;
    const int g_lo = lo >> 2, ng = ((lo + ncols - 1) >> 2) - g_lo + 1;  // groups of 4 floats of a source row
    for (int item = tid; item < 3 * nvy * ng; item += 256) {
      const int cr = item / ng, g = g_lo + item - cr * ng;
      const int c = cr / nvy, oyl = cr - c * nvy;
      const int first = ly[oyl];
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int t = 0; t < taps; ++t) {
        const float *row = src + ((int64_t)c * H + sym_index(first + t, H)) * W;
        const float w = wy[oyl * taps + t];
        f32x4 v;
        if (a.src_vec) {
          v = *reinterpret_cast<const f32x4 *>(row + 4 * g);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = row[min(4 * g + k, W - 1)];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(w, v[k], acc[k]);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int rel = 4 * g + k - lo;
        if (rel >= 0 && rel < ncols) mid[(c * toh + oyl) * ms + rel] = acc[k];
      }
    }
  }
  __syncthreads();

  // ---- 2. horizontal pass: mid -> outt
  for (int item = tid; item < 3 * nvy * nvx; item += 256) {
    const int cr = item / nvx, oxl = item - cr * nvx;
    const int c = cr / nvy, oyl = cr - c * nvy;
    const float *m = mid + (c * toh + oyl) * ms;
    const int first = lx[oxl];
    float acc = 0.f;
    for (int t = 0; t < taps; ++t) {
      const int rel = min(max(sym_index(first + t, W) - lo, 0), ncols - 1);
      acc = __builtin_fmaf(wx[t * tow + oxl], m[rel], acc);
    }
    outt[(c * toh + oyl) * os + oxl] = acc;
  }
  __syncthreads();

  // ---- 3. store
  const int ho = a.ho, wo = a.wo;
  if (!a.out_u8) {
    float *dst = static_cast<float *>(a.dst) + (int64_t)img * 3 * ho * wo;
    if (a.dst_vec) {  // wo % 4 == 0: a group of 4 columns lies inside the frame or outside it
      const int gq = tow >> 2;
      for (int item = tid; item < 3 * nvy * gq; item += 256) {
        const int cr = item / gq, oxl = 4 * (item - cr * gq);
        const int c = cr / nvy, oyl = cr - c * nvy;
        if (ox0 + oxl >= wo) continue;
        const float *o = outt + (c * toh + oyl) * os + oxl;
        const f32x4 v = {o[0], o[1], o[2], o[3]};
        *reinterpret_cast<f32x4 *>(dst + ((int64_t)c * ho + oy0 + oyl) * wo + ox0 + oxl) = v;
      }
    } else {
      for (int item = tid; item < 3 * nvy * nvx; item += 256) {
        const int cr = item / nvx, oxl = item - cr * nvx;
        const int c = cr / nvy, oyl = cr - c * nvy;
        dst[((int64_t)c * ho + oy0 + oyl) * wo + ox0 + oxl] = outt[(c * toh + oyl) * os + oxl];
      }
    }
  } else {
    uint8_t *dst = static_cast<uint8_t *>(a.dst) + (int64_t)img * ho * wo * 3;
    if (a.dst_vec) {
      const int gq = tow >> 2;
      for (int item = tid; item < nvy * gq; item += 256) {
        const int oyl = item / gq, oxl = 4 * (item - oyl * gq);
        if (ox0 + oxl >= wo) continue;
        float v[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) v[c][i] = to_u8(outt[(c * toh + oyl) * os + oxl + i]);
        store_px4(dst + ((int64_t)(oy0 + oyl) * wo + ox0 + oxl) * 3, v, true);
      }
    } else {
      for (int item = tid; item < 3 * nvy * nvx; item += 256) {
        const int pr = item / 3, c = item - pr * 3;
        const int oyl = pr / nvx, oxl = pr - oyl * nvx;
        dst[((int64_t)(oy0 + oyl) * wo + ox0 + oxl) * 3 + c] = (uint8_t)(unsigned)to_u8(outt[(c * toh + oyl) * os + oxl]);
      }
    }
  }
}

static inline bool resize_aligned(const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// How far the taps of one axis reach beyond a frame of `in` samples resampled to `out` (the reference's sym_len_s / sym_len_e): weights
// are non-zero strictly inside (u - kw / 2, u + kw / 2).  edvr_amd/data.py: imresize_shape states the same rule for Python callers.
static bool resize_axis_fits(int in, int out, double scale, bool aa_down) {
  const double kw = aa_down ? 4.0 / scale : 4.0, shift = 0.5 * (1.0 - 1.0 / scale);
  const double first = std::floor(1 / scale + shift - kw / 2) + 1, last = std::ceil(out / scale + shift + kw / 2) - 1;  // 1-based
  return 1 - first <= in && last - in <= in;
}

// tile: an enlargement writes 16 x 64 outputs from a few source rows; a reduction keeps 8 output rows (8 / scale + taps source rows)
// and as many columns as 64 KB of LDS hold.  Sets toh, tow, taps, ms; returns the bytes of LDS.
static size_t resize_tile(ResizeArgs &a, double scale, bool aa_down) {
  a.taps = (int)std::ceil(aa_down ? 4.0 / scale : 4.0) + 2;
  a.toh = scale >= 1.0 ? 16 : 8;
  size_t lds = 0;
  for (a.tow = 64; a.tow >= 16; a.tow >>= 1) {
    a.ms = ((int)std::ceil((a.tow - 1) / scale) + a.taps + 2) | 1;  // first taps of the tile's columns spread over <= ceil((tow - 1) / scale) + 1
    lds = sizeof(float) * ((size_t)3 * a.toh * a.ms + 3 * a.toh * (a.tow + 1) + (size_t)(a.toh + a.tow) * a.taps + a.toh + a.tow);
    if (lds <= 64 * 1024) break;
  }
  return lds;
}

static int resize_launch(bool u8in, const void *src, void *dst, int n, int H, int W, int64_t src_img_stride, int ho, int wo, double scale,
                         int antialiasing, int out_kind, edvr_stream_t stream) {
  EDVR_REQUIRE(src && dst && n > 0 && n <= 65535 && H > 0 && W > 0 && ho > 0 && wo > 0 &&
                   (out_kind == EDVR_RESIZE_OUT_F32 || out_kind == EDVR_RESIZE_OUT_U8) && (u8in || n == 1 || src_img_stride >= 3 * (int64_t)H * W),
               "imresize_bicubic: bad arguments");
  EDVR_REQUIRE(scale >= 0.125 && scale <= 8.0, "imresize_bicubic: scale %g is outside [1/8, 8]", scale);
  EDVR_REQUIRE(std::fabs(ho - H * scale) <= 1.0 && std::fabs(wo - W * scale) <= 1.0,
               "imresize_bicubic: output %d x %d is not ceil(%d x %d times %g)", ho, wo, H, W, scale);
  const bool aa_down = antialiasing && scale < 1.0;
  EDVR_REQUIRE(resize_axis_fits(H, ho, scale, aa_down) && resize_axis_fits(W, wo, scale, aa_down),
               "imresize_bicubic: a %d x %d frame is shorter than the symmetric extension reaches at scale %g", H, W, scale);
  ResizeArgs a;
  a.src = src, a.dst = dst, a.src_img_stride = src_img_stride, a.scale = scale, a.H = H, a.W = W, a.ho = ho, a.wo = wo;
  a.aa_down = aa_down, a.out_u8 = out_kind == EDVR_RESIZE_OUT_U8;
  const size_t lds = resize_tile(a, scale, aa_down);
  EDVR_REQUIRE(lds <= 64 * 1024 && cdiv(ho, a.toh) <= 65535, "imresize_bicubic: no tile for scale %g / %d output rows", scale, ho);
  a.src_vec = u8in ? ((3 * (int64_t)W) % 16 == 0 && resize_aligned(src, 16)) : (W % 4 == 0 && src_img_stride % 4 == 0 && resize_aligned(src, 16));
  a.dst_vec = wo % 4 == 0 && resize_aligned(dst, a.out_u8 ? 4 : 16);
  const dim3 grid(cdiv(wo, a.tow), cdiv(ho, a.toh), n);
  a.table = nullptr, a.wh = a.ww = a.pitch = 0;
  if (u8in) hipLaunchKernelGGL((imresize_bicubic_kernel<true, false>), grid, dim3(256), lds, as_stream(stream), a);
  else hipLaunchKernelGGL((imresize_bicubic_kernel<false, false>), grid, dim3(256), lds, as_stream(stream), a);
  return check_launch("imresize_bicubic_kernel");
}

// n crops of p x p LQ samples from n windows of their GT frames (lq_window.h): the same kernel, the same tile, another view of the source
static int resize_windows_launch(const uint8_t *src, const int32_t *table, const int32_t *table_host, uint8_t *dst, int n, int p, int wh, int ww,
                                 int pitch, int scale, edvr_stream_t stream) {
  EDVR_REQUIRE(src && table && dst, "imresize_bicubic_windows: bad arguments");
  const char *why = lqw_check(LQW_BI, scale, n, p, wh, ww, pitch, src, table_host);
  EDVR_REQUIRE(!why, "imresize_bicubic_windows: %s (n %d, crop %d, window %d x %d, pitch %d, scale %d)", why, n, p, wh, ww, pitch, scale);
  ResizeArgs a;
  a.src = src, a.dst = dst, a.src_img_stride = 0, a.scale = 1.0 / scale, a.H = a.W = 0, a.ho = a.wo = p;
  a.aa_down = 1, a.out_u8 = 1;
  const size_t lds = resize_tile(a, a.scale, true);
  EDVR_REQUIRE(lds <= 64 * 1024, "imresize_bicubic_windows: no tile for scale %d", scale);
  a.src_vec = 1;  // lqw_check: every window row starts on a 16-byte boundary and the pitch covers its last group
  a.dst_vec = p % 4 == 0 && resize_aligned(dst, 4);
  a.table = table, a.wh = wh, a.ww = ww, a.pitch = pitch;
  hipLaunchKernelGGL((imresize_bicubic_kernel<true, true>), dim3(cdiv(p, a.tow), cdiv(p, a.toh), n), dim3(256), lds, as_stream(stream), a);
  return check_launch("imresize_bicubic_kernel (windows)");
}

}  // namespace edvr

extern "C" int edvr_imresize_bicubic_u8_windows(const uint8_t *src, const int32_t *table, const int32_t *table_host, uint8_t *dst, int n, int p,
                                                int wh, int ww, int pitch, int scale, edvr_stream_t stream) {
  return edvr::resize_windows_launch(src, table, table_host, dst, n, p, wh, ww, pitch, scale, stream);
}

extern "C" int edvr_imresize_bicubic_u8(const uint8_t *src, void *dst, int n, int H, int W, int ho, int wo, double scale, int antialiasing,
                                        int out_kind, edvr_stream_t stream) {
  return edvr::resize_launch(true, src, dst, n, H, W, 0, ho, wo, scale, antialiasing, out_kind, stream);
}

extern "C" int edvr_imresize_bicubic_f32(const float *src, void *dst, int n, int H, int W, int64_t src_img_stride, int ho, int wo,
                                         double scale, int antialiasing, int out_kind, edvr_stream_t stream) {
  return edvr::resize_launch(false, src, dst, n, H, W, src_img_stride, ho, wo, scale, antialiasing, out_kind, stream);
}
