// bd.hip - "BD" downsampling on the device: DUF's 13 x 13 Gaussian blur (sigma = 0.4 s) sampled at every s-th input sample, s in {2, 3, 4} -
// the LQ frames of the Vid4 / Vimeo-90K-T "BD" tables, next to the bicubic ("BI") ones of resize.hip.
//
// Reference: duf_downsample / generate_gaussian_kernel (basicsr/data/data_util.py:281-331) - on the host, F.pad(reflect) of the whole
// window by 6 + 2 s, a 169-tap F.conv2d of stride s one channel at a time, a crop of two outputs per side.  The same samples, directly:
//   out[i, j] = sum_{a, b = 0..12} g[a] g[b] x[R(i s - 6 + a, H), R(j s - 6 + b, W)],  R(p, n) = -p (p < 0), 2 (n - 1) - p (p >= n), p
// with g the 1-D kernel of scipy.ndimage.gaussian_filter (truncated at r = int(4 sigma + 0.5) = 3, 5, 6: 7, 11, 13 non-zero taps), whose
// outer product is the reference's 2-D filter exactly.  Separable: rows first, then columns, 2 (2 r + 1) taps per output instead of 169.
//
// ONE launch does both passes, in the structure of resize.hip.  The kernel is a template on s: the tap count 2 r + 1, the stride and the
// tile are compile-time, every tap loop is fully unrolled and the 13 float32 weights (computed on the host in float64) are kernel
// arguments, i.e. scalar registers - no weight table, no dynamically indexed per-thread array, 0 bytes of scratch.
// A workgroup owns a TOH x 64 OUTPUT tile of one frame (TOH = 16 at s = 2, else 8), all three channels:
//   1. vertical pass: thread = 16 contiguous source bytes (or 4 floats) of the tile's column window x TWO adjacent output rows: the
//      2 r + 1 + s source rows the pair needs are loaded (one 16-byte load each where rows are 16-byte aligned) and converted (div255 per
//      byte, as edvr_frames_u8_to_f32) once and feed both rows' accumulators, taps in ascending order; the result goes to LDS (`mid`);
//   2. columns of the window that lie outside the frame are copied inside LDS from their reflections (edge tiles only), so that
//   3. the horizontal pass (thread = one output sample) reads mid at the fixed pattern column = s * x + t and writes an LDS output tile;
//   4. store: float planes (16 bytes per lane) or tensor2img bytes (three dwords per 4 pixels) of the SAME float values - the byte
//      output is the rounding of the float output by construction, and the uint8 source differs from the float one in the load only.
// LDS layout of a mid row: lanes of the horizontal pass read at a stride of s floats, which on the 32 banks of ds_read_b32 is a 2-way
// (s = 2) or 4-way (s = 4) conflict in a plain [row][column] layout.  At s = 2 and 4 a row is therefore stored de-interleaved by phase,
// column k at (k % s) * PS + k / s: tap t of output x reads (t % s) * PS + x + t / s - consecutive lanes, consecutive banks.  s = 3 is
// coprime to 32 and keeps the plain layout.  Resulting conflict degree of the horizontal pass: 1 (none) for all three scales on tiles of
// full width (a wave then reads one row); tiles narrower than 32 outputs put several rows into one 32-lane group and may collide.  The
// float vertical pass writes lanes 4 columns apart: conflict-free at s = 4, 2-way at s = 2 (free for ds_write_b32), up to 2-way at
// s = 3; the byte vertical pass scatters 16 interleaved bytes per lane over three planes (16 stores per 17 x 16 conversions).
#include <algorithm>
#include <cmath>

#include "common.h"
#include "lq_window.h"
#include "pixel.h"

namespace edvr {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct BdArgs {
  const void *src;
  void *dst;
  int64_t src_img_stride;  // float source: floats between images (the uint8 source is dense)
  int H, W, ho, wo;
  int src_vec, dst_vec, out_u8;
  float g[13];  // the 1-D kernel, g[6] its centre; zero beyond the truncation radius
  // the windowed form (WIN; lq_window.h): the source is n windows of wh rows of `pitch` bytes, H and W come from the table, ho = wo = p
  const int32_t *table;
  int wh, ww, pitch;
};

template <int S>
struct BdCfg {
  static constexpr int R = S == 2 ? 3 : (S == 3 ? 5 : 6);  // int(4 * 0.4 * S + 0.5)
  static constexpr int NT = 2 * R + 1;                     // non-zero taps
  static constexpr int TOH = S == 2 ? 16 : 8, TOW = 64;    // output tile
  static constexpr int PH = S == 3 ? 1 : S;                // phases a mid row is de-interleaved into
  static constexpr int NCOLS = (TOW - 1) * S + NT;         // columns of the tile's window
  static constexpr int PS = (NCOLS + PH - 1) / PH;         // floats of one phase
  static constexpr int MS = PH * PS;                       // floats of one mid row
  static constexpr int OS = TOW + 1;
  // where column k of the window lives in its mid row
  __device__ static __forceinline__ int at(int k) { return PH == 1 ? k : (k % PH) * PS + k / PH; }
};

// index of the reflection that does not repeat the edge sample; the host admits only frames one reflection covers (n >= 7), the clamp
// keeps every read inside the frame regardless (rows of the unused second row of a pair reach further)
__device__ __forceinline__ int refl_index(int p, int n) {
  p = p < 0 ? -p : (p >= n ? 2 * (n - 1) - p : p);
  return min(max(p, 0), n - 1);
}

// WIN: output (oy, ox) of image `img` is sample (top + oy, left + ox) of the downsampled FRAME, and the source is a window of that frame
// (U8IN, byte output); every index is formed in frame coordinates and passes through view_index last
template <int S, bool U8IN, bool WIN>
__global__ __launch_bounds__(256) void bd_downsample_kernel(const BdArgs a) {
  using C = BdCfg<S>;
  constexpr int R = C::R, NT = C::NT, TOH = C::TOH, TOW = C::TOW, MS = C::MS, OS = C::OS, G0 = 6 - R;
  __shared__ float mid[3 * TOH * MS];   // [3][TOH] rows, vertical pass
  __shared__ float outt[3 * TOH * OS];  // [3][TOH][TOW + 1], both passes
  int bx, by, img;
  xcd_block_index(bx, by, img);
  const int oy0 = by * TOH, ox0 = bx * TOW;
  const int nvy = min(TOH, a.ho - oy0), nvx = min(TOW, a.wo - ox0);
  const int tid = threadIdx.x;
  int H = a.H, W = a.W;
  int ay0 = 0, ax0 = 0;                  // absolute index of output (0, 0)
  int vy0 = 0, vx0 = 0, vh = H, vw = W;  // the source view: rows [vy0, vy0 + vh) x columns [vx0, vx0 + vw) of the frame
  if (WIN) {
    const int32_t *rec = a.table + (int64_t)LQW_REC * img;
    vy0 = window_origin(rec[LQW_Y0]), vx0 = window_origin(rec[LQW_X0]), vh = a.wh, vw = a.ww;
    H = rec[LQW_H], W = rec[LQW_W], ay0 = rec[LQW_TOP], ax0 = rec[LQW_LEFT];
  }
  const int64_t pitch = WIN ? (int64_t)a.pitch : (int64_t)W * 3;  // bytes of a source row (U8IN)
  // the tile's column window [p0, p1] in unreflected coordinates; [lo, hi] is the part of it inside the frame.  Every reflection of a
  // column of the window falls into [lo, hi]: -p <= R <= p1 on the left, p0 <= W - 1 - R <= 2 (W - 1) - p on the right (W >= 7 > R).
  const int p0 = (ax0 + ox0) * S - R, p1 = p0 + (nvx - 1) * S + NT - 1;
  int lo = max(p0, 0), hi = min(p1, W - 1);
  if (WIN) {  // a window holds every column of non-zero weight; whatever the table says, [lo, hi] stays inside [p0, p1]
    lo = min(max(lo, vx0), p1), hi = max(min(hi, vx0 + vw - 1), lo);
  }
  const int npair = (nvy + 1) >> 1;

  // ---- 1. vertical pass: source -> mid, two output rows per thread
  if (U8IN) {
    const uint8_t *src = static_cast<const uint8_t *>(a.src) + (int64_t)img * vh * pitch;
    const int g_lo = (3 * (lo - vx0)) >> 4, ng = ((3 * (hi - vx0) + 2) >> 4) - g_lo + 1;  // 16-byte groups of a source row
    const int g_max = WIN ? (a.pitch >> 4) - 1 : 0;
    for (int item = tid; item < npair * ng; item += 256) {
      const int pr = item / ng;
      int g = g_lo + item - pr * ng;
      if (WIN) g = min(max(g, 0), g_max);
      const int oyl = 2 * pr, y0 = (ay0 + oy0 + oyl) * S - R;
      float acc0[16], acc1[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) acc0[k] = 0.f, acc1[k] = 0.f;
#pragma unroll
      for (int j = 0; j < NT + S; ++j) {
        const uint8_t *row = src + view_index<WIN>(refl_index(y0 + j, H), vy0, vh) * pitch;
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
        for (int k = 0; k < 16; ++k) {
          const float v = div255((q[k >> 2] >> (8 * (k & 3))) & 0xffu);
          if (j < NT) acc0[k] = __builtin_fmaf(a.g[G0 + (j < NT ? j : 0)], v, acc0[k]);
          if (j >= S) acc1[k] = __builtin_fmaf(a.g[G0 + (j >= S ? j - S : 0)], v, acc1[k]);
        }
      }
      const int px0 = (16 * g) / 3, r0 = 16 * g - 3 * px0;
      const bool second = oyl + 1 < nvy;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int col = vx0 + px0 + (r0 + k) / 3, c = (r0 + k) % 3;
        if (col >= lo && col <= hi) {
          float *m = mid + (c * TOH + oyl) * MS + C::at(col - p0);
          m[0] = acc0[k];
          if (second) m[MS] = acc1[k];
        }
      }
    }
  } else {
    const float *src = static_cast<const float *>(a.src) + (int64_t)img * a.src_img_stride;
    const int g_lo = lo >> 2, ng = (hi >> 2) - g_lo + 1;  // groups of 4 floats of a source row
    for (int item = tid; item < 3 * npair * ng; item += 256) {
      const int cp = item / ng, g = g_lo + item - cp * ng;
      const int c = cp / npair, pr = cp - c * npair;
      const int oyl = 2 * pr, y0 = (oy0 + oyl) * S - R;
      float acc0[4] = {0.f, 0.f, 0.f, 0.f}, acc1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < NT + S; ++j) {
        const float *row = src + ((int64_t)c * H + refl_index(y0 + j, H)) * W;
        f32x4 v;
        if (a.src_vec) {
          v = *reinterpret_cast<const f32x4 *>(row + 4 * g);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = row[min(4 * g + k, W - 1)];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (j < NT) acc0[k] = __builtin_fmaf(a.g[G0 + (j < NT ? j : 0)], v[k], acc0[k]);
          if (j >= S) acc1[k] = __builtin_fmaf(a.g[G0 + (j >= S ? j - S : 0)], v[k], acc1[k]);
        }
      }
      const bool second = oyl + 1 < nvy;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = 4 * g + k;
        if (col >= lo && col <= hi) {
          float *m = mid + (c * TOH + oyl) * MS + C::at(col - p0);
          m[0] = acc0[k];
          if (second) m[MS] = acc1[k];
        }
      }
    }
  }
  __syncthreads();

  // ---- 2. columns of the window outside the frame: copies of their reflections (the branch is uniform over the workgroup)
  if (p0 < 0 || p1 > W - 1) {
    const int nl = lo - p0, ne = nl + (p1 - hi);
    for (int item = tid; item < 3 * nvy * ne; item += 256) {
      const int cr = item / ne, e = item - cr * ne;
      const int c = cr / nvy, oyl = cr - c * nvy;
      const int p = e < nl ? p0 + e : hi + 1 + (e - nl);
      const int q = min(max(refl_index(p, W), lo), hi);
      float *m = mid + (c * TOH + oyl) * MS;
      m[C::at(p - p0)] = m[C::at(q - p0)];
    }
  }
  __syncthreads();

  // ---- 3. horizontal pass: mid -> outt
  for (int item = tid; item < 3 * nvy * nvx; item += 256) {
    const int cr = item / nvx, oxl = item - cr * nvx;
    const int c = cr / nvy, oyl = cr - c * nvy;
    const float *m = mid + (c * TOH + oyl) * MS + (C::PH == 1 ? oxl * S : oxl);
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc = __builtin_fmaf(a.g[G0 + t], m[C::at(t)], acc);  // at(s x + t) = at(t) + (x or s x)
    outt[(c * TOH + oyl) * OS + oxl] = acc;
  }
  __syncthreads();

  // ---- 4. store
  const int ho = a.ho, wo = a.wo;
  if (!a.out_u8) {
    float *dst = static_cast<float *>(a.dst) + (int64_t)img * 3 * ho * wo;
    if (a.dst_vec) {  // wo % 4 == 0: a group of 4 columns lies inside the frame or outside it
      constexpr int gq = TOW >> 2;
      for (int item = tid; item < 3 * nvy * gq; item += 256) {
        const int cr = item / gq, oxl = 4 * (item - cr * gq);
        const int c = cr / nvy, oyl = cr - c * nvy;
        if (ox0 + oxl >= wo) continue;
        const float *o = outt + (c * TOH + oyl) * OS + oxl;
        const f32x4 v = {o[0], o[1], o[2], o[3]};
        *reinterpret_cast<f32x4 *>(dst + ((int64_t)c * ho + oy0 + oyl) * wo + ox0 + oxl) = v;
      }
    } else {
      for (int item = tid; item < 3 * nvy * nvx; item += 256) {
        const int cr = item / nvx, oxl = item - cr * nvx;
        const int c = cr / nvy, oyl = cr - c * nvy;
        dst[((int64_t)c * ho + oy0 + oyl) * wo + ox0 + oxl] = outt[(c * TOH + oyl) * OS + oxl];
      }
    }
  } else {
    uint8_t *dst = static_cast<uint8_t *>(a.dst) + (int64_t)img * ho * wo * 3;
    if (a.dst_vec) {
      constexpr int gq = TOW >> 2;
      for (int item = tid; item < nvy * gq; item += 256) {
        const int oyl = item / gq, oxl = 4 * (item - oyl * gq);
        if (ox0 + oxl >= wo) continue;
        float v[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) v[c][i] = to_u8(outt[(c * TOH + oyl) * OS + oxl + i]);
        store_px4(dst + ((int64_t)(oy0 + oyl) * wo + ox0 + oxl) * 3, v, true);
      }
    } else {
      for (int item = tid; item < 3 * nvy * nvx; item += 256) {
        const int pr = item / 3, c = item - pr * 3;
        const int oyl = pr / nvx, oxl = pr - oyl * nvx;
        dst[((int64_t)(oy0 + oyl) * wo + ox0 + oxl) * 3 + c] = (uint8_t)(unsigned)to_u8(outt[(c * TOH + oyl) * OS + oxl]);
      }
    }
  }
}

static inline bool bd_aligned(const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

template <int S>
static void bd_dispatch(bool u8in, const BdArgs &a, int n, hipStream_t stream) {
  const dim3 grid(cdiv(a.wo, BdCfg<S>::TOW), cdiv(a.ho, BdCfg<S>::TOH), n);
  if (a.table) hipLaunchKernelGGL((bd_downsample_kernel<S, true, true>), grid, dim3(256), 0, stream, a);
  else if (u8in) hipLaunchKernelGGL((bd_downsample_kernel<S, true, false>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((bd_downsample_kernel<S, false, false>), grid, dim3(256), 0, stream, a);
}

// scipy.ndimage's 1-D Gaussian at sigma = 0.4 scale, truncated at int(4 sigma + 0.5), normalised; float64 here, float32 in the kernel
static void bd_kernel_weights(int scale, float *g) {
  const double sigma = 0.4 * scale;
  const int r = (int)(4.0 * sigma + 0.5);
  double w[13], sum = 0.0;
  for (int d = -6; d <= 6; ++d) sum += w[d + 6] = std::abs(d) <= r ? std::exp(-0.5 / (sigma * sigma) * d * d) : 0.0;
  for (int t = 0; t < 13; ++t) g[t] = (float)(w[t] / sum);
}

static int bd_launch(bool u8in, const void *src, void *dst, int n, int H, int W, int64_t src_img_stride, int ho, int wo, int scale, int out_u8,
                     edvr_stream_t stream) {
  EDVR_REQUIRE(src && dst && n > 0 && n <= 65535 && H > 0 && W > 0 && (u8in || n == 1 || src_img_stride >= 3 * (int64_t)H * W),
               "bd_downsample: bad arguments");
  EDVR_REQUIRE(scale >= 2 && scale <= 4, "bd_downsample: scale %d is not 2, 3 or 4", scale);
  EDVR_REQUIRE(std::min(H, W) >= 7, "bd_downsample: a %d x %d frame has fewer than 7 rows or columns, the reach of the 13-tap kernel's one reflection", H, W);
  EDVR_REQUIRE(ho == cdiv(H, scale) && wo == cdiv(W, scale), "bd_downsample: output %d x %d is not ceil(%d x %d / %d)", ho, wo, H, W, scale);
  EDVR_REQUIRE(cdiv(ho, 8) <= 65535 && (int64_t)H * W <= INT32_MAX / 4, "bd_downsample: a %d x %d frame is too large", H, W);
  BdArgs a;
  a.src = src, a.dst = dst, a.src_img_stride = src_img_stride, a.H = H, a.W = W, a.ho = ho, a.wo = wo, a.out_u8 = out_u8 != 0;
  bd_kernel_weights(scale, a.g);
  a.table = nullptr, a.wh = a.ww = a.pitch = 0;
  a.src_vec = u8in ? ((3 * (int64_t)W) % 16 == 0 && bd_aligned(src, 16)) : (W % 4 == 0 && src_img_stride % 4 == 0 && bd_aligned(src, 16));
  a.dst_vec = wo % 4 == 0 && bd_aligned(dst, a.out_u8 ? 4 : 16);
  if (scale == 2) bd_dispatch<2>(u8in, a, n, as_stream(stream));
  else if (scale == 3) bd_dispatch<3>(u8in, a, n, as_stream(stream));
  else bd_dispatch<4>(u8in, a, n, as_stream(stream));
  return check_launch("bd_downsample_kernel");
}

// n crops of p x p LQ samples from n windows of their GT frames (lq_window.h): the same kernel, the same tile, another view of the source
static int bd_windows_launch(const uint8_t *src, const int32_t *table, const int32_t *table_host, uint8_t *dst, int n, int p, int wh, int ww,
                             int pitch, int scale, edvr_stream_t stream) {
  EDVR_REQUIRE(src && table && dst, "bd_downsample_windows: bad arguments");
  const char *why = lqw_check(LQW_BD, scale, n, p, wh, ww, pitch, src, table_host);
  EDVR_REQUIRE(!why, "bd_downsample_windows: %s (n %d, crop %d, window %d x %d, pitch %d, scale %d)", why, n, p, wh, ww, pitch, scale);
  BdArgs a;
  a.src = src, a.dst = dst, a.src_img_stride = 0, a.H = a.W = 0, a.ho = a.wo = p, a.out_u8 = 1;
  bd_kernel_weights(scale, a.g);
  a.src_vec = 1;  // lqw_check: every window row starts on a 16-byte boundary and the pitch covers its last group
  a.dst_vec = p % 4 == 0 && bd_aligned(dst, 4);
  a.table = table, a.wh = wh, a.ww = ww, a.pitch = pitch;
  if (scale == 2) bd_dispatch<2>(true, a, n, as_stream(stream));
  else if (scale == 3) bd_dispatch<3>(true, a, n, as_stream(stream));
  else bd_dispatch<4>(true, a, n, as_stream(stream));
  return check_launch("bd_downsample_kernel (windows)");
}

}  // namespace edvr

extern "C" int edvr_bd_downsample_u8_windows(const uint8_t *src, const int32_t *table, const int32_t *table_host, uint8_t *dst, int n, int p,
                                             int wh, int ww, int pitch, int scale, edvr_stream_t stream) {
  return edvr::bd_windows_launch(src, table, table_host, dst, n, p, wh, ww, pitch, scale, stream);
}

extern "C" int edvr_bd_downsample_u8(const uint8_t *src, void *dst, int n, int H, int W, int ho, int wo, int scale, int out_u8,
                                     edvr_stream_t stream) {
  return edvr::bd_launch(true, src, dst, n, H, W, 0, ho, wo, scale, out_u8, stream);
}

extern "C" int edvr_bd_downsample_f32(const float *src, void *dst, int n, int H, int W, int64_t src_img_stride, int ho, int wo, int scale,
                                      int out_u8, edvr_stream_t stream) {
  return edvr::bd_launch(false, src, dst, n, H, W, src_img_stride, ho, wo, scale, out_u8, stream);
}
