// resample.hip - the network's float32 result at a stated size: separable resampling with tables, the stage
// between VideoRestorer and the one quantisation of rgb_to_yuv.  Unlike resize.hip (MATLAB's imresize: one scalar scale, symmetric
// extension, bicubic) the two axes have their own ratios and any of three kernels; the taps and weights of each axis come from the host
// (edvr_amd/resample.py: R1 - R5 in float64, rounded to float32), the arithmetic here is R4 and R6: columns first, then rows, every sum in
// float64 in tap order from 0, rounded to float32 once per pass.  A float32 x float32 product is exact in float64, so the contracted fma
// of the build and the multiply-and-add of the restatement (tests/resample_ref.py) agree bit for bit.
//
// ONE launch.  A workgroup owns a toh x tow OUTPUT tile of one image, every plane in turn:
//   0. the tile's table rows go to LDS once (weights of the columns as [tap][column]: lanes of a wave read neighbouring banks);
//   1. horizontal pass: thread = one output column x four of the clamped source rows [rlo, rlo + nrows) the tile's vertical taps reach
//      (one weight read per tap, four independent sums), taps read from global memory - scalar loads, or 16-byte loads of the aligned groups of 4 that hold its taps where the rows start
//      on 16-byte boundaries; the taps left and right of the frame read the edge sample (R4), in tap order either way, so the two paths
//      give the same bits.  The result goes to LDS `mid` as float32;
//   2. vertical pass: thread = 4 neighbouring output columns x one output row, one 16-byte LDS read per tap, four named accumulators;
//   3. one 16-byte store where the output rows start on 16-byte boundaries, up to four scalar stores otherwise.
// Tap loops have run-time bounds; nothing is indexed dynamically in registers (0 scratch).  Every index taken from a table is clamped
// before it addresses memory: a wrong table gives wrong samples, never an access outside the frame or the LDS.
#include <algorithm>

#include "common.h"

namespace edvr {

typedef float rs_f32x4 __attribute__((ext_vector_type(4)));

constexpr int RESAMPLE_MAX_TAPS = 49;       // ceil(2 * 3 * 8) + 1: lanczos3 at the ratio 8
constexpr int RESAMPLE_TOW = 64;            // columns of a tile: one wave per row of the horizontal pass
constexpr size_t RESAMPLE_LDS = 64 * 1024;  // what resize_tile keeps to

struct ResampleArgs {
  const float *src;
  float *dst;
  int64_t src_img_stride, dst_img_stride;
  const int32_t *fy, *fx;  // first tap of every output row / column
  const float *wy, *wx;    // [Ho][Ty], [Wo][Tx]
  int c, H, W, Ho, Wo, Ty, Tx;
  int toh, tow;  // output tile (tow % 4 == 0)
  int mrows;     // rows of `mid`: at least the source rows a tile's vertical taps reach
  int src_vec, dst_vec;
};

__global__ __launch_bounds__(256) void resample_kernel(const ResampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rs_smem[];
  const int toh = a.toh, tow = a.tow, Ty = a.Ty, Tx = a.Tx, H = a.H, W = a.W, Ho = a.Ho, Wo = a.Wo;
  float *mid = rs_smem;                                   // [mrows][tow]
  float *swx = mid + a.mrows * tow;                       // [Tx][tow]
  float *swy = swx + Tx * tow;                            // [toh][Ty]
  int *sfx = reinterpret_cast<int *>(swy + toh * Ty);     // [tow]
  int *sfy = sfx + tow;                                   // [toh]
  int bx, by, img;
  xcd_block_index(bx, by, img);
  const int oy0 = by * toh, ox0 = bx * tow;
  const int nvy = min(toh, Ho - oy0), nvx = min(tow, Wo - ox0);
  const int tid = threadIdx.x;

  // ---- 0. the tile's table rows; a first tap beyond the frame by a whole row of taps reads the edge alone, as any further one would
  for (int i = tid; i < nvx * Tx; i += 256) {
    const int t = i / nvx, j = i - t * nvx;
    swx[t * tow + j] = a.wx[(int64_t)(ox0 + j) * Tx + t];
  }
  for (int i = tid; i < nvy * Ty; i += 256) swy[i] = a.wy[(int64_t)oy0 * Ty + i];
  if (tid < nvx) sfx[tid] = min(max(a.fx[ox0 + tid], -Tx), W);
  if (tid >= 64 && tid - 64 < nvy) sfy[tid - 64] = min(max(a.fy[oy0 + tid - 64], -Ty), H);
  __syncthreads();

  // the clamped source rows the tile's vertical taps reach
  const int rlo = min(max(sfy[0], 0), H - 1);
  const int rhi = min(max(sfy[nvy - 1] + Ty - 1, 0), H - 1);
  const int nrows = min(max(rhi - rlo + 1, 1), a.mrows);
  const int gq = tow >> 2;

  for (int ch = 0; ch < a.c; ++ch) {
    const float *plane = a.src + (int64_t)img * a.src_img_stride + (int64_t)ch * H * W;
    // ---- 1. horizontal pass: global -> mid; a thread takes 4 source rows of its column: one weight read per tap, four independent sums
    const int nq = (nrows + 3) >> 2;
    for (int item = tid; item < nq * nvx; item += 256) {
      const int q = item / nvx, j = item - q * nvx, r0 = 4 * q;
      const float *row0 = plane + (int64_t)(rlo + r0) * W;  // r0 < nrows; the rows past the last are read again, not stored
      const float *row1 = plane + (int64_t)(rlo + min(r0 + 1, nrows - 1)) * W;
      const float *row2 = plane + (int64_t)(rlo + min(r0 + 2, nrows - 1)) * W;
      const float *row3 = plane + (int64_t)(rlo + min(r0 + 3, nrows - 1)) * W;
      const float *w = swx + j;
      const int first = sfx[j];
      double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
      auto tap = [&](int t, float e0, float e1, float e2, float e3) {
        const double wt = (double)w[t * tow];
        acc0 = __builtin_fma(wt, (double)e0, acc0);
        acc1 = __builtin_fma(wt, (double)e1, acc1);
        acc2 = __builtin_fma(wt, (double)e2, acc2);
        acc3 = __builtin_fma(wt, (double)e3, acc3);
      };
      if (a.src_vec) {
        int t = 0;
        const int nl = min(Tx, max(-first, 0));  // taps left of the frame
        if (nl > 0) {
          const float e0 = row0[0], e1 = row1[0], e2 = row2[0], e3 = row3[0];
          for (; t < nl; ++t) tap(t, e0, e1, e2, e3);
        }
        if (t < Tx) {  // first + t >= 0 here
          const int lo = first + t, hi = min(first + Tx - 1, W - 1);
          for (int g = lo >> 2; 4 * g <= hi; ++g) {  // W % 4 == 0: a group of 4 lies inside the row
            const rs_f32x4 v0 = *reinterpret_cast<const rs_f32x4 *>(row0 + 4 * g), v1 = *reinterpret_cast<const rs_f32x4 *>(row1 + 4 * g);
            const rs_f32x4 v2 = *reinterpret_cast<const rs_f32x4 *>(row2 + 4 * g), v3 = *reinterpret_cast<const rs_f32x4 *>(row3 + 4 * g);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int i = 4 * g + k;
              if (i >= lo && i <= hi) tap(i - first, v0[k], v1[k], v2[k], v3[k]);
            }
          }
          t = max(t, hi - first + 1);
          if (t < Tx) {  // taps right of the frame
            const float e0 = row0[W - 1], e1 = row1[W - 1], e2 = row2[W - 1], e3 = row3[W - 1];
            for (; t < Tx; ++t) tap(t, e0, e1, e2, e3);
          }
        }
      } else {
        for (int t = 0; t < Tx; ++t) {
          const int i = min(max(first + t, 0), W - 1);
          tap(t, row0[i], row1[i], row2[i], row3[i]);
        }
      }
      float *m = mid + r0 * tow + j;
      const int left = nrows - r0;
      m[0] = (float)acc0;
      if (left > 1) m[tow] = (float)acc1;
      if (left > 2) m[2 * tow] = (float)acc2;
      if (left > 3) m[3 * tow] = (float)acc3;
    }
    __syncthreads();

    // ---- 2. vertical pass: mid -> registers, 3. store
    float *oplane = a.dst + (int64_t)img * a.dst_img_stride + (int64_t)ch * Ho * Wo;
    for (int item = tid; item < nvy * gq; item += 256) {
      const int oyl = item / gq, oxl = 4 * (item - oyl * gq);
      if (oxl >= nvx) continue;
      const int first = sfy[oyl];
      const float *w = swy + oyl * Ty;
      double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
      for (int t = 0; t < Ty; ++t) {
        const int r = min(max(min(max(first + t, 0), H - 1) - rlo, 0), nrows - 1);
        const rs_f32x4 v = *reinterpret_cast<const rs_f32x4 *>(mid + r * tow + oxl);
        const double wt = (double)w[t];
        acc0 = __builtin_fma(wt, (double)v[0], acc0);
        acc1 = __builtin_fma(wt, (double)v[1], acc1);
        acc2 = __builtin_fma(wt, (double)v[2], acc2);
        acc3 = __builtin_fma(wt, (double)v[3], acc3);
      }
      float *o = oplane + (int64_t)(oy0 + oyl) * Wo + ox0 + oxl;
      if (a.dst_vec) {  // Wo % 4 == 0: a group of 4 columns lies inside the frame or outside it
        const rs_f32x4 v = {(float)acc0, (float)acc1, (float)acc2, (float)acc3};
        *reinterpret_cast<rs_f32x4 *>(o) = v;
      } else {
        const int left = nvx - oxl;
        o[0] = (float)acc0;
        if (left > 1) o[1] = (float)acc1;
        if (left > 2) o[2] = (float)acc2;
        if (left > 3) o[3] = (float)acc3;
      }
    }
    __syncthreads();  // the next plane's horizontal pass overwrites mid
  }
}

static inline bool resample_aligned(const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// Tile: 64 columns; as many rows, from 32 down, as keep the LDS within 64 KB.  The rows of `mid` are the source rows the vertical taps of
// toh output rows reach: first taps spread over at most ceil((toh - 1) H / Ho) rows (R2, R3) plus Ty - so toh shrinks as H / Ho grows
// toward 8: 32 up to a ratio of about 5.5 with lanczos3, 16 from there on.  Sets toh, tow, mrows; returns the bytes of LDS.
static size_t resample_tile(int H, int Ho, int Ty, int Tx, int &toh, int &tow, int &mrows) {
  tow = RESAMPLE_TOW;
  size_t lds = 0;
  for (toh = 32; toh >= 1; toh >>= 1) {
    mrows = (int)std::min<int64_t>(H, cdiv64((int64_t)(toh - 1) * H, Ho) + Ty);
    lds = sizeof(float) * ((size_t)mrows * tow + (size_t)Tx * tow + (size_t)toh * Ty + tow + toh);
    if (lds <= RESAMPLE_LDS) break;
  }
  return lds;
}

static bool resample_geometry(int H, int W, int Ho, int Wo, int Ty, int Tx) {
  return H > 0 && W > 0 && Ho > 0 && Wo > 0 && Ty >= 1 && Ty <= RESAMPLE_MAX_TAPS && Tx >= 1 && Tx <= RESAMPLE_MAX_TAPS;
}

static bool resample_ratio(int in, int out) { return (int64_t)in <= 8 * (int64_t)out && (int64_t)out <= 8 * (int64_t)in; }

}  // namespace edvr

extern "C" int edvr_resample_tile(int H, int W, int Ho, int Wo, int Ty, int Tx, int *toh, int *tow) {
  EDVR_REQUIRE(toh && tow && edvr::resample_geometry(H, W, Ho, Wo, Ty, Tx), "resample_tile: bad arguments (taps are 1 ... 49)");
  EDVR_REQUIRE(edvr::resample_ratio(H, Ho) && edvr::resample_ratio(W, Wo), "resample_tile: %d x %d -> %d x %d has a ratio outside [1/8, 8]", H, W,
               Ho, Wo);
  int mrows;
  edvr::resample_tile(H, Ho, Ty, Tx, *toh, *tow, mrows);
  return EDVR_OK;
}

extern "C" int edvr_resample_f32(const float *src, float *dst, int n, int c, int H, int W, int64_t src_img_stride, int Ho, int Wo,
                                 int64_t dst_img_stride, const int32_t *fy, const float *wy, int Ty, const int32_t *fx, const float *wx, int Tx,
                                 edvr_stream_t stream) {
  using namespace edvr;
  EDVR_REQUIRE(src && dst && fy && wy && fx && wx, "resample: null pointer");
  EDVR_REQUIRE(n >= 1 && n <= 65535 && c >= 1, "resample: %d images of %d planes (1 ... 65535 images, at least one plane)", n, c);
  EDVR_REQUIRE(resample_geometry(H, W, Ho, Wo, Ty, Tx), "resample: bad size %d x %d -> %d x %d or taps %d, %d outside 1 ... 49", H, W, Ho, Wo, Ty, Tx);
  EDVR_REQUIRE(resample_ratio(H, Ho) && resample_ratio(W, Wo), "resample: %d x %d -> %d x %d has a ratio outside [1/8, 8]", H, W, Ho, Wo);
  EDVR_REQUIRE(src_img_stride >= (int64_t)c * H * W && dst_img_stride >= (int64_t)c * Ho * Wo, "resample: an image stride is smaller than an image");
  ResampleArgs a;
  a.src = src, a.dst = dst, a.src_img_stride = src_img_stride, a.dst_img_stride = dst_img_stride;
  a.fy = fy, a.fx = fx, a.wy = wy, a.wx = wx;
  a.c = c, a.H = H, a.W = W, a.Ho = Ho, a.Wo = Wo, a.Ty = Ty, a.Tx = Tx;
  const size_t lds = resample_tile(H, Ho, Ty, Tx, a.toh, a.tow, a.mrows);
  EDVR_REQUIRE(lds <= RESAMPLE_LDS && cdiv(Ho, a.toh) <= 65535, "resample: no tile for %d -> %d rows with %d taps", H, Ho, Ty);
  a.src_vec = W % 4 == 0 && src_img_stride % 4 == 0 && resample_aligned(src, 16);
  a.dst_vec = Wo % 4 == 0 && dst_img_stride % 4 == 0 && resample_aligned(dst, 16);
  hipLaunchKernelGGL(resample_kernel, dim3(cdiv(Wo, a.tow), cdiv(Ho, a.toh), n), dim3(256), lds, as_stream(stream), a);
  return check_launch("resample_kernel");
}
