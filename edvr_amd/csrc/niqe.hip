// niqe.hip - the per-pixel part of NIQE (basicsr/metrics/niqe.py:10-205), the reference's no-reference metric, for gfx950.
//
// The reference converts the frame to Y on the host, runs two 7x7 scipy convolutions per scale for the MSCN map
// z = (x - mu) / (sigma + 1), cuts it into 96x96 blocks (48x48 at scale 2) and fits ten asymmetric generalised Gaussians per block.
// Every fit needs five numbers of its map only - sum of squares and count of the negative and of the positive values, sum of
// absolute values - so this kernel computes z for one block in LDS, forms the five maps (z and its four np.roll products) and
// reduces them to 25 doubles; the fits and the 36x36 algebra run on the host in float64 (edvr_amd/metrics.py: niqe_from_moments).
//
// z is float32 EXACTLY as NumPy computes it on float32 arrays (scipy.ndimage.convolve accumulates the 49 products in double, in
// row-major tap order, and rounds once): in a constant neighbourhood the reference gets z == 0 exactly and such pixels count on
// neither side; a float64 mu would leave +-1e-14 there and its sign would decide the counts.  -ffp-contract=fast is on, so every
// step is rounded on its own (mul_alone below where a product feeds an add): nothing may fuse.  The sums are float64 in a fixed order
// (the reference: float32 pairwise).
#include <cmath>

#include "common.h"
#include "pixel.h"  // to_u8, y_of_pixel / y_of_bytes

namespace edvr {

struct NiqeWindow {
  double q[4][4];  // window[3 +- i][3 +- j]: the 7x7 Gaussian is symmetric, 16 values travel in the kernel-argument block
};

constexpr int NIQE_B = 96;                 // block side at scale 1 (the reference's block_size_h / block_size_w)
constexpr int NIQE_R = 3;                  // window radius
constexpr int NIQE_STRIP = 32;             // rows of z per staging pass at scale 1 (24 at scale 2: 48 = 2 x 24)
constexpr int NIQE_SW = NIQE_B + 2 * NIQE_R;      // 102
constexpr int NIQE_SH = NIQE_STRIP + 2 * NIQE_R;  // 38

// A product rounded on its own.  __fmul_rn / __dmul_rn are a plain `*` to the compiler, and -ffp-contract=fast fuses a `*` into the add or
// subtract that consumes it: m2 - mu * mu as one fma loses the rounding of mu * mu that NumPy performs, right where the subtraction
// cancels.  fma(a, b, +0) IS the rounded product (no product here is a negative zero: the window is positive, pixels are >= 0, mu * mu
// >= 0) and cannot be fused any further.
__device__ __forceinline__ float mul_alone(float a, float b) { return __builtin_fmaf(a, b, 0.f); }
__device__ __forceinline__ double mul_alone(double a, double b) { return __builtin_fma(a, b, 0.0); }

// one pixel of the scale-1 plane in [0, 255]: Y of an RGB pixel, or the byte of a 1-channel image
__device__ __forceinline__ float niqe_px(const float *__restrict__ p, int c, int64_t o, int64_t hw) {
  return c == 3 ? y_of_pixel(p, o, hw) : to_u8(p[o]);
}
__device__ __forceinline__ float niqe_px(const uint8_t *__restrict__ p, int, int64_t o, int64_t) {
  return y_of_bytes((float)p[3 * o], (float)p[3 * o + 1], (float)p[3 * o + 2]);  // interleaved (h, w, 3) RGB bytes
}

// S = 1 | 2.  (y0, x0): origin of the kept rectangle in the image; kh, kw: its size at scale 1 (multiples of 96)
template <int S, typename T>
__device__ __forceinline__ void niqe_block(const T *__restrict__ p, double *__restrict__ out, int c, int w, int64_t hw, int y0, int x0, int kh,
                                           int kw, int by, int bx, const NiqeWindow &win, float (*zt)[NIQE_B + 1], float (*strip)[NIQE_SW],
                                           double (*red)[25]) {
  constexpr int B = NIQE_B / S, ROWS = NIQE_STRIP - 8 * (S - 1), SH = ROWS + 2 * NIQE_R, SW = B + 2 * NIQE_R;
  static_assert(B % ROWS == 0 && SH <= NIQE_SH && SW <= NIQE_SW, "strip geometry");
  const int tid = threadIdx.x, sh = kh / S, sw = kw / S;  // the plane of this scale
  for (int r0 = 0; r0 < B; r0 += ROWS) {
    // ---- stage rows [by B + r0 - 3, + SH) x columns [bx B - 3, + SW) of this scale's plane; mode='nearest' replicates the edge of the
    // KEPT rectangle: the clamp never lets a cropped or discarded pixel in
    for (int e = tid; e < SH * SW; e += 256) {
      const int r = e / SW, q = e % SW;
      const int yy = min(max(by * B + r0 + r - NIQE_R, 0), sh - 1), xx = min(max(bx * B + q - NIQE_R, 0), sw - 1);
      float v;
      if (S == 1) {
        v = niqe_px(p, c, (int64_t)(y0 + yy) * w + (x0 + xx), hw);
      } else {
        // cv2.resize(img / 255., (w // 2, h // 2), INTER_LINEAR) * 255. at the exact factor 1/2: the 2x2 mean, in float32
        const int64_t o = (int64_t)(y0 + 2 * yy) * w + (x0 + 2 * xx);
        const float a = __fdiv_rn(niqe_px(p, c, o, hw), 255.f), b = __fdiv_rn(niqe_px(p, c, o + 1, hw), 255.f);
        const float cc = __fdiv_rn(niqe_px(p, c, o + w, hw), 255.f), d = __fdiv_rn(niqe_px(p, c, o + w + 1, hw), 255.f);
        v = __fmul_rn(__fmul_rn(__fadd_rn(__fadd_rn(a, b), __fadd_rn(cc, d)), 0.25f), 255.f);
      }
      strip[r][q] = v;
    }
    __syncthreads();
    // ---- z of ROWS x B pixels
    for (int e = tid; e < ROWS * B; e += 256) {
      const int r = e / B, q = e % B;
      double s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int ky = 0; ky < 7; ++ky)
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
          const double g = win.q[ky < 3 ? 3 - ky : ky - 3][kx < 3 ? 3 - kx : kx - 3];
          const float x = strip[r + ky][q + kx];
          s1 = __dadd_rn(s1, mul_alone(g, (double)x));
          s2 = __dadd_rn(s2, mul_alone(g, (double)__fmul_rn(x, x)));
        }
      const float x = strip[r + NIQE_R][q + NIQE_R], mu = (float)s1, m2 = (float)s2;
      const float sigma = sqrtf(fabsf(__fsub_rn(m2, mul_alone(mu, mu))));  // sqrtf: correctly rounded (__fsqrt_rn is the native approximation)
      zt[r0 + r][q] = __fdiv_rn(__fsub_rn(x, mu), __fadd_rn(sigma, 1.f));
    }
    __syncthreads();  // the strip is free again, and after the last pass z is complete
  }
  // ---- the five maps: z, z * np.roll(z, s) for s = [0,1], [1,0], [1,1], [1,-1] (the roll wraps inside the block)
  double sneg[5], spos[5], sabs[5];
  int nneg[5], npos[5];
#pragma unroll
  for (int m = 0; m < 5; ++m) sneg[m] = spos[m] = sabs[m] = 0.0, nneg[m] = npos[m] = 0;
  for (int e = tid; e < B * B; e += 256) {
    const int r = e / B, q = e % B;
    const int ru = r ? r - 1 : B - 1, ql = q ? q - 1 : B - 1, qr = q == B - 1 ? 0 : q + 1;
    const float z = zt[r][q];
    const float v[5] = {z, __fmul_rn(z, zt[r][ql]), __fmul_rn(z, zt[ru][q]), __fmul_rn(z, zt[ru][ql]), __fmul_rn(z, zt[ru][qr])};
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      const double sq = (double)__fmul_rn(v[m], v[m]);  // the reference squares in float32
      if (v[m] < 0.f) sneg[m] = __dadd_rn(sneg[m], sq), ++nneg[m];
      if (v[m] > 0.f) spos[m] = __dadd_rn(spos[m], sq), ++npos[m];
      sabs[m] = __dadd_rn(sabs[m], (double)fabsf(v[m]));
    }
  }
  // ---- fixed-order tree: lanes, then the four waves
#pragma unroll
  for (int m = 0; m < 5; ++m) {
    double t[5] = {sneg[m], (double)nneg[m], spos[m], (double)npos[m], sabs[m]};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) t[k] = __dadd_rn(t[k], __shfl_down(t[k], o, 64));
      if ((tid & 63) == 0) red[tid >> 6][m * 5 + k] = t[k];
    }
  }
  __syncthreads();
  if (tid < 25) out[tid] = __dadd_rn(__dadd_rn(red[0][tid], red[1][tid]), __dadd_rn(red[2][tid], red[3][tid]));
}

// grid (blocks, 2 scales, n images), 256 threads; block index = bx * nbh + by (the reference's idx_w-outer order)
template <typename T>
__global__ __launch_bounds__(256) void niqe_moments_kernel(const T *__restrict__ x, double *__restrict__ out, int c, int h, int w,
                                                           int64_t img_stride, int crop, int nbh, int nbw, const NiqeWindow win) {
  __shared__ float zt[NIQE_B][NIQE_B + 1];
  __shared__ float strip[NIQE_SH][NIQE_SW];
  __shared__ double red[4][25];
  const int blk = blockIdx.x, scale = blockIdx.y, img = blockIdx.z;
  const int bx = blk / nbh, by = blk % nbh;
  const T *p = x + (int64_t)img * img_stride;
  double *o = out + (((int64_t)img * 2 + scale) * gridDim.x + blk) * 25;
  const int64_t hw = (int64_t)h * w;
  if (scale == 0)
    niqe_block<1>(p, o, c, w, hw, crop, crop, nbh * NIQE_B, nbw * NIQE_B, by, bx, win, zt, strip, red);
  else
    niqe_block<2>(p, o, c, w, hw, crop, crop, nbh * NIQE_B, nbw * NIQE_B, by, bx, win, zt, strip, red);
}

static int niqe_grid(int h, int w, int crop, int &nbh, int &nbw) {
  if (crop < 0 || h <= 2 * crop || w <= 2 * crop) return nbh = nbw = 0;
  nbh = (h - 2 * crop) / NIQE_B, nbw = (w - 2 * crop) / NIQE_B;
  return nbh * nbw;
}

template <typename T>
static int niqe_launch(const T *x, double *out, int n, int c, int h, int w, int64_t img_stride, int crop, hipStream_t stream) {
  int nbh, nbw;
  const int blocks = niqe_grid(h, w, crop, nbh, nbw);
  EDVR_REQUIRE(blocks > 0, "niqe: %dx%d with crop_border %d leaves no 96x96 block", h, w, crop);
  EDVR_REQUIRE(n <= 65535, "niqe: at most 65535 images per launch, got %d", n);
  // 7x7 Gaussian, sigma 7/6, normalised to sum 1 (MATLAB's fspecial('gaussian', 7, 7/6), the gaussian_window of the reference's
  // parameter file to 1.4e-17), in double on the host
  NiqeWindow win;
  double g[7][7], sum = 0.0;
  const double sigma = 7.0 / 6.0;
  for (int i = 0; i < 7; ++i)
    for (int j = 0; j < 7; ++j) sum += g[i][j] = std::exp(-((i - 3) * (i - 3) + (j - 3) * (j - 3)) / (2.0 * sigma * sigma));
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) win.q[i][j] = g[3 + i][3 + j] / sum;
  hipLaunchKernelGGL(niqe_moments_kernel<T>, dim3(blocks, 2, n), dim3(256), 0, stream, x, out, c, h, w, img_stride, crop, nbh, nbw, win);
  return check_launch("niqe_moments_kernel");
}

}  // namespace edvr

extern "C" {

size_t edvr_niqe_blocks(int h, int w, int crop_border) {
  int nbh, nbw;
  return (size_t)edvr::niqe_grid(h, w, crop_border, nbh, nbw);
}

int edvr_niqe_moments_f32(const float *x, double *out, int n, int c, int h, int w, int64_t img_stride, int crop_border, edvr_stream_t stream) {
  using namespace edvr;
  EDVR_REQUIRE(x && out && n > 0 && (c == 1 || c == 3) && h > 0 && w > 0, "niqe_moments: bad arguments");
  return niqe_launch(x, out, n, c, h, w, img_stride ? img_stride : (int64_t)c * h * w, crop_border, as_stream(stream));
}

int edvr_niqe_moments_u8(const uint8_t *x, double *out, int n, int h, int w, int64_t img_stride, int crop_border, edvr_stream_t stream) {
  using namespace edvr;
  EDVR_REQUIRE(x && out && n > 0 && h > 0 && w > 0, "niqe_moments: bad arguments");
  return niqe_launch(x, out, n, 3, h, w, img_stride ? img_stride : (int64_t)3 * h * w, crop_border, as_stream(stream));
}

}  // extern "C"
