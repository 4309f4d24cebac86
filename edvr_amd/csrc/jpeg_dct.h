// jpeg_dct.h - the device helpers the block-DCT codecs share (jpeg.hip, mpeg.hip): the 13-bit Loeffler DCT both ways, the integer colour
// conversion and the 4-pixel row accesses of DESIGN 4.16.  All arithmetic is 32-bit integer.
#pragma once
#include "common.h"

namespace edvr {

__device__ __forceinline__ int jm(int x, int c) { return __mul24(x, c); }
__device__ __forceinline__ int jd(int x, int k) { return (x + (1 << (k - 1))) >> k; }
__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// the odd part both transforms share: (t4, t5, t6, t7) -> the four sums before the final descale, in place
__device__ __forceinline__ void jpeg_odd(int &t4, int &t5, int &t6, int &t7) {
  int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = jm(z3 + z4, 9633);
  t4 = jm(t4, 2446), t5 = jm(t5, 16819), t6 = jm(t6, 25172), t7 = jm(t7, 12299);
  z1 = jm(z1, -7373), z2 = jm(z2, -20995), z3 = jm(z3, -16069) + z5, z4 = jm(z4, -3196) + z5;
  t4 += z1 + z3, t5 += z2 + z4, t6 += z2 + z3, t7 += z1 + z4;
}

template <bool ROWS>
__device__ __forceinline__ void jpeg_fdct8(int (&d)[8]) {
  constexpr int K = ROWS ? 11 : 15;
  const int t0 = d[0] + d[7], t1 = d[1] + d[6], t2 = d[2] + d[5], t3 = d[3] + d[4];
  int t7 = d[0] - d[7], t6 = d[1] - d[6], t5 = d[2] - d[5], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = ROWS ? (t10 + t11) << 2 : jd(t10 + t11, 2);
  d[4] = ROWS ? (t10 - t11) << 2 : jd(t10 - t11, 2);
  const int z = jm(t12 + t13, 4433);
  d[2] = jd(z + jm(t13, 6270), K);
  d[6] = jd(z - jm(t12, 15137), K);
  jpeg_odd(t4, t5, t6, t7);
  d[7] = jd(t4, K), d[5] = jd(t5, K), d[3] = jd(t6, K), d[1] = jd(t7, K);
}

template <int K>
__device__ __forceinline__ void jpeg_idct8(int (&c)[8]) {
  const int z = jm(c[2] + c[6], 4433);
  const int e2 = z - jm(c[6], 15137), e3 = z + jm(c[2], 6270);
  const int e0 = (c[0] + c[4]) << 13, e1 = (c[0] - c[4]) << 13;
  const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  int t0 = c[7], t1 = c[5], t2 = c[3], t3 = c[1];
  jpeg_odd(t0, t1, t2, t3);
  c[0] = jd(t10 + t3, K), c[7] = jd(t10 - t3, K);
  c[1] = jd(t11 + t2, K), c[6] = jd(t11 - t2, K);
  c[2] = jd(t12 + t1, K), c[5] = jd(t12 - t1, K);
  c[3] = jd(t13 + t0, K), c[4] = jd(t13 - t0, K);
}

// 4 pixels px .. px + 3 of a row of W pixels, columns clamped to the row (the padding of the definition's step 2)
__device__ __forceinline__ void jpeg_load4(const uint8_t *__restrict__ row, int px, int W, bool vec, int (&r)[4], int (&g)[4], int (&b)[4]) {
  if (vec && px >= 0 && px + 3 < W) {
    const uint32_t *p = reinterpret_cast<const uint32_t *>(row + 3 * (int64_t)px);
    const uint32_t u0 = p[0], u1 = p[1], u2 = p[2];
    r[0] = u0 & 255, g[0] = (u0 >> 8) & 255, b[0] = (u0 >> 16) & 255, r[1] = u0 >> 24;
    g[1] = u1 & 255, b[1] = (u1 >> 8) & 255, r[2] = (u1 >> 16) & 255, g[2] = u1 >> 24;
    b[2] = u2 & 255, r[3] = (u2 >> 8) & 255, g[3] = (u2 >> 16) & 255, b[3] = u2 >> 24;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint8_t *p = row + 3 * (int64_t)min(max(px + i, 0), W - 1);
      r[i] = p[0], g[i] = p[1], b[i] = p[2];
    }
  }
}

// pixels px .. px + 3 of a row of W pixels, those inside the row; v[i] = R | G << 8 | B << 16
__device__ __forceinline__ void jpeg_store4(uint8_t *__restrict__ row, int px, int W, bool vec, const uint32_t (&v)[4]) {
  if (vec && px + 3 < W) {
    uint32_t *p = reinterpret_cast<uint32_t *>(row + 3 * (int64_t)px);
    p[0] = v[0] | (v[1] << 24), p[1] = (v[1] >> 8) | (v[2] << 16), p[2] = (v[2] >> 16) | (v[3] << 8);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (px + i < W) {
        uint8_t *p = row + 3 * (int64_t)(px + i);
        p[0] = (uint8_t)(v[i] & 255), p[1] = (uint8_t)((v[i] >> 8) & 255), p[2] = (uint8_t)(v[i] >> 16);
      }
  }
}

__device__ __forceinline__ int jpeg_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int jpeg_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16; }
__device__ __forceinline__ int jpeg_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16; }

__device__ __forceinline__ uint32_t jpeg_rgb(int y, int cb, int cr) {
  cb -= 128, cr -= 128;
  const int r = clamp255(y + ((91881 * cr + 32768) >> 16));
  const int g = clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  const int b = clamp255(y + ((116130 * cb + 32768) >> 16));
  return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}

static inline bool jpeg_aligned4(const void *p, int64_t stride, int n) {
  return reinterpret_cast<uintptr_t>(p) % 4 == 0 && (n == 1 || stride % 4 == 0);
}

}  // namespace edvr
