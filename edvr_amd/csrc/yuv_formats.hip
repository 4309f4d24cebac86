// yuv_formats.hip - planar Y'CbCr of every Y4M format the container code accepts (4:2:0, 4:2:2, 4:4:4 at 8 ... 16 bits) <-> float32 RGB on
// the device: what yuv.hip does for 8-bit 4:2:0, for the footage that is not 8-bit 4:2:0 (10-bit phone and camera material, 4:2:2
// intermediates, 4:4:4 screen captures) and for an output that keeps more than 8 of the network's bits.  yuv.hip stays the 8-bit 4:2:0 path.
//
// Frame of (H, W), subsampling (sx, sy), depth d: the dense planes Y (H, W), Cb, Cr (Hc, Wc) = ((H + sy) >> sy, (W + sx) >> sx); a sample
// is a byte for d = 8, otherwise a little-endian 16-bit word.  A batch is n such frames `yuv_stride` BYTES apart; with 16-bit samples
// the base address and the stride are even (checked on the host: the kernels read and write words).
//
// Definition: that of yuv.hip with the offsets and the matrix scaled for the depth by the caller - the
// kernels see 12 floats and, in the encode, the largest sample 2^d - 1; nothing else depends on d, so the depth is a RUN-TIME argument
// and only the sample type (byte | word) is a template parameter.  Every product and sum is one float32 operation in the order written:
//   decode  the sample as read (bits above d are not masked), exactly a float; chroma upsampled along the SUBSAMPLED axes only:
//           'nearest' replicates, 'bilinear' is the centre-sited 1/4 - 3/4 filter, vertical (sy) then horizontal (sx), indices clamped;
//           d = (Y - yoff, Cb - coff, Cr - coff);  v_k = (Mi[k][0] d0 + Mi[k][1] d1) + Mi[k][2] d2;  clamp(v_k, 0, 255) / 255.0f
//   encode  x = clamp(f, 0, 1) * 255.0f (NaN -> 0);  p_k = ((M[k][0] r + M[k][1] g) + M[k][2] b) + off_k;  Y = rint(clamp(p_0, 0, 2^d - 1));
//           chroma 4:2:0 ((a + b) + (c + d)) * 0.25f, 4:2:2 (p[2l] + p[2l + 1]) * 0.5f, 4:4:4 p; row and column indices clamped to the
//           frame (an odd edge replicates); clamped to [0, 2^d - 1], rounded half to even.
//
// Kernel shape: as yuv.hip.  One thread owns 16 columns of one row pair (sy = 1) or of one row (sy = 0), so every luma sample, chroma
// sample and RGB float is loaded or stored by exactly one thread (the bilinear decode re-reads neighbouring chroma through the cache).
// The subsampling is a template parameter (it decides how many rows and chroma samples a thread holds in registers), as are the two
// access-width flags, both of which need W % 16 == 0: YV - 16-byte plane accesses (two per luma row of words; 8-byte ones for the 8
// chroma bytes of a subsampled row), where the batch base and stride are 16-byte aligned; RV - 16-byte float accesses.  The scalar
// forms clamp every load index into the plane and guard every store.  Consecutive threads own consecutive 16-column groups.  No LDS,
// 0 bytes of scratch.
#include <cstdint>

#include "common.h"

namespace edvr {

typedef float yf_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t yf_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t yf_u32x2 __attribute__((ext_vector_type(2)));

struct YuvFmtArgs {
  const void *src;
  void *dst;
  int64_t yuv_stride;  // BYTES between the frames of the batch
  int64_t rgb_stride;  // floats between images
  int H, W, Hc, Wc;
  int gw, hr, total;  // 16-column groups per row, row groups (pairs for sy = 1, rows for sy = 0) per frame, threads with work
  float m[9];         // decode: Mi, encode: M (row-major)
  float off[3];       // (yoff, coff, coff)
  float maxv;         // 2^d - 1
};

// (exact in float32 for 16-bit samples and weights 1/4, 3/4: 16 + 2 + 2 fractional bits after both passes)
__device__ __forceinline__ float yf_mix(float wa, float a, float wb, float b) { return __fadd_rn(__fmul_rn(wa, a), __fmul_rn(wb, b)); }
// a product rounded on its own (yuv_mul of yuv.hip: the empty asm keeps -ffp-contract=fast from fusing it into the add that consumes it)
__device__ __forceinline__ float yf_mul(float a, float b) {
  float p = __fmul_rn(a, b);
  asm volatile("" : "+v"(p));
  return p;
}
__device__ __forceinline__ float yf_dot(const float *m, float a, float b, float c) {
  return __fadd_rn(__fadd_rn(yf_mul(m[0], a), yf_mul(m[1], b)), yf_mul(m[2], c));
}
__device__ __forceinline__ uint32_t yf_sample(float v, float maxv) { return (uint32_t)rintf(fminf(fmaxf(v, 0.f), maxv)); }

// N samples of a plane row from column x0 as floats: whole 16-byte (8-byte for 8 bytes) accesses, or one by one with the column clamped
template <typename T, int N, bool VEC>
__device__ __forceinline__ void yf_load(const T *__restrict__ row, int x0, int w, float *v) {
  if (VEC) {
    constexpr int BYTES = N * (int)sizeof(T), PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    uint32_t q[BYTES / 4];
    if (BYTES == 8) {
      const yf_u32x2 t = *reinterpret_cast<const yf_u32x2 *>(row + x0);
      q[0] = t[0], q[1] = t[1];
    } else {
#pragma unroll
      for (int c = 0; c < BYTES / 16; ++c) {
        const yf_u32x4 t = reinterpret_cast<const yf_u32x4 *>(row + x0)[c];
        q[4 * c] = t[0], q[4 * c + 1] = t[1], q[4 * c + 2] = t[2], q[4 * c + 3] = t[3];
      }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = (float)((q[j / PER] >> (BITS * (j % PER))) & ((1u << BITS) - 1u));
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = (float)row[min(x0 + j, w - 1)];
  }
}

// chroma samples c0 - 1 ... c0 + CW of a plane row, v[j] = column clamp(c0 - 1 + j); the two outer ones only when HALO
template <typename T, int CW, bool VEC, bool HALO>
__device__ __forceinline__ void yf_load_chroma(const T *__restrict__ row, int c0, int wc, float (&v)[CW + 2]) {
  yf_load<T, CW, VEC>(row, c0, wc, v + 1);
  v[0] = HALO ? (float)row[max(c0 - 1, 0)] : 0.f;
  v[CW + 1] = HALO ? (float)row[min(c0 + CW, wc - 1)] : 0.f;
}

// N samples (each below 2^(8 sizeof(T))) to a plane row from column x0: whole accesses, or one by one where the column exists
template <typename T, int N, bool VEC>
__device__ __forceinline__ void yf_store(T *__restrict__ row, int x0, int w, const uint32_t *v) {
  if (VEC) {
    constexpr int BYTES = N * (int)sizeof(T), PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    uint32_t q[BYTES / 4];
#pragma unroll
    for (int j = 0; j < N; ++j) q[j / PER] = (j % PER) == 0 ? v[j] : (q[j / PER] | (v[j] << (BITS * (j % PER))));
    if (BYTES == 8) {
      const yf_u32x2 t = {q[0], q[1]};
      *reinterpret_cast<yf_u32x2 *>(row + x0) = t;
    } else {
#pragma unroll
      for (int c = 0; c < BYTES / 16; ++c) {
        const yf_u32x4 t = {q[4 * c], q[4 * c + 1], q[4 * c + 2], q[4 * c + 3]};
        reinterpret_cast<yf_u32x4 *>(row + x0)[c] = t;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (x0 + j < w) row[x0 + j] = (T)v[j];
  }
}

template <int SX, int SY, typename T, bool YV, bool RV, bool BIL>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const YuvFmtArgs a) {
  constexpr int R = 1 + SY, CW = 16 >> SX;  // rows and chroma samples per plane row of a thread
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= a.total) return;
  const int cg = item % a.gw, t = item / a.gw, rg = t % a.hr, img = t / a.hr;
  const int H = a.H, W = a.W, Hc = a.Hc, Wc = a.Wc;
  const T *yp = reinterpret_cast<const T *>(static_cast<const uint8_t *>(a.src) + (int64_t)img * a.yuv_stride);
  const int y0 = R * rg, x0 = 16 * cg, c0 = x0 >> SX;
  const bool second = SY && y0 + 1 < H;

  float ly[R][16];
  yf_load<T, 16, YV>(yp + (int64_t)y0 * W, x0, W, ly[0]);
  if constexpr (SY) yf_load<T, 16, YV>(yp + (int64_t)(second ? y0 + 1 : y0) * W, x0, W, ly[1]);

  // chroma after the vertical pass: cv[plane][row of the group][column c0 - 1 + j]; chroma row rg serves the whole group
  float cv[2][R][CW + 2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const T *plane = yp + (int64_t)H * W + (int64_t)p * Hc * Wc;
    float mid[CW + 2];
    yf_load_chroma<T, CW, YV, BIL && SX>(plane + (int64_t)rg * Wc, c0, Wc, mid);
    if constexpr (SY) {
      if (BIL) {
        float up[CW + 2], dn[CW + 2];
        yf_load_chroma<T, CW, YV, BIL && SX>(plane + (int64_t)max(rg - 1, 0) * Wc, c0, Wc, up);
        yf_load_chroma<T, CW, YV, BIL && SX>(plane + (int64_t)min(rg + 1, Hc - 1) * Wc, c0, Wc, dn);
#pragma unroll
        for (int j = 0; j < CW + 2; ++j) {
          cv[p][0][j] = yf_mix(0.25f, up[j], 0.75f, mid[j]);
          cv[p][1][j] = yf_mix(0.75f, mid[j], 0.25f, dn[j]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < CW + 2; ++j) cv[p][0][j] = cv[p][1][j] = mid[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < CW + 2; ++j) cv[p][0][j] = mid[j];
    }
  }

  float *img_dst = static_cast<float *>(a.dst) + (int64_t)img * a.rgb_stride;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r == 1 && !second) break;
    const int y = y0 + r;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float v[3][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int px = 4 * g + i, l = px >> SX;
        float c[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const float *s = cv[p][r];
          if (SX && BIL) c[p] = (px & 1) ? yf_mix(0.75f, s[l + 1], 0.25f, s[l + 2]) : yf_mix(0.25f, s[l], 0.75f, s[l + 1]);
          else c[p] = s[l + 1];
        }
        const float d0 = __fsub_rn(ly[r][px], a.off[0]);
        const float d1 = __fsub_rn(c[0], a.off[1]), d2 = __fsub_rn(c[1], a.off[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k][i] = __fdiv_rn(fminf(fmaxf(yf_dot(a.m + 3 * k, d0, d1, d2), 0.f), 255.f), 255.f);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float *o = img_dst + ((int64_t)k * H + y) * W + x0 + 4 * g;
        if (RV) {
          const yf_f32x4 s = {v[k][0], v[k][1], v[k][2], v[k][3]};
          *reinterpret_cast<yf_f32x4 *>(o) = s;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (x0 + 4 * g + i < W) o[i] = v[k][i];
        }
      }
    }
  }
}

template <int SX, int SY, typename T, bool YV, bool RV>
__global__ __launch_bounds__(256) void rgb_to_yuv_kernel(const YuvFmtArgs a) {
  constexpr int R = 1 + SY, CW = 16 >> SX;
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= a.total) return;
  const int cg = item % a.gw, t = item / a.gw, rg = t % a.hr, img = t / a.hr;
  const int H = a.H, W = a.W, Hc = a.Hc, Wc = a.Wc;
  const int y0 = R * rg, x0 = 16 * cg, c0 = x0 >> SX;
  const bool second = SY && y0 + 1 < H;
  const int ys[2] = {y0, second ? y0 + 1 : y0};  // an odd last row is its own partner
  const float *img_src = static_cast<const float *>(a.src) + (int64_t)img * a.rgb_stride;

  uint32_t yq[R][16], cq[2][CW];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float p[R][3][4];  // row, (Y, Cb, Cr), column
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float x[3][4];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float *s = img_src + ((int64_t)k * H + ys[r]) * W;
        yf_f32x4 w;
        if (RV) {
          w = *reinterpret_cast<const yf_f32x4 *>(s + x0 + 4 * g);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) w[i] = s[min(x0 + 4 * g + i, W - 1)];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) x[k][i] = __fmul_rn(fminf(fmaxf(w[i], 0.f), 1.f), 255.f);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) p[r][k][i] = __fadd_rn(yf_dot(a.m + 3 * k, x[0][i], x[1][i], x[2][i]), a.off[k]);
        yq[r][4 * g + i] = yf_sample(p[r][0][i], a.maxv);
      }
    }
#pragma unroll
    for (int k = 1; k < 3; ++k) {
      if constexpr (SX && SY) {
#pragma unroll
        for (int l = 0; l < 2; ++l)
          cq[k - 1][2 * g + l] = yf_sample(
              __fmul_rn(__fadd_rn(__fadd_rn(p[0][k][2 * l], p[0][k][2 * l + 1]), __fadd_rn(p[1][k][2 * l], p[1][k][2 * l + 1])), 0.25f), a.maxv);
      } else if constexpr (SX) {
#pragma unroll
        for (int l = 0; l < 2; ++l) cq[k - 1][2 * g + l] = yf_sample(__fmul_rn(__fadd_rn(p[0][k][2 * l], p[0][k][2 * l + 1]), 0.5f), a.maxv);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) cq[k - 1][4 * g + i] = yf_sample(p[0][k][i], a.maxv);
      }
    }
  }

  T *yp = reinterpret_cast<T *>(static_cast<uint8_t *>(a.dst) + (int64_t)img * a.yuv_stride);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r == 1 && !second) break;
    yf_store<T, 16, YV>(yp + (int64_t)(y0 + r) * W, x0, W, yq[r]);
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) yf_store<T, CW, YV>(yp + (int64_t)H * W + (int64_t)k * Hc * Wc + (int64_t)rg * Wc, c0, Wc, cq[k]);
}

static inline bool yf_aligned(const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// validates, fills the geometry and the two access-width flags; coef: 12 host floats, the matrix row-major, then the offsets
static int yf_fill(YuvFmtArgs &a, const char *what, const void *yuv, const void *rgb, int n, int H, int W, int sub_x, int sub_y, int depth,
                   int64_t yuv_stride, int64_t rgb_stride, const float *coef, bool &yv, bool &rv) {
  EDVR_REQUIRE(yuv && rgb && coef && n > 0 && H > 0 && W > 0, "%s: bad arguments", what);
  EDVR_REQUIRE(depth >= 8 && depth <= 16, "%s: a depth of %d bits is outside 8 ... 16", what, depth);
  EDVR_REQUIRE((sub_x == 1 && sub_y == 1) || (sub_x == 1 && sub_y == 0) || (sub_x == 0 && sub_y == 0),
               "%s: chroma subsampling (%d, %d) is none of 4:2:0 (1, 1), 4:2:2 (1, 0), 4:4:4 (0, 0)", what, sub_x, sub_y);
  EDVR_REQUIRE((int64_t)H * W <= INT32_MAX / 4, "%s: a %d x %d frame is too large", what, H, W);
  const int bps = depth > 8 ? 2 : 1;
  a.H = H, a.W = W, a.Hc = (H + sub_y) >> sub_y, a.Wc = (W + sub_x) >> sub_x;
  const int64_t framesize = ((int64_t)H * W + 2 * (int64_t)a.Hc * a.Wc) * bps;
  EDVR_REQUIRE(n == 1 || yuv_stride >= framesize, "%s: frames %lld bytes apart do not hold the %lld bytes of a %d x %d frame", what,
               (long long)yuv_stride, (long long)framesize, H, W);
  EDVR_REQUIRE(bps == 1 || (yf_aligned(yuv, 2) && (n == 1 || yuv_stride % 2 == 0)),
               "%s: 16-bit samples need an even base address and an even frame stride (%lld)", what, (long long)yuv_stride);
  EDVR_REQUIRE(n == 1 || rgb_stride >= 3 * (int64_t)H * W, "%s: images %lld floats apart overlap", what, (long long)rgb_stride);
  a.gw = cdiv(W, 16), a.hr = sub_y ? a.Hc : H;
  const int64_t total = (int64_t)n * a.hr * a.gw;
  EDVR_REQUIRE(total <= INT32_MAX - 256, "%s: %d frames of %d x %d are too many for one launch", what, n, H, W);
  a.total = (int)total;
  a.yuv_stride = yuv_stride, a.rgb_stride = rgb_stride;
  for (int i = 0; i < 9; ++i) a.m[i] = coef[i];
  for (int i = 0; i < 3; ++i) a.off[i] = coef[9 + i];
  a.maxv = (float)((1 << depth) - 1);
  // W % 16 == 0: H W and Hc Wc samples are multiples of 16 and 8, so every plane row starts as aligned as its accesses are wide
  const bool whole = W % 16 == 0;
  yv = whole && yf_aligned(yuv, 16) && (n == 1 || yuv_stride % 16 == 0);
  rv = whole && yf_aligned(rgb, 16) && (n == 1 || rgb_stride % 4 == 0);
  return EDVR_OK;
}

template <int SX, int SY, typename T, bool BIL>
static void yf_decode_launch(bool yv, bool rv, const YuvFmtArgs &a, hipStream_t stream) {
  const dim3 grid(cdiv(a.total, 256)), block(256);
  if (yv && rv) hipLaunchKernelGGL((yuv_to_rgb_kernel<SX, SY, T, true, true, BIL>), grid, block, 0, stream, a);
  else if (yv) hipLaunchKernelGGL((yuv_to_rgb_kernel<SX, SY, T, true, false, BIL>), grid, block, 0, stream, a);
  else if (rv) hipLaunchKernelGGL((yuv_to_rgb_kernel<SX, SY, T, false, true, BIL>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((yuv_to_rgb_kernel<SX, SY, T, false, false, BIL>), grid, block, 0, stream, a);
}

template <int SX, int SY, typename T>
static void yf_encode_launch(bool yv, bool rv, const YuvFmtArgs &a, hipStream_t stream) {
  const dim3 grid(cdiv(a.total, 256)), block(256);
  if (yv && rv) hipLaunchKernelGGL((rgb_to_yuv_kernel<SX, SY, T, true, true>), grid, block, 0, stream, a);
  else if (yv) hipLaunchKernelGGL((rgb_to_yuv_kernel<SX, SY, T, true, false>), grid, block, 0, stream, a);
  else if (rv) hipLaunchKernelGGL((rgb_to_yuv_kernel<SX, SY, T, false, true>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((rgb_to_yuv_kernel<SX, SY, T, false, false>), grid, block, 0, stream, a);
}

// (4:4:4 has nothing to filter: its one decode instance per sample type serves both values of `bilinear`)
template <int SX, int SY>
static void yf_decode_dispatch(bool wide, bool bil, bool yv, bool rv, const YuvFmtArgs &a, hipStream_t stream) {
  if (SX && bil) {
    if (wide) yf_decode_launch<SX, SY, uint16_t, SX != 0>(yv, rv, a, stream);
    else yf_decode_launch<SX, SY, uint8_t, SX != 0>(yv, rv, a, stream);
  } else {
    if (wide) yf_decode_launch<SX, SY, uint16_t, false>(yv, rv, a, stream);
    else yf_decode_launch<SX, SY, uint8_t, false>(yv, rv, a, stream);
  }
}

template <int SX, int SY>
static void yf_encode_dispatch(bool wide, bool yv, bool rv, const YuvFmtArgs &a, hipStream_t stream) {
  if (wide) yf_encode_launch<SX, SY, uint16_t>(yv, rv, a, stream);
  else yf_encode_launch<SX, SY, uint8_t>(yv, rv, a, stream);
}

}  // namespace edvr

extern "C" int edvr_yuv_to_rgb_f32(const uint8_t *yuv, float *rgb, int n, int H, int W, int sub_x, int sub_y, int depth, int64_t yuv_stride,
                                   int64_t rgb_img_stride, const float *coef, int bilinear, edvr_stream_t stream) {
  using namespace edvr;
  YuvFmtArgs a;
  bool yv, rv;
  const int rc = yf_fill(a, "yuv_to_rgb", yuv, rgb, n, H, W, sub_x, sub_y, depth, yuv_stride, rgb_img_stride, coef, yv, rv);
  if (rc != EDVR_OK) return rc;
  a.src = yuv, a.dst = rgb;
  const bool wide = depth > 8, bil = bilinear != 0;
  if (sub_y) yf_decode_dispatch<1, 1>(wide, bil, yv, rv, a, as_stream(stream));
  else if (sub_x) yf_decode_dispatch<1, 0>(wide, bil, yv, rv, a, as_stream(stream));
  else yf_decode_dispatch<0, 0>(wide, bil, yv, rv, a, as_stream(stream));
  return check_launch("yuv_to_rgb_kernel");
}

extern "C" int edvr_rgb_to_yuv_f32(const float *rgb, uint8_t *yuv, int n, int H, int W, int sub_x, int sub_y, int depth, int64_t rgb_img_stride,
                                   int64_t yuv_stride, const float *coef, edvr_stream_t stream) {
  using namespace edvr;
  YuvFmtArgs a;
  bool yv, rv;
  const int rc = yf_fill(a, "rgb_to_yuv", yuv, rgb, n, H, W, sub_x, sub_y, depth, yuv_stride, rgb_img_stride, coef, yv, rv);
  if (rc != EDVR_OK) return rc;
  a.src = rgb, a.dst = yuv;
  const bool wide = depth > 8;
  if (sub_y) yf_encode_dispatch<1, 1>(wide, yv, rv, a, as_stream(stream));
  else if (sub_x) yf_encode_dispatch<1, 0>(wide, yv, rv, a, as_stream(stream));
  else yf_encode_dispatch<0, 0>(wide, yv, rv, a, as_stream(stream));
  return check_launch("rgb_to_yuv_kernel");
}
