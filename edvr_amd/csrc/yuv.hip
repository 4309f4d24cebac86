// yuv.hip - planar Y'CbCr of every Y4M format the container code accepts (4:2:0, 4:2:2, 4:4:4 at 8 ... 16 bits) <-> RGB on the device, both
// directions, so that decoded video reaches VideoRestorer without passing through RGB bytes on the host and the network's float32 result
// is quantised ONCE, to YUV samples.  One kernel family: 8-bit 4:2:0 (I420, what almost all footage is) is its <1, 1, uint8_t> instances.
//
// Frame of (H, W), subsampling (sx, sy), depth d: the dense planes Y (H, W), Cb, Cr (Hc, Wc) = ((H + sy) >> sy, (W + sx) >> sx) - the
// payload of a YUV4MPEG2 frame; a sample is a byte for d = 8, otherwise a little-endian 16-bit word.  A batch is n such frames
// `yuv_stride` BYTES apart at any base address (a Y4M read buffer: stride framesize + 6, base 6 past its start); with 16-bit samples the
// base address and the stride are even (checked on the host: the kernels read and write words).
// RGB is planar float32 (n, 3, H, W) in [0, 1] for every format or, for 8-bit 4:2:0 alone, interleaved uint8 (n, H, W, 3).
//
// Definition (depths and subsamplings: 4.14; chroma siting: 4.15).  M (3 x 3, RGB in 0 ... 255 -> Y, Cb, Cr without offsets), its inverse Mi and
// the offsets (yoff, coff, coff) are computed by the caller in float64 for the depth, rounded to float32 and arrive as kernel arguments -
// no tables.  The kernels see these 12 floats and, in the encode, the largest sample 2^d - 1; nothing else depends on d, so the depth is a
// RUN-TIME argument and only the sample type (byte | word) is a template parameter.  Every product and every sum below is one float32
// operation, rounded on its own, in the order written (yuv_mul keeps the products out of fused multiply-adds):
//   decode  the sample as read (bits above d are not masked), exactly a float; chroma upsampled along the SUBSAMPLED axes only:
//           'nearest' replicates (plane[i >> sy][j >> sx]); 'bilinear' (centre-sited) per axis, indices clamped to the plane,
//           even 2k: 0.25 c[k - 1] + 0.75 c[k], odd 2k + 1: 0.75 c[k] + 0.25 c[k + 1], vertical (sy) then horizontal (sx) (exact in float32);
//           d = (Y - yoff, Cb - coff, Cr - coff);  v_k = (Mi[k][0] d0 + Mi[k][1] d1) + Mi[k][2] d2
//           float32 (n, 3, H, W): clamp(v_k, 0, 255) / 255.0f      uint8 (n, H, W, 3): rint(clamp(v_k, 0, 255))
//   encode  x = clamp(f, 0, 1) * 255.0f (float32 (n, 3, H, W), NaN -> 0 as to_u8 of pixel.h) or the byte (uint8 (n, H, W, 3));
//           p_k = ((M[k][0] r + M[k][1] g) + M[k][2] b) + off_k;  Y = rint(clamp(p_0, 0, 2^d - 1));
//           chroma 4:2:0 (k, l) = ((p[2k][2l] + p[2k][2l + 1]) + (p[2k + 1][2l] + p[2k + 1][2l + 1])) * 0.25f, 4:2:2 (p[2l] + p[2l + 1]) * 0.5f,
//           4:4:4 p; row and column indices clamped to the frame (an odd edge replicates); clamped to [0, 2^d - 1], rounded half to even.
//   siting  per SUBSAMPLED axis, centre (everything above: chroma sample k lies between luma samples 2k and 2k + 1) or co-sited (on luma
//           sample 2k): 'left' = co-sited columns (H.264 / HEVC / AV1 4:2:0, every 4:2:2), 'topleft' = co-sited columns and rows (BT.2020).
//           decode, co-sited axis: even 2k: c[k], odd 2k + 1: 0.5 c[k] + 0.5 c[k + 1] - the two-tap form above with other weights, so the
//           four weights per axis are RUN-TIME arguments (wv, wh) and every siting runs the same decode instances; centre through them
//           is the same float32 value (the weights are the same constants).
//           encode, co-sited axis: [1 2 1] / 4 around luma sample 2k.  Horizontal first, un-normalised: co-sited h[r][l] = (p[r][2l - 1] +
//           p[r][2l + 1]) + (p[r][2l] + p[r][2l]) (scale 4), centre h[r][l] = p[r][2l] + p[r][2l + 1] (scale 2); then vertical over h:
//           co-sited (h[2k - 1] + h[2k + 1]) + (h[2k] + h[2k]) (4), centre h[2k] + h[2k + 1] (2), 4:2:2 h[r] (1); then ONE product with the
//           reciprocal of the scales' product (a power of two), clamp, round.  Indices clamped to the frame.  Both axes centred: the
//           expression above, bit for bit.  The co-sited axes are template parameters (CX, CY) of the subsampled encode instances.
//
// Kernel shape: both kernels move samples and nothing else.  One thread owns 16 columns of one row pair (sy = 1) or of one row (sy = 0),
// so every luma sample, chroma sample and RGB sample is loaded or stored by exactly one thread (the bilinear decode re-reads the
// neighbouring chroma rows and one sample left and right of its own through the cache: at 4:2:0, 1/4 of a sample per pixel and plane;
// the co-sited encode recomputes, from RGB read through the cache, Cb / Cr of the column left of its 16 (CX: one scalar pixel per row) and
// the row above its pair (CY: that row's 16 columns, with the 16-byte loads where RV)).
// The subsampling is a template parameter (it decides how many rows and chroma samples a thread holds in registers), as are the RGB side
// (U8; its staging arrays exist in those instances only) and two flags that pick the access width per side, both of which need
// W % 16 == 0 (every thread's 16 columns are whole): YV - 16-byte plane accesses (two per luma row of words; 8-byte ones for the 8 chroma
// bytes of a subsampled row), where the batch base and stride are 16-byte aligned; RV - 16-byte float / packed RGB byte accesses, where
// the RGB tensor is.  The scalar forms clamp every load index into the plane and guard every store, and cover odd sizes, W % 16 != 0 and
// the 6-byte offset of a Y4M buffer.  Consecutive threads own consecutive 16-column groups.  No LDS, 0 bytes of scratch.
#include <cstdint>

#include "common.h"

namespace edvr {

typedef float yuv_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t yuv_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t yuv_u32x2 __attribute__((ext_vector_type(2)));

struct YuvArgs {
  const void *src;
  void *dst;
  int64_t yuv_stride;  // BYTES between the frames of the batch
  int64_t rgb_stride;  // float RGB: floats between images; byte RGB: dense
  int H, W, Hc, Wc;
  int gw, hr, total;  // 16-column groups per row, row groups (pairs for sy = 1, rows for sy = 0) per frame, threads with work
  float m[9];         // decode: Mi, encode: M (row-major)
  float off[3];       // (yoff, coff, coff)
  float maxv;         // 2^d - 1 (read by the instances with 16-bit samples)
  // bilinear decode, per axis (v: rows, h: columns): even 2k = w[0] c[k - 1] + w[1] c[k], odd 2k + 1 = w[2] c[k] + w[3] c[k + 1]
  float wv[4], wh[4];
};

// (exact in float32 for 16-bit samples and weights 0, 1/4, 1/2, 3/4, 1 - 16 + 2 + 2 fractional bits after both passes: fused or not, the
// same value)
__device__ __forceinline__ float yuv_mix(float wa, float a, float wb, float b) { return __fadd_rn(__fmul_rn(wa, a), __fmul_rn(wb, b)); }
// a product rounded on its own: __fmul_rn is a plain `*` to the compiler, and -ffp-contract=fast would fuse it into the add that
// consumes it; the empty asm keeps the two apart (as accumulate_weighted of ensemble.hip does)
__device__ __forceinline__ float yuv_mul(float a, float b) {
  float p = __fmul_rn(a, b);
  asm volatile("" : "+v"(p));
  return p;
}
__device__ __forceinline__ float yuv_dot(const float *m, float a, float b, float c) {
  return __fadd_rn(__fadd_rn(yuv_mul(m[0], a), yuv_mul(m[1], b)), yuv_mul(m[2], c));
}
__device__ __forceinline__ uint32_t yuv_sample(float v, float maxv) { return (uint32_t)rintf(fminf(fmaxf(v, 0.f), maxv)); }

// N samples of a plane row from column x0 as floats: whole 16-byte (8-byte for 8 bytes) accesses, or one by one with the column clamped
template <typename T, int N, bool VEC>
__device__ __forceinline__ void yuv_load(const T *__restrict__ row, int x0, int w, float *v) {
  if (VEC) {
    constexpr int BYTES = N * (int)sizeof(T), PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    uint32_t q[BYTES / 4];
    if (BYTES == 8) {
      const yuv_u32x2 t = *reinterpret_cast<const yuv_u32x2 *>(row + x0);
      q[0] = t[0], q[1] = t[1];
    } else {
#pragma unroll
      for (int c = 0; c < BYTES / 16; ++c) {
        const yuv_u32x4 t = reinterpret_cast<const yuv_u32x4 *>(row + x0)[c];
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
__device__ __forceinline__ void yuv_load_chroma(const T *__restrict__ row, int c0, int wc, float (&v)[CW + 2]) {
  yuv_load<T, CW, VEC>(row, c0, wc, v + 1);
  v[0] = HALO ? (float)row[max(c0 - 1, 0)] : 0.f;
  v[CW + 1] = HALO ? (float)row[min(c0 + CW, wc - 1)] : 0.f;
}

// N samples (each below 2^(8 sizeof(T))) to a plane row from column x0: whole accesses, or one by one where the column exists
template <typename T, int N, bool VEC>
__device__ __forceinline__ void yuv_store(T *__restrict__ row, int x0, int w, const uint32_t *v) {
  if (VEC) {
    constexpr int BYTES = N * (int)sizeof(T), PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    uint32_t q[BYTES / 4];
#pragma unroll
    for (int j = 0; j < N; ++j) q[j / PER] = (j % PER) == 0 ? v[j] : (q[j / PER] | (v[j] << (BITS * (j % PER))));
    if (BYTES == 8) {
      const yuv_u32x2 t = {q[0], q[1]};
      *reinterpret_cast<yuv_u32x2 *>(row + x0) = t;
    } else {
#pragma unroll
      for (int c = 0; c < BYTES / 16; ++c) {
        const yuv_u32x4 t = {q[4 * c], q[4 * c + 1], q[4 * c + 2], q[4 * c + 3]};
        reinterpret_cast<yuv_u32x4 *>(row + x0)[c] = t;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (x0 + j < w) row[x0 + j] = (T)v[j];
  }
}

// columns 4 g ... 4 g + 3 of a thread's 16 as the RGB tensor holds them, v[channel][column]: from the luma row and, after the vertical
// pass, the two chroma rows (s[j] = chroma column c0 - 1 + j)
template <int SX, bool BIL, bool U8>
__device__ __forceinline__ void yuv_pixels4(const YuvArgs &a, const float *ly, const float *cb, const float *cr, int g, float (&v)[3][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int px = 4 * g + i, l = px >> SX;
    float c[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const float *s = p ? cr : cb;
      if (SX && BIL) c[p] = (px & 1) ? yuv_mix(a.wh[2], s[l + 1], a.wh[3], s[l + 2]) : yuv_mix(a.wh[0], s[l], a.wh[1], s[l + 1]);
      else c[p] = s[l + 1];
    }
    const float d0 = __fsub_rn(ly[px], a.off[0]);
    const float d1 = __fsub_rn(c[0], a.off[1]), d2 = __fsub_rn(c[1], a.off[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float w = fminf(fmaxf(yuv_dot(a.m + 3 * k, d0, d1, d2), 0.f), 255.f);
      v[k][i] = U8 ? rintf(w) : __fdiv_rn(w, 255.f);
    }
  }
}

template <int SX, int SY, typename T, bool YV, bool RV, bool BIL, bool U8>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const YuvArgs a) {
  constexpr int R = 1 + SY, CW = 16 >> SX;  // rows and chroma samples per plane row of a thread
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= a.total) return;
  const int cg = item % a.gw, t = item / a.gw, rg = t % a.hr, img = t / a.hr;
  const int H = a.H, W = a.W, Hc = a.Hc, Wc = a.Wc;
  const T *yp = reinterpret_cast<const T *>(static_cast<const uint8_t *>(a.src) + (int64_t)img * a.yuv_stride);
  const int y0 = R * rg, x0 = 16 * cg, c0 = x0 >> SX;
  const bool second = SY && y0 + 1 < H;

  float ly[R][16];
  yuv_load<T, 16, YV>(yp + (int64_t)y0 * W, x0, W, ly[0]);
  if constexpr (SY) yuv_load<T, 16, YV>(yp + (int64_t)(second ? y0 + 1 : y0) * W, x0, W, ly[1]);

  // chroma after the vertical pass: cv[plane][row of the group][column c0 - 1 + j]; chroma row rg serves the whole group
  float cv[2][R][CW + 2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const T *plane = yp + (int64_t)H * W + (int64_t)p * Hc * Wc;
    float mid[CW + 2];
    yuv_load_chroma<T, CW, YV, BIL && SX>(plane + (int64_t)rg * Wc, c0, Wc, mid);
    if constexpr (SY) {
      if (BIL) {
        float up[CW + 2], dn[CW + 2];
        yuv_load_chroma<T, CW, YV, BIL && SX>(plane + (int64_t)max(rg - 1, 0) * Wc, c0, Wc, up);
        yuv_load_chroma<T, CW, YV, BIL && SX>(plane + (int64_t)min(rg + 1, Hc - 1) * Wc, c0, Wc, dn);
#pragma unroll
        for (int j = 0; j < CW + 2; ++j) {
          cv[p][0][j] = yuv_mix(a.wv[0], up[j], a.wv[1], mid[j]);
          cv[p][1][j] = yuv_mix(a.wv[2], mid[j], a.wv[3], dn[j]);
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

#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r == 1 && !second) break;
    const int y = y0 + r;
    if constexpr (U8) {
      uint8_t *row = static_cast<uint8_t *>(a.dst) + (((int64_t)img * H + y) * W + x0) * 3;
      uint32_t packed[12];  // RV: the 48 interleaved bytes of this row
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float v[3][4];
        yuv_pixels4<SX, BIL, U8>(a, ly[r], cv[0][r], cv[1][r], g, v);
        if (RV) {
#pragma unroll
          for (int b = 0; b < 12; ++b) {
            const uint32_t byte = (uint32_t)v[b % 3][b / 3];
            if (b % 4 == 0) packed[3 * g + b / 4] = byte;
            else packed[3 * g + b / 4] |= byte << (8 * (b % 4));
          }
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (x0 + 4 * g + i < W)
#pragma unroll
              for (int k = 0; k < 3; ++k) row[(4 * g + i) * 3 + k] = (uint8_t)(unsigned)v[k][i];
        }
      }
      if (RV) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const yuv_u32x4 w = {packed[4 * s], packed[4 * s + 1], packed[4 * s + 2], packed[4 * s + 3]};
          reinterpret_cast<yuv_u32x4 *>(row)[s] = w;
        }
      }
    } else {
      float *img_dst = static_cast<float *>(a.dst) + (int64_t)img * a.rgb_stride;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float v[3][4];
        yuv_pixels4<SX, BIL, U8>(a, ly[r], cv[0][r], cv[1][r], g, v);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          float *o = img_dst + ((int64_t)k * H + y) * W + x0 + 4 * g;
          if (RV) {
            const yuv_f32x4 s = {v[k][0], v[k][1], v[k][2], v[k][3]};
            *reinterpret_cast<yuv_f32x4 *>(o) = s;
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (x0 + 4 * g + i < W) o[i] = v[k][i];
          }
        }
      }
    }
  }
}

// four columns of a row, x[channel][column] in 0 ... 255 -> p[(Y, Cb, Cr)][column] before quantisation and the four luma samples
__device__ __forceinline__ void yuv_ycc4(const YuvArgs &a, float maxv, const float (&x)[3][4], float (&p)[3][4], uint32_t *yq) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k][i] = __fadd_rn(yuv_dot(a.m + 3 * k, x[0][i], x[1][i], x[2][i]), a.off[k]);
    yq[i] = yuv_sample(p[0][i], maxv);
  }
}

// the chroma samples that columns 4 g ... 4 g + 3 of a row group give: the filter over the subsampled axes (the mean, or [1 2 1] / 4 along
// a co-sited axis), p[row][(Y, Cb, Cr)][column]; rows 0 and 1 are the group's own, row 2 (CY) the one above it; left[row] = (Cb, Cr) of
// column 4 g - 1 (read where CX)
template <int SX, int SY, bool CX, bool CY>
__device__ __forceinline__ void yuv_chroma4(float maxv, const float (&p)[1 + SY + CY][3][4], const float (&left)[1 + SY + CY][2], int g,
                                            uint32_t (&cq)[2][16 >> SX]) {
  constexpr int NR = 1 + SY + CY;
#pragma unroll
  for (int k = 1; k < 3; ++k) {
    if constexpr (SX) {
      constexpr float inv = 1.f / (float)((CX ? 4 : 2) * (SY ? (CY ? 4 : 2) : 1));
#pragma unroll
      for (int l = 0; l < 2; ++l) {
        float h[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          if (CX) h[r] = __fadd_rn(__fadd_rn(l ? p[r][k][1] : left[r][k - 1], p[r][k][2 * l + 1]), __fadd_rn(p[r][k][2 * l], p[r][k][2 * l]));
          else h[r] = __fadd_rn(p[r][k][2 * l], p[r][k][2 * l + 1]);
        }
        float s = h[0];
        if constexpr (SY) s = CY ? __fadd_rn(__fadd_rn(h[NR - 1], h[1]), __fadd_rn(h[0], h[0])) : __fadd_rn(h[0], h[1]);
        cq[k - 1][2 * g + l] = yuv_sample(__fmul_rn(s, inv), maxv);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) cq[k - 1][4 * g + i] = yuv_sample(p[0][k][i], maxv);
    }
  }
}

// (Cb, Cr) before quantisation of ONE pixel, from a scalar RGB load: the halo column of a co-sited horizontal axis.  The operations of
// the kernel's own columns in their order, so that a neighbouring thread's value of the same pixel is the same float.
template <bool U8>
__device__ __forceinline__ void yuv_cbcr1(const YuvArgs &a, int img, int y, int x, float (&c)[2]) {
  float v[3];
  if constexpr (U8) {
    const uint8_t *s = static_cast<const uint8_t *>(a.src) + (((int64_t)img * a.H + y) * a.W + x) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = (float)s[k];
  } else {
    const float *s = static_cast<const float *>(a.src) + (int64_t)img * a.rgb_stride + (int64_t)y * a.W + x;
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = __fmul_rn(fminf(fmaxf(s[(int64_t)k * a.H * a.W], 0.f), 1.f), 255.f);
  }
#pragma unroll
  for (int k = 1; k < 3; ++k) c[k - 1] = __fadd_rn(yuv_dot(a.m + 3 * k, v[0], v[1], v[2]), a.off[k]);
}

// CX / CY: the horizontal / vertical axis is subsampled AND co-sited ([1 2 1] / 4 instead of the mean of two).  CY adds a third row to
// what a thread reads, the one above its pair (NR rows: R own, which also give luma, then that one); CX one pixel left of its 16 per row.
template <int SX, int SY, typename T, bool YV, bool RV, bool U8, bool CX, bool CY>
__global__ __launch_bounds__(256) void rgb_to_yuv_kernel(const YuvArgs a) {
  static_assert((!CX || SX) && (!CY || SY), "only a subsampled axis has a siting");
  constexpr int R = 1 + SY, NR = R + CY, CW = 16 >> SX;
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= a.total) return;
  const int cg = item % a.gw, t = item / a.gw, rg = t % a.hr, img = t / a.hr;
  const int H = a.H, W = a.W, Hc = a.Hc, Wc = a.Wc;
  const int y0 = R * rg, x0 = 16 * cg, c0 = x0 >> SX;
  const bool second = SY && y0 + 1 < H;
  const int ys[3] = {y0, second ? y0 + 1 : y0, max(y0 - 1, 0)};  // an odd last row is its own partner; the row above clamps at row 0
  const float maxv = sizeof(T) == 1 ? 255.f : a.maxv;  // byte samples exist at depth 8 only: a constant clamp folds into one instruction

  uint32_t yq[NR][16], cq[2][CW];  // (yq of the row above is never stored: the compiler drops what computes it)
  float left[NR][2];
  if constexpr (CX) {
#pragma unroll
    for (int r = 0; r < NR; ++r) yuv_cbcr1<U8>(a, img, ys[r], max(x0 - 1, 0), left[r]);
  }
  if constexpr (U8) {
    uint32_t in[NR][12];  // the 48 interleaved bytes of each row
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const uint8_t *row = static_cast<const uint8_t *>(a.src) + ((int64_t)img * H + ys[r]) * W * 3;
      if (RV) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const yuv_u32x4 w = *reinterpret_cast<const yuv_u32x4 *>(row + (int64_t)x0 * 3 + 16 * s);
          in[r][4 * s] = w[0], in[r][4 * s + 1] = w[1], in[r][4 * s + 2] = w[2], in[r][4 * s + 3] = w[3];
        }
      } else {
#pragma unroll
        for (int d = 0; d < 12; ++d) {
          in[r][d] = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int b = 4 * d + e;  // byte of the 48: channel b % 3 of column x0 + b / 3
            in[r][d] |= (uint32_t)row[(int64_t)min(x0 + b / 3, W - 1) * 3 + b % 3] << (8 * e);
          }
        }
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float p[NR][3][4];  // row, (Y, Cb, Cr), column
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        float x[3][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const int b = 3 * (4 * g + i) + k;
            x[k][i] = (float)((in[r][b >> 2] >> (8 * (b & 3))) & 0xffu);
          }
        yuv_ycc4(a, maxv, x, p[r], yq[r] + 4 * g);
      }
      yuv_chroma4<SX, SY, CX, CY>(maxv, p, left, g, cq);
      if constexpr (CX) {
#pragma unroll
        for (int r = 0; r < NR; ++r) left[r][0] = p[r][1][3], left[r][1] = p[r][2][3];
      }
    }
  } else {
    const float *img_src = static_cast<const float *>(a.src) + (int64_t)img * a.rgb_stride;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float p[NR][3][4];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        float x[3][4];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float *s = img_src + ((int64_t)k * H + ys[r]) * W;
          yuv_f32x4 w;
          if (RV) {
            w = *reinterpret_cast<const yuv_f32x4 *>(s + x0 + 4 * g);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = s[min(x0 + 4 * g + i, W - 1)];
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) x[k][i] = __fmul_rn(fminf(fmaxf(w[i], 0.f), 1.f), 255.f);
        }
        yuv_ycc4(a, maxv, x, p[r], yq[r] + 4 * g);
      }
      yuv_chroma4<SX, SY, CX, CY>(maxv, p, left, g, cq);
      if constexpr (CX) {
#pragma unroll
        for (int r = 0; r < NR; ++r) left[r][0] = p[r][1][3], left[r][1] = p[r][2][3];
      }
    }
  }

  T *yp = reinterpret_cast<T *>(static_cast<uint8_t *>(a.dst) + (int64_t)img * a.yuv_stride);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r == 1 && !second) break;
    yuv_store<T, 16, YV>(yp + (int64_t)(y0 + r) * W, x0, W, yq[r]);
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) yuv_store<T, CW, YV>(yp + (int64_t)H * W + (int64_t)k * Hc * Wc + (int64_t)rg * Wc, c0, Wc, cq[k]);
}

static inline bool yuv_aligned(const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// validates, fills the geometry and the two access-width flags; coef: 12 host floats, the matrix row-major, then the offsets.
// Byte RGB (8-bit 4:2:0 only) is dense: it has no image stride to validate.
static int yuv_fill(YuvArgs &a, const char *what, const void *yuv, const void *rgb, bool rgb_u8, int n, int H, int W, int sub_x, int sub_y,
                    int depth, int64_t yuv_stride, int64_t rgb_stride, const float *coef, int siting_x, int siting_y, bool &yv, bool &rv) {
  EDVR_REQUIRE(yuv && rgb && coef && n > 0 && H > 0 && W > 0, "%s: bad arguments", what);
  EDVR_REQUIRE((siting_x == 0 || siting_x == 1) && (siting_y == 0 || siting_y == 1),
               "%s: a siting is 0 (centre) or 1 (co-sited) per axis, got (%d, %d)", what, siting_x, siting_y);
  EDVR_REQUIRE(siting_y <= siting_x, "%s: co-sited rows go with co-sited columns ('topleft'); (0, 1) is no siting in use", what);
  EDVR_REQUIRE(depth >= 8 && depth <= 16, "%s: a depth of %d bits is outside 8 ... 16", what, depth);
  EDVR_REQUIRE((sub_x == 1 && sub_y == 1) || (sub_x == 1 && sub_y == 0) || (sub_x == 0 && sub_y == 0),
               "%s: chroma subsampling (%d, %d) is none of 4:2:0 (1, 1), 4:2:2 (1, 0), 4:4:4 (0, 0)", what, sub_x, sub_y);
  EDVR_REQUIRE(!rgb_u8 || (sub_x == 1 && sub_y == 1 && depth == 8), "%s: uint8 RGB goes with 8-bit 4:2:0 only", what);
  EDVR_REQUIRE((int64_t)H * W <= INT32_MAX / 4, "%s: a %d x %d frame is too large", what, H, W);
  const int bps = depth > 8 ? 2 : 1;
  a.H = H, a.W = W, a.Hc = (H + sub_y) >> sub_y, a.Wc = (W + sub_x) >> sub_x;
  const int64_t framesize = ((int64_t)H * W + 2 * (int64_t)a.Hc * a.Wc) * bps;
  EDVR_REQUIRE(n == 1 || yuv_stride >= framesize, "%s: frames %lld bytes apart do not hold the %lld bytes of a %d x %d frame", what,
               (long long)yuv_stride, (long long)framesize, H, W);
  EDVR_REQUIRE(bps == 1 || (yuv_aligned(yuv, 2) && (n == 1 || yuv_stride % 2 == 0)),
               "%s: 16-bit samples need an even base address and an even frame stride (%lld)", what, (long long)yuv_stride);
  EDVR_REQUIRE(rgb_u8 || n == 1 || rgb_stride >= 3 * (int64_t)H * W, "%s: images %lld floats apart overlap", what, (long long)rgb_stride);
  a.gw = cdiv(W, 16), a.hr = sub_y ? a.Hc : H;
  const int64_t total = (int64_t)n * a.hr * a.gw;
  EDVR_REQUIRE(total <= INT32_MAX - 256, "%s: %d frames of %d x %d are too many for one launch", what, n, H, W);
  a.total = (int)total;
  a.yuv_stride = yuv_stride, a.rgb_stride = rgb_stride;
  for (int i = 0; i < 9; ++i) a.m[i] = coef[i];
  for (int i = 0; i < 3; ++i) a.off[i] = coef[9 + i];
  a.maxv = (float)((1 << depth) - 1);
  // the decode's weights: centre (1/4, 3/4 | 3/4, 1/4), co-sited (0, 1 | 1/2, 1/2); an axis that is not subsampled never reads its four
  static const float centre[4] = {0.25f, 0.75f, 0.75f, 0.25f}, cosited[4] = {0.f, 1.f, 0.5f, 0.5f};
  for (int i = 0; i < 4; ++i) a.wv[i] = (siting_y ? cosited : centre)[i], a.wh[i] = (siting_x ? cosited : centre)[i];
  // W % 16 == 0: H W and Hc Wc samples are multiples of 16 and 8, so every plane row starts as aligned as its accesses are wide
  const bool whole = W % 16 == 0;
  yv = whole && yuv_aligned(yuv, 16) && (n == 1 || yuv_stride % 16 == 0);
  rv = whole && yuv_aligned(rgb, 16) && (rgb_u8 || n == 1 || rgb_stride % 4 == 0);
  return EDVR_OK;
}

template <int SX, int SY, typename T, bool BIL, bool U8>
static void yuv_decode_launch(bool yv, bool rv, const YuvArgs &a, hipStream_t stream) {
  const dim3 grid(cdiv(a.total, 256)), block(256);
  if (yv && rv) hipLaunchKernelGGL((yuv_to_rgb_kernel<SX, SY, T, true, true, BIL, U8>), grid, block, 0, stream, a);
  else if (yv) hipLaunchKernelGGL((yuv_to_rgb_kernel<SX, SY, T, true, false, BIL, U8>), grid, block, 0, stream, a);
  else if (rv) hipLaunchKernelGGL((yuv_to_rgb_kernel<SX, SY, T, false, true, BIL, U8>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((yuv_to_rgb_kernel<SX, SY, T, false, false, BIL, U8>), grid, block, 0, stream, a);
}

template <int SX, int SY, typename T, bool U8, bool CX, bool CY>
static void yuv_encode_launch(bool yv, bool rv, const YuvArgs &a, hipStream_t stream) {
  const dim3 grid(cdiv(a.total, 256)), block(256);
  if (yv && rv) hipLaunchKernelGGL((rgb_to_yuv_kernel<SX, SY, T, true, true, U8, CX, CY>), grid, block, 0, stream, a);
  else if (yv) hipLaunchKernelGGL((rgb_to_yuv_kernel<SX, SY, T, true, false, U8, CX, CY>), grid, block, 0, stream, a);
  else if (rv) hipLaunchKernelGGL((rgb_to_yuv_kernel<SX, SY, T, false, true, U8, CX, CY>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((rgb_to_yuv_kernel<SX, SY, T, false, false, U8, CX, CY>), grid, block, 0, stream, a);
}

// the siting -> the instance: (centre, centre), 'left' (co-sited columns), 'topleft' (both) where the axis is subsampled; co-sited rows
// under centred columns is a siting nobody uses and has no instance (the callers refuse it)
template <int SX, int SY, typename T, bool U8>
static void yuv_encode_siting(bool cx, bool cy, bool yv, bool rv, const YuvArgs &a, hipStream_t stream) {
  if constexpr (SX) {
    if (cx && SY && cy) return yuv_encode_launch<SX, SY, T, U8, true, SY != 0>(yv, rv, a, stream);
    if (cx) return yuv_encode_launch<SX, SY, T, U8, true, false>(yv, rv, a, stream);
  }
  yuv_encode_launch<SX, SY, T, U8, false, false>(yv, rv, a, stream);
}

// (4:4:4 has nothing to filter: its one decode instance per sample type serves both values of `bilinear`)
template <int SX, int SY, typename T, bool U8>
static void yuv_decode_filter(bool bil, bool yv, bool rv, const YuvArgs &a, hipStream_t stream) {
  if (SX && bil) yuv_decode_launch<SX, SY, T, SX != 0, U8>(yv, rv, a, stream);
  else yuv_decode_launch<SX, SY, T, false, U8>(yv, rv, a, stream);
}

// the format -> the instance.  Byte RGB is instantiated for 8-bit 4:2:0 alone, which yuv_fill has made sure of.
template <bool U8>
static int yuv_decode(const char *what, const uint8_t *yuv, void *rgb, int n, int H, int W, int sub_x, int sub_y, int depth, int64_t yuv_stride,
                      int64_t rgb_stride, const float *coef, int bilinear, int siting_x, int siting_y, edvr_stream_t stream) {
  YuvArgs a;
  bool yv, rv;
  const int rc = yuv_fill(a, what, yuv, rgb, U8, n, H, W, sub_x, sub_y, depth, yuv_stride, rgb_stride, coef, siting_x, siting_y, yv, rv);
  if (rc != EDVR_OK) return rc;
  a.src = yuv, a.dst = rgb;
  const bool wide = depth > 8, bil = bilinear != 0;
  hipStream_t s = as_stream(stream);
  if constexpr (U8) {
    yuv_decode_filter<1, 1, uint8_t, true>(bil, yv, rv, a, s);
  } else if (sub_y) {
    wide ? yuv_decode_filter<1, 1, uint16_t, false>(bil, yv, rv, a, s) : yuv_decode_filter<1, 1, uint8_t, false>(bil, yv, rv, a, s);
  } else if (sub_x) {
    wide ? yuv_decode_filter<1, 0, uint16_t, false>(bil, yv, rv, a, s) : yuv_decode_filter<1, 0, uint8_t, false>(bil, yv, rv, a, s);
  } else {
    wide ? yuv_decode_filter<0, 0, uint16_t, false>(bil, yv, rv, a, s) : yuv_decode_filter<0, 0, uint8_t, false>(bil, yv, rv, a, s);
  }
  return check_launch("yuv_to_rgb_kernel");
}

template <bool U8>
static int yuv_encode(const char *what, const void *rgb, uint8_t *yuv, int n, int H, int W, int sub_x, int sub_y, int depth, int64_t rgb_stride,
                      int64_t yuv_stride, const float *coef, int siting_x, int siting_y, edvr_stream_t stream) {
  YuvArgs a;
  bool yv, rv;
  const int rc = yuv_fill(a, what, yuv, rgb, U8, n, H, W, sub_x, sub_y, depth, yuv_stride, rgb_stride, coef, siting_x, siting_y, yv, rv);
  if (rc != EDVR_OK) return rc;
  a.src = rgb, a.dst = yuv;
  const bool wide = depth > 8, cx = siting_x != 0, cy = siting_y != 0;
  hipStream_t s = as_stream(stream);
  if constexpr (U8) {
    yuv_encode_siting<1, 1, uint8_t, true>(cx, cy, yv, rv, a, s);
  } else if (sub_y) {
    wide ? yuv_encode_siting<1, 1, uint16_t, false>(cx, cy, yv, rv, a, s) : yuv_encode_siting<1, 1, uint8_t, false>(cx, cy, yv, rv, a, s);
  } else if (sub_x) {
    wide ? yuv_encode_siting<1, 0, uint16_t, false>(cx, cy, yv, rv, a, s) : yuv_encode_siting<1, 0, uint8_t, false>(cx, cy, yv, rv, a, s);
  } else {
    wide ? yuv_encode_siting<0, 0, uint16_t, false>(cx, cy, yv, rv, a, s) : yuv_encode_siting<0, 0, uint8_t, false>(cx, cy, yv, rv, a, s);
  }
  return check_launch("rgb_to_yuv_kernel");
}

}  // namespace edvr

extern "C" int edvr_yuv_to_rgb_f32(const uint8_t *yuv, float *rgb, int n, int H, int W, int sub_x, int sub_y, int depth, int64_t yuv_stride,
                                   int64_t rgb_img_stride, const float *coef, int bilinear, edvr_stream_t stream) {
  return edvr::yuv_decode<false>("yuv_to_rgb", yuv, rgb, n, H, W, sub_x, sub_y, depth, yuv_stride, rgb_img_stride, coef, bilinear, 0, 0, stream);
}

extern "C" int edvr_rgb_to_yuv_f32(const float *rgb, uint8_t *yuv, int n, int H, int W, int sub_x, int sub_y, int depth, int64_t rgb_img_stride,
                                   int64_t yuv_stride, const float *coef, edvr_stream_t stream) {
  return edvr::yuv_encode<false>("rgb_to_yuv", rgb, yuv, n, H, W, sub_x, sub_y, depth, rgb_img_stride, yuv_stride, coef, 0, 0, stream);
}

extern "C" int edvr_yuv420_to_rgb_f32(const uint8_t *yuv, float *rgb, int n, int H, int W, int64_t yuv_stride, int64_t rgb_img_stride,
                                      const float *coef, int bilinear, edvr_stream_t stream) {
  return edvr::yuv_decode<false>("yuv420_to_rgb", yuv, rgb, n, H, W, 1, 1, 8, yuv_stride, rgb_img_stride, coef, bilinear, 0, 0, stream);
}

extern "C" int edvr_yuv420_to_rgb_u8(const uint8_t *yuv, uint8_t *rgb, int n, int H, int W, int64_t yuv_stride, const float *coef, int bilinear,
                                     edvr_stream_t stream) {
  return edvr::yuv_decode<true>("yuv420_to_rgb", yuv, rgb, n, H, W, 1, 1, 8, yuv_stride, 0, coef, bilinear, 0, 0, stream);
}

extern "C" int edvr_rgb_to_yuv420_f32(const float *rgb, uint8_t *yuv, int n, int H, int W, int64_t rgb_img_stride, int64_t yuv_stride,
                                      const float *coef, edvr_stream_t stream) {
  return edvr::yuv_encode<false>("rgb_to_yuv420", rgb, yuv, n, H, W, 1, 1, 8, rgb_img_stride, yuv_stride, coef, 0, 0, stream);
}

extern "C" int edvr_rgb_to_yuv420_u8(const uint8_t *rgb, uint8_t *yuv, int n, int H, int W, int64_t yuv_stride, const float *coef,
                                     edvr_stream_t stream) {
  return edvr::yuv_encode<true>("rgb_to_yuv420", rgb, yuv, n, H, W, 1, 1, 8, 0, yuv_stride, coef, 0, 0, stream);
}

// the same with a chroma siting per axis (0 centre, 1 co-sited): each function above is its sited form at (0, 0)
extern "C" int edvr_yuv_to_rgb_sited_f32(const uint8_t *yuv, float *rgb, int n, int H, int W, int sub_x, int sub_y, int depth, int64_t yuv_stride,
                                         int64_t rgb_img_stride, const float *coef, int bilinear, int siting_x, int siting_y,
                                         edvr_stream_t stream) {
  return edvr::yuv_decode<false>("yuv_to_rgb", yuv, rgb, n, H, W, sub_x, sub_y, depth, yuv_stride, rgb_img_stride, coef, bilinear, siting_x,
                                 siting_y, stream);
}

extern "C" int edvr_rgb_to_yuv_sited_f32(const float *rgb, uint8_t *yuv, int n, int H, int W, int sub_x, int sub_y, int depth,
                                         int64_t rgb_img_stride, int64_t yuv_stride, const float *coef, int siting_x, int siting_y,
                                         edvr_stream_t stream) {
  return edvr::yuv_encode<false>("rgb_to_yuv", rgb, yuv, n, H, W, sub_x, sub_y, depth, rgb_img_stride, yuv_stride, coef, siting_x, siting_y,
                                 stream);
}

extern "C" int edvr_yuv420_to_rgb_sited_u8(const uint8_t *yuv, uint8_t *rgb, int n, int H, int W, int64_t yuv_stride, const float *coef,
                                           int bilinear, int siting_x, int siting_y, edvr_stream_t stream) {
  return edvr::yuv_decode<true>("yuv420_to_rgb", yuv, rgb, n, H, W, 1, 1, 8, yuv_stride, 0, coef, bilinear, siting_x, siting_y, stream);
}

extern "C" int edvr_rgb_to_yuv420_sited_u8(const uint8_t *rgb, uint8_t *yuv, int n, int H, int W, int64_t yuv_stride, const float *coef,
                                           int siting_x, int siting_y, edvr_stream_t stream) {
  return edvr::yuv_encode<true>("rgb_to_yuv420", rgb, yuv, n, H, W, 1, 1, 8, 0, yuv_stride, coef, siting_x, siting_y, stream);
}
