// yuv.hip - 8-bit Y'CbCr 4:2:0 (I420: the payload of a YUV4MPEG2 frame) <-> RGB on the device, both directions, so that decoded video
// reaches VideoRestorer without passing through RGB bytes on the host and the network's float32 result is quantised ONCE, to YUV bytes.
//
// Frame of (H, W): H W luma bytes, then Hc Wc bytes of Cb, then of Cr, Hc = ceil(H / 2), Wc = ceil(W / 2), each plane dense.  A batch is n
// such frames `yuv_stride` bytes apart at any base address (a Y4M read buffer: stride framesize + 6, base 6 past its start).
//
// Definition.  M (3 x 3, RGB in 0 ... 255 -> Y, Cb, Cr without offsets), its inverse Mi and the offsets (yoff, 128, 128)
// are computed by the caller in float64, rounded to float32 and arrive as kernel arguments - no tables.  Every product and every sum
// below is one float32 operation, rounded on its own, in the order written (yuv_mul keeps the products out of fused multiply-adds):
//   decode  C = chroma plane upsampled: 'nearest' plane[i >> 1][j >> 1]; 'bilinear' (centre-sited) per axis, indices clamped to the plane,
//             even 2k: 0.25 c[k - 1] + 0.75 c[k], odd 2k + 1: 0.75 c[k] + 0.25 c[k + 1], vertical then horizontal (exact in float32);
//           d = (Y - yoff, Cb - 128, Cr - 128);  v_k = (Mi[k][0] d0 + Mi[k][1] d1) + Mi[k][2] d2
//           float32 (n, 3, H, W): clamp(v_k, 0, 255) / 255.0f      uint8 (n, H, W, 3): rint(clamp(v_k, 0, 255))
//   encode  x = clamp(f, 0, 1) * 255.0f (float32 (n, 3, H, W), NaN -> 0 as to_u8 of pixel.h) or the byte (uint8 (n, H, W, 3));
//           p_k = ((M[k][0] r + M[k][1] g) + M[k][2] b) + off_k;  Y = rint(clamp(p_0, 0, 255));
//           chroma (k, l) = rint(clamp(((p[2k][2l] + p[2k][2l + 1]) + (p[2k + 1][2l] + p[2k + 1][2l + 1])) * 0.25f, 0, 255)), row and
//           column indices clamped to the frame (an odd edge replicates).
//
// Kernel shape: both kernels move bytes and nothing else.  One thread owns 2 rows x 16 columns = one chroma row of 8 samples per plane,
// so every luma byte, chroma byte and RGB sample is loaded by exactly one thread (the bilinear decode re-reads the two neighbouring chroma
// rows and one sample left and right of its 8 through the cache: 1/4 of a byte per pixel and plane).  Two template flags pick the access
// width per side, both need W % 16 == 0 (every thread's 16 columns are whole): YV - 16-byte luma and 8-byte chroma accesses, where the
// batch base and stride are 16-byte aligned; RV - 16-byte float / packed RGB byte accesses, where the RGB tensor is.  The scalar forms
// clamp every load index into the frame and guard every store, and cover odd sizes, W % 16 != 0 and the 6-byte offset of a Y4M buffer.
// Consecutive threads own consecutive 16-column groups of one row pair.  No LDS, 0 bytes of scratch.
#include <cstdint>

#include "common.h"
#include "pixel.h"

namespace edvr {

typedef float yuv_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t yuv_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t yuv_u32x2 __attribute__((ext_vector_type(2)));

struct YuvArgs {
  const void *src;
  void *dst;
  int64_t yuv_stride;  // bytes between the frames of the I420 batch
  int64_t rgb_stride;  // float RGB: floats between images; byte RGB: dense
  int H, W, Hc, Wc;
  int gw, hp, total;  // 16-column groups per row, row pairs per frame, threads with work
  float m[9];         // decode: Mi, encode: M (row-major)
  float off[3];       // (yoff, 128, 128)
};

// (exact in float32 for bytes and weights 1/4, 3/4: fused or not, the same value)
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
__device__ __forceinline__ float yuv_byte(float v) { return rintf(fminf(fmaxf(v, 0.f), 255.f)); }

// 16 bytes of a plane row from column x0 as four little-endian dwords; the scalar form clamps the column to the row
template <bool VEC>
__device__ __forceinline__ void yuv_load16(const uint8_t *__restrict__ row, int x0, int w, uint32_t (&q)[4]) {
  if (VEC) {
    const yuv_u32x4 v = *reinterpret_cast<const yuv_u32x4 *>(row + x0);
    q[0] = v[0], q[1] = v[1], q[2] = v[2], q[3] = v[3];
  } else {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      q[d] = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) q[d] |= (uint32_t)row[min(x0 + 4 * d + e, w - 1)] << (8 * e);
    }
  }
}

// chroma samples c0 - 1 ... c0 + 8 of a plane row as floats, v[j] = column clamp(c0 - 1 + j); the two outer ones only when WIDE
template <bool VEC, bool WIDE>
__device__ __forceinline__ void yuv_load_chroma(const uint8_t *__restrict__ row, int c0, int wc, float (&v)[10]) {
  if (VEC) {
    const yuv_u32x2 q = *reinterpret_cast<const yuv_u32x2 *>(row + c0);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[1 + j] = (float)((q[j >> 2] >> (8 * (j & 3))) & 0xffu);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[1 + j] = (float)row[min(c0 + j, wc - 1)];
  }
  v[0] = WIDE ? (float)row[max(c0 - 1, 0)] : 0.f;
  v[9] = WIDE ? (float)row[min(c0 + 8, wc - 1)] : 0.f;
}

template <bool YV, bool RV, bool BIL, bool U8>
__global__ __launch_bounds__(256) void yuv420_to_rgb_kernel(const YuvArgs a) {
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= a.total) return;
  const int cg = item % a.gw, t = item / a.gw, rp = t % a.hp, img = t / a.hp;
  const int H = a.H, W = a.W, Hc = a.Hc, Wc = a.Wc;
  const uint8_t *yp = static_cast<const uint8_t *>(a.src) + (int64_t)img * a.yuv_stride;
  const int y0 = 2 * rp, x0 = 16 * cg, c0 = 8 * cg;
  const bool second = y0 + 1 < H;

  uint32_t q[2][4];
  yuv_load16<YV>(yp + (int64_t)y0 * W, x0, W, q[0]);
  yuv_load16<YV>(yp + (int64_t)(second ? y0 + 1 : y0) * W, x0, W, q[1]);

  // chroma after the vertical pass: cv[plane][row of the pair][column c0 - 1 + j]
  float cv[2][2][10];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const uint8_t *plane = yp + (int64_t)H * W + (int64_t)p * Hc * Wc;
    float mid[10];
    yuv_load_chroma<YV, BIL>(plane + (int64_t)rp * Wc, c0, Wc, mid);
    if (BIL) {
      float up[10], dn[10];
      yuv_load_chroma<YV, true>(plane + (int64_t)max(rp - 1, 0) * Wc, c0, Wc, up);
      yuv_load_chroma<YV, true>(plane + (int64_t)min(rp + 1, Hc - 1) * Wc, c0, Wc, dn);
#pragma unroll
      for (int j = 0; j < 10; ++j) {
        cv[p][0][j] = yuv_mix(0.25f, up[j], 0.75f, mid[j]);
        cv[p][1][j] = yuv_mix(0.75f, mid[j], 0.25f, dn[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 10; ++j) cv[p][0][j] = cv[p][1][j] = mid[j];
    }
  }

#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (r == 1 && !second) break;
    const int y = y0 + r;
    uint32_t packed[12];  // U8: the 48 interleaved bytes of this row
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float v[3][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int px = 4 * g + i, l = px >> 1;
        float c[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const float *s = cv[p][r];
          c[p] = !BIL ? s[l + 1] : ((px & 1) ? yuv_mix(0.75f, s[l + 1], 0.25f, s[l + 2]) : yuv_mix(0.25f, s[l], 0.75f, s[l + 1]));
        }
        const float d0 = __fsub_rn((float)((q[r][g] >> (8 * i)) & 0xffu), a.off[0]);
        const float d1 = __fsub_rn(c[0], a.off[1]), d2 = __fsub_rn(c[1], a.off[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float w = fminf(fmaxf(yuv_dot(a.m + 3 * k, d0, d1, d2), 0.f), 255.f);
          v[k][i] = U8 ? rintf(w) : __fdiv_rn(w, 255.f);
        }
      }
      if (U8) {
        uint8_t *row = static_cast<uint8_t *>(a.dst) + ((int64_t)img * H + y) * W * 3;
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
              for (int k = 0; k < 3; ++k) row[(int64_t)(x0 + 4 * g + i) * 3 + k] = (uint8_t)(unsigned)v[k][i];
        }
      } else {
        float *img_dst = static_cast<float *>(a.dst) + (int64_t)img * a.rgb_stride;
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
    if (U8 && RV) {
      yuv_u32x4 *o = reinterpret_cast<yuv_u32x4 *>(static_cast<uint8_t *>(a.dst) + (((int64_t)img * H + y) * W + x0) * 3);
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const yuv_u32x4 w = {packed[4 * s], packed[4 * s + 1], packed[4 * s + 2], packed[4 * s + 3]};
        o[s] = w;
      }
    }
  }
}

template <bool YV, bool RV, bool U8>
__global__ __launch_bounds__(256) void rgb_to_yuv420_kernel(const YuvArgs a) {
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= a.total) return;
  const int cg = item % a.gw, t = item / a.gw, rp = t % a.hp, img = t / a.hp;
  const int H = a.H, W = a.W, Hc = a.Hc, Wc = a.Wc;
  const int y0 = 2 * rp, x0 = 16 * cg, c0 = 8 * cg;
  const bool second = y0 + 1 < H;
  const int ys[2] = {y0, second ? y0 + 1 : y0};  // an odd last row is its own partner

  uint32_t in[2][12];  // U8: the 48 interleaved bytes of each row
  if (U8) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
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
  }

  uint32_t yq[2][4], cq[2][2];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float p[2][3][4];  // row, (Y, Cb, Cr), column
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      float x[3][4];
      if (U8) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const int b = 3 * (4 * g + i) + k;
            x[k][i] = (float)((in[r][b >> 2] >> (8 * (b & 3))) & 0xffu);
          }
      } else {
        const float *img_src = static_cast<const float *>(a.src) + (int64_t)img * a.rgb_stride;
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
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) p[r][k][i] = __fadd_rn(yuv_dot(a.m + 3 * k, x[0][i], x[1][i], x[2][i]), a.off[k]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t byte = (uint32_t)yuv_byte(p[r][0][i]);
        yq[r][g] = i == 0 ? byte : (yq[r][g] | (byte << (8 * i)));
      }
    }
#pragma unroll
    for (int k = 1; k < 3; ++k)
#pragma unroll
      for (int l = 0; l < 2; ++l) {
        const float s = __fmul_rn(__fadd_rn(__fadd_rn(p[0][k][2 * l], p[0][k][2 * l + 1]), __fadd_rn(p[1][k][2 * l], p[1][k][2 * l + 1])), 0.25f);
        const uint32_t byte = (uint32_t)yuv_byte(s);
        const int j = 2 * g + l;  // chroma sample c0 + j
        cq[k - 1][j >> 2] = (j & 3) == 0 ? byte : (cq[k - 1][j >> 2] | (byte << (8 * (j & 3))));
      }
  }

  uint8_t *yp = static_cast<uint8_t *>(a.dst) + (int64_t)img * a.yuv_stride;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (r == 1 && !second) break;
    uint8_t *row = yp + (int64_t)(y0 + r) * W + x0;
    if (YV) {
      const yuv_u32x4 w = {yq[r][0], yq[r][1], yq[r][2], yq[r][3]};
      *reinterpret_cast<yuv_u32x4 *>(row) = w;
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (x0 + i < W) row[i] = (uint8_t)(yq[r][i >> 2] >> (8 * (i & 3)));
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    uint8_t *row = yp + (int64_t)H * W + (int64_t)k * Hc * Wc + (int64_t)rp * Wc + c0;
    if (YV) {
      const yuv_u32x2 w = {cq[k][0], cq[k][1]};
      *reinterpret_cast<yuv_u32x2 *>(row) = w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (c0 + j < Wc) row[j] = (uint8_t)(cq[k][j >> 2] >> (8 * (j & 3)));
    }
  }
}

static inline bool yuv_aligned(const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// fills the geometry and the two access-width flags; the coefficients are 12 host floats: the matrix row-major, then the offsets
static int yuv_fill(YuvArgs &a, const char *what, const void *yuv, const void *rgb, bool rgb_u8, int n, int H, int W, int64_t yuv_stride,
                    int64_t rgb_stride, const float *coef, bool &yv, bool &rv) {
  EDVR_REQUIRE(yuv && rgb && coef && n > 0 && H > 0 && W > 0, "%s: bad arguments", what);
  EDVR_REQUIRE((int64_t)H * W <= INT32_MAX / 4, "%s: a %d x %d frame is too large", what, H, W);
  a.H = H, a.W = W, a.Hc = (H + 1) / 2, a.Wc = (W + 1) / 2;
  const int64_t framesize = (int64_t)H * W + 2 * (int64_t)a.Hc * a.Wc;
  EDVR_REQUIRE(n == 1 || yuv_stride >= framesize, "%s: frames %lld bytes apart do not hold the %lld bytes of a %d x %d I420 frame", what,
               (long long)yuv_stride, (long long)framesize, H, W);
  EDVR_REQUIRE(rgb_u8 || n == 1 || rgb_stride >= 3 * (int64_t)H * W, "%s: images %lld floats apart overlap", what, (long long)rgb_stride);
  a.gw = cdiv(W, 16), a.hp = a.Hc;
  const int64_t total = (int64_t)n * a.hp * a.gw;
  EDVR_REQUIRE(total <= INT32_MAX - 256, "%s: %d frames of %d x %d are too many for one launch", what, n, H, W);
  a.total = (int)total;
  a.yuv_stride = yuv_stride, a.rgb_stride = rgb_stride;
  for (int i = 0; i < 9; ++i) a.m[i] = coef[i];
  for (int i = 0; i < 3; ++i) a.off[i] = coef[9 + i];
  const bool whole = W % 16 == 0;  // then H W and Hc Wc are multiples of 16 and 8: every plane row starts as aligned as the frame
  yv = whole && yuv_aligned(yuv, 16) && (n == 1 || yuv_stride % 16 == 0);
  rv = whole && yuv_aligned(rgb, 16) && (rgb_u8 || n == 1 || rgb_stride % 4 == 0);
  return EDVR_OK;
}

template <bool BIL, bool U8>
static void yuv_decode_dispatch(bool yv, bool rv, const YuvArgs &a, hipStream_t stream) {
  const dim3 grid(cdiv(a.total, 256)), block(256);
  if (yv && rv) hipLaunchKernelGGL((yuv420_to_rgb_kernel<true, true, BIL, U8>), grid, block, 0, stream, a);
  else if (yv) hipLaunchKernelGGL((yuv420_to_rgb_kernel<true, false, BIL, U8>), grid, block, 0, stream, a);
  else if (rv) hipLaunchKernelGGL((yuv420_to_rgb_kernel<false, true, BIL, U8>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((yuv420_to_rgb_kernel<false, false, BIL, U8>), grid, block, 0, stream, a);
}

template <bool U8>
static int yuv_decode(const uint8_t *yuv, void *rgb, int n, int H, int W, int64_t yuv_stride, int64_t rgb_stride, const float *coef, int bilinear,
                      edvr_stream_t stream) {
  YuvArgs a;
  bool yv, rv;
  const int rc = yuv_fill(a, "yuv420_to_rgb", yuv, rgb, U8, n, H, W, yuv_stride, rgb_stride, coef, yv, rv);
  if (rc != EDVR_OK) return rc;
  a.src = yuv, a.dst = rgb;
  if (bilinear) yuv_decode_dispatch<true, U8>(yv, rv, a, as_stream(stream));
  else yuv_decode_dispatch<false, U8>(yv, rv, a, as_stream(stream));
  return check_launch("yuv420_to_rgb_kernel");
}

template <bool U8>
static int yuv_encode(const void *rgb, uint8_t *yuv, int n, int H, int W, int64_t rgb_stride, int64_t yuv_stride, const float *coef,
                      edvr_stream_t stream) {
  YuvArgs a;
  bool yv, rv;
  const int rc = yuv_fill(a, "rgb_to_yuv420", yuv, rgb, U8, n, H, W, yuv_stride, rgb_stride, coef, yv, rv);
  if (rc != EDVR_OK) return rc;
  a.src = rgb, a.dst = yuv;
  const dim3 grid(cdiv(a.total, 256)), block(256);
  hipStream_t s = as_stream(stream);
  if (yv && rv) hipLaunchKernelGGL((rgb_to_yuv420_kernel<true, true, U8>), grid, block, 0, s, a);
  else if (yv) hipLaunchKernelGGL((rgb_to_yuv420_kernel<true, false, U8>), grid, block, 0, s, a);
  else if (rv) hipLaunchKernelGGL((rgb_to_yuv420_kernel<false, true, U8>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((rgb_to_yuv420_kernel<false, false, U8>), grid, block, 0, s, a);
  return check_launch("rgb_to_yuv420_kernel");
}

}  // namespace edvr

extern "C" int edvr_yuv420_to_rgb_f32(const uint8_t *yuv, float *rgb, int n, int H, int W, int64_t yuv_stride, int64_t rgb_img_stride,
                                      const float *coef, int bilinear, edvr_stream_t stream) {
  return edvr::yuv_decode<false>(yuv, rgb, n, H, W, yuv_stride, rgb_img_stride, coef, bilinear, stream);
}

extern "C" int edvr_yuv420_to_rgb_u8(const uint8_t *yuv, uint8_t *rgb, int n, int H, int W, int64_t yuv_stride, const float *coef, int bilinear,
                                     edvr_stream_t stream) {
  return edvr::yuv_decode<true>(yuv, rgb, n, H, W, yuv_stride, 0, coef, bilinear, stream);
}

extern "C" int edvr_rgb_to_yuv420_f32(const float *rgb, uint8_t *yuv, int n, int H, int W, int64_t rgb_img_stride, int64_t yuv_stride,
                                      const float *coef, edvr_stream_t stream) {
  return edvr::yuv_encode<false>(rgb, yuv, n, H, W, rgb_img_stride, yuv_stride, coef, stream);
}

extern "C" int edvr_rgb_to_yuv420_u8(const uint8_t *rgb, uint8_t *yuv, int n, int H, int W, int64_t yuv_stride, const float *coef,
                                     edvr_stream_t stream) {
  return edvr::yuv_encode<true>(rgb, yuv, n, H, W, 0, yuv_stride, coef, stream);
}
