// degrade.hip - blur and noise on the device: what an 8-bit RGB frame looks like behind soft optics and a noisy sensor, the two steps of
// the first-order degradation model that come before compression (jpeg.hip).  Definition: DESIGN 4.17.  The blur is a per-image ksize x
// ksize kernel of Q20 integer weights that sum to 2^20, over the frame extended by the reflection that does not repeat the edge sample:
// exact 32-bit integer arithmetic, so the order of the sum is free.  The noise is Gaussian, s = sqrt(shot v + read^2) per sample, from
// ONE Philox4x32-10 call per pixel (counter (x, y, ctr_t, 0), the image's 64-bit key) and two Box-Muller draws, in float32.
//
// ONE launch, grid (tiles, n), no workspace.  A workgroup of 256 lanes owns a 64 x 64 pixel tile of one image:
//   0. the image's weights in LDS, rows 24 words apart and zero beyond ksize (ksize 0 is the 1 x 1 kernel {2^20});
//   1. fill: the tile and its ring as BYTES in LDS, three planes of 84 rows of 96 columns (tile column 0 is column 12: pixel quads stay
//      dword aligned).  A lane reads 4 pixels of a row - three dwords where rows are 4-byte aligned and the quad lies inside the frame,
//      reflected pixel by pixel otherwise - and writes one dword per plane.  Only the rows and quads that the image's ksize reaches;
//   2. taps: a lane computes 4 adjacent pixels x 3 channels (12 accumulators) of a row, 4 rows per lane.  Per kernel row it walks the
//      plane row dword by dword: v_alignbyte_b32 by the image's (12 - r) & 3 turns two dwords into the 4 bytes under taps 4 j .. 4 j + 3 of
//      pixel 0, the next such word holds the 3 bytes the other pixels need besides: 7 byte extracts and 16 v_mad_u32_u24 per plane and
//      LDS dword, with 4 weights from one broadcast 16-byte read.  The loops run ksize and ceil(ksize / 4) times: a 7 x 7 image costs 7 x 8
//      taps, not 21 x 21.  The 32 lanes of an LDS lane group cover 16 dwords each of rows y and y + 2: 48 words apart, no shared bank;
//   3. round (no noise) or add the noise, clamp, and store 12 bytes per lane.
#include <algorithm>

#include "common.h"

namespace edvr {

struct DegradeArgs {
  const uint8_t *src;
  uint8_t *dst;
  const int32_t *table;    // n records of EDVR_DEGRADE_RECORD_INTS
  const int32_t *weights;  // Q20 kernels, or null where no record blurs
  int H, W;
  int64_t src_stride, dst_stride;  // bytes between images
  int src_vec, dst_vec;            // every pixel quad of a row starts on a 4-byte boundary
};

enum { DGR_KSIZE = 0, DGR_WEIGHTS = 1, DGR_READ = 2, DGR_SHOT = 3, DGR_FLAGS = 4, DGR_KEY_LO = 5, DGR_KEY_HI = 6, DGR_CTR_T = 7 };

constexpr int DT = EDVR_DEGRADE_TILE;      // tile side, pixels
constexpr int DK = EDVR_DEGRADE_MAX_KSIZE; // 21
constexpr int DR = DK / 2;                 // ring, pixels
constexpr int DL = 12;                     // column of the tile's first pixel in a plane row: the ring, rounded up to a dword
constexpr int DROWS = DT + 2 * DR;         // 84
constexpr int DPW = 24;                    // words of a plane row (96 columns)
constexpr int DWP = 24;                    // words of a weight row (21 taps, read in fours)

__device__ __forceinline__ int degrade_refl(int p, int n) {  // refl_index of bd.hip
  p = p < 0 ? -p : (p >= n ? 2 * (n - 1) - p : p);
  return min(max(p, 0), n - 1);
}

// pixels px .. px + 3 of a row of W pixels, those inside the row; v[i] = R | G << 8 | B << 16
__device__ __forceinline__ void degrade_store4(uint8_t *__restrict__ row, int px, int W, bool vec, const uint32_t (&v)[4]) {
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

// Philox4x32-10 (Salmon et al., Random123): counter c, key k -> c
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c[0] = hi1 ^ c[1] ^ k0, c[1] = lo1, c[2] = hi0 ^ c[3] ^ k1, c[3] = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
}

// rho = sqrt(-2 ln u), u = ((r >> 8) + 0.5) 2^-24, and phi = 2 pi (q >> 8) 2^-24: every operation rounded to float32 on its own
__device__ __forceinline__ void degrade_polar(uint32_t r, uint32_t q, float &rho, float &phi) {
#pragma clang fp contract(off)
  const float u = __fmaf_rn((float)(r >> 8), 0x1p-24f, 0x1p-25f);
  rho = sqrtf(-2.0f * logf(u));
  phi = 6.283185307179586f * ((float)(q >> 8) * 0x1p-24f);
}

// one sample: t = v + s z, s = sqrt(shot v + read^2), -> clamp(floor(t + 0.5), 0, 255)
__device__ __forceinline__ uint32_t degrade_noisy(int acc, float z, float read, float shot) {
#pragma clang fp contract(off)
  const float v = (float)acc * 0x1p-20f;
  const float a = shot * v, b = read * read;
  const float s = sqrtf(a + b);
  const float sz = s * z;
  const float t = v + sz;
  return (uint32_t)fminf(fmaxf(floorf(t + 0.5f), 0.0f), 255.0f);
}

__global__ __launch_bounds__(256) void degrade_kernel(const DegradeArgs a) {
  __shared__ uint32_t pl[3][DROWS][DPW];                        // R, G, B bytes: row y0 - 10 + i, columns x0 - 12 ... x0 + 83
  __shared__ __attribute__((aligned(16))) int wq[DK][DWP];  // the image's weights, 0 beyond ksize
  const int tid = threadIdx.x, img = blockIdx.y;
  const int H = a.H, W = a.W;
  const int tiles_x = (W + DT - 1) / DT;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * DT, x0 = tx * DT;
  const int64_t pitch = 3 * (int64_t)W;
  const uint8_t *src = a.src + img * a.src_stride;
  uint8_t *dst = a.dst + img * a.dst_stride;
  const int32_t *rec = a.table + (int64_t)EDVR_DEGRADE_RECORD_INTS * img;

  // (everything read from the record is uniform over the workgroup)
  int k = rec[DGR_KSIZE];
  if (k < 3 || k > DK || !(k & 1) || !a.weights) k = 0;  // any other value: no blur - every index below then stays inside LDS
  const int r = k >> 1, kk = max(k, 1), nj = (kk + 3) >> 2;
  const uint32_t read_bits = (uint32_t)rec[DGR_READ], shot_bits = (uint32_t)rec[DGR_SHOT];
  const bool noisy = (read_bits | shot_bits) != 0;

  // ---- 0. weights
  {
    const int32_t *w = a.weights + (k ? max(rec[DGR_WEIGHTS], 0) : 0);
    for (int i = tid; i < DK * DWP; i += 256) {
      const int row = i / DWP, col = i - row * DWP;
      int v = 0;
      if (k) {
        if (row < k && col < k) v = min(max(w[row * k + col], 0), 1 << 20);
      } else if (i == 0) {
        v = 1 << 20;
      }
      wq[row][col] = v;
    }
  }

  // ---- 1. fill: rows DR - r ... DR + DT + r - 1, quads (DL - r) / 4 ... (DL + DT - 1 + r) / 4
  {
    const int row0 = DR - r, nrows = DT + 2 * r;
    const int quad0 = (DL - r) >> 2, nquads = ((DL + DT - 1 + r) >> 2) - quad0 + 1;
    for (int item = tid; item < nrows * nquads; item += 256) {
      const int ri = item / nquads, row = row0 + ri, quad = quad0 + (item - ri * nquads);
      const int xs = x0 - DL + 4 * quad;
      const uint8_t *line = src + degrade_refl(y0 - DR + row, H) * pitch;
      uint32_t pr, pg, pb;
      if (a.src_vec && xs >= 0 && xs + 3 < W) {
        const uint32_t *p = reinterpret_cast<const uint32_t *>(line + 3 * (int64_t)xs);
        const uint32_t u0 = p[0], u1 = p[1], u2 = p[2];  // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        pr = (u0 & 255) | ((u0 >> 24) << 8) | (((u1 >> 16) & 255) << 16) | (((u2 >> 8) & 255) << 24);
        pg = ((u0 >> 8) & 255) | ((u1 & 255) << 8) | ((u1 >> 24) << 16) | (((u2 >> 16) & 255) << 24);
        pb = ((u0 >> 16) & 255) | (((u1 >> 8) & 255) << 8) | ((u2 & 255) << 16) | ((u2 >> 24) << 24);
      } else {
        pr = pg = pb = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint8_t *p = line + 3 * (int64_t)degrade_refl(xs + i, W);
          pr |= (uint32_t)p[0] << (8 * i), pg |= (uint32_t)p[1] << (8 * i), pb |= (uint32_t)p[2] << (8 * i);
        }
      }
      pl[0][row][quad] = pr, pl[1][row][quad] = pg, pl[2][row][quad] = pb;
    }
  }
  __syncthreads();

  // ---- 2. taps, 3. noise and store
  const int lane = tid & 63, quad = lane & 15;
  const int rsub = ((lane >> 4) & 1) * 2 + (lane >> 5);  // lanes 0 - 31: rows 0 and 2, lanes 32 - 63: rows 1 and 3
  const int first = DL + 4 * quad - r;                   // plane column under tap 0 of pixel 0
  const int sd = first >> 2;
  const uint32_t sh = (uint32_t)first & 3;               // = (DL - r) & 3: uniform
  const float read = __uint_as_float(read_bits), shot = __uint_as_float(shot_bits);
  const bool gray = rec[DGR_FLAGS] & EDVR_DEGRADE_GRAY;
  const uint32_t key_lo = (uint32_t)rec[DGR_KEY_LO], key_hi = (uint32_t)rec[DGR_KEY_HI], ctr_t = (uint32_t)rec[DGR_CTR_T];
  for (int pass = 0; pass < DT / 16; ++pass) {
    const int row = 16 * pass + 4 * (tid >> 6) + rsub, py = y0 + row, px = x0 + 4 * quad;
    if (py >= H || px >= W) continue;
    int acc[3][4] = {};
    for (int ka = 0; ka < kk; ++ka) {
      const int prow = row + DR - r + ka;
      uint32_t dc[3], vc[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint32_t d0 = pl[c][prow][sd];
        dc[c] = pl[c][prow][sd + 1];
        vc[c] = __builtin_amdgcn_alignbyte(dc[c], d0, sh);
      }
      for (int j = 0; j < nj; ++j) {
        const int4 w4 = *reinterpret_cast<const int4 *>(&wq[ka][4 * j]);
        const uint32_t w[4] = {(uint32_t)w4.x, (uint32_t)w4.y, (uint32_t)w4.z, (uint32_t)w4.w};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const uint32_t dn = pl[c][prow][sd + j + 2];
          const uint32_t vn = __builtin_amdgcn_alignbyte(dn, dc[c], sh);
          const uint32_t b[7] = {vc[c] & 255, (vc[c] >> 8) & 255, (vc[c] >> 16) & 255, vc[c] >> 24, vn & 255, (vn >> 8) & 255, (vn >> 16) & 255};
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[c][i] = (int)(__umul24(b[q + i], w[q]) + (uint32_t)acc[c][i]);
          dc[c] = dn, vc[c] = vn;
        }
      }
    }
    uint32_t v[4];
    if (!noisy) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        v[i] = (uint32_t)((acc[0][i] + (1 << 19)) >> 20) | ((uint32_t)((acc[1][i] + (1 << 19)) >> 20) << 8) | ((uint32_t)((acc[2][i] + (1 << 19)) >> 20) << 16);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint32_t c[4] = {(uint32_t)(px + i), (uint32_t)py, ctr_t, 0u};
        philox4x32_10(c, key_lo, key_hi);
        float rho, phi;
        degrade_polar(c[0], c[1], rho, phi);
        float zr, zg, zb;
        {
#pragma clang fp contract(off)
          zr = rho * cosf(phi);
          if (gray) {
            zg = zb = zr;
          } else {
            zg = rho * sinf(phi);
            degrade_polar(c[2], c[3], rho, phi);
            zb = rho * cosf(phi);
          }
        }
        v[i] = degrade_noisy(acc[0][i], zr, read, shot) | (degrade_noisy(acc[1][i], zg, read, shot) << 8) | (degrade_noisy(acc[2][i], zb, read, shot) << 16);
      }
    }
    degrade_store4(dst + py * pitch, px, W, a.dst_vec, v);
  }
}

__global__ void philox_words_kernel(uint32_t *__restrict__ dst, uint32_t key_lo, uint32_t key_hi, uint32_t ctr_t, int H, int W) {
  const int64_t total = (int64_t)H * W;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    uint32_t c[4] = {(uint32_t)x, (uint32_t)y, ctr_t, 0u};
    philox4x32_10(c, key_lo, key_hi);
    *reinterpret_cast<uint4 *>(dst + 4 * i) = make_uint4(c[0], c[1], c[2], c[3]);
  }
}

static inline bool degrade_aligned4(const void *p, int64_t stride, int n) {
  return reinterpret_cast<uintptr_t>(p) % 4 == 0 && (n == 1 || stride % 4 == 0);
}

}  // namespace edvr

extern "C" int edvr_degrade_u8(const uint8_t *src, uint8_t *dst, const int32_t *table, const int32_t *weights, int n, int H, int W,
                               int64_t src_image_stride, int64_t dst_image_stride, edvr_stream_t stream) {
  using namespace edvr;
  EDVR_REQUIRE(src && dst && table && n > 0 && n <= 65535 && H > 0 && W > 0, "degrade: bad arguments");
  EDVR_REQUIRE((int64_t)H * W <= (int64_t)1 << 29, "degrade: a %d x %d frame is too large", H, W);
  const int64_t frame = 3 * (int64_t)H * W;
  if (src_image_stride == 0) src_image_stride = frame;
  if (dst_image_stride == 0) dst_image_stride = frame;
  EDVR_REQUIRE(n == 1 || (src_image_stride >= frame && dst_image_stride >= frame), "degrade: an image stride is shorter than a frame of %lld bytes",
               (long long)frame);
  DegradeArgs a;
  a.src = src, a.dst = dst, a.table = table, a.weights = weights, a.H = H, a.W = W;
  a.src_stride = src_image_stride, a.dst_stride = dst_image_stride;
  a.src_vec = W % 4 == 0 && degrade_aligned4(src, src_image_stride, n);
  a.dst_vec = W % 4 == 0 && degrade_aligned4(dst, dst_image_stride, n);
  const dim3 grid((unsigned)(cdiv(W, DT) * cdiv(H, DT)), (unsigned)n);
  hipLaunchKernelGGL(degrade_kernel, grid, dim3(256), 0, as_stream(stream), a);
  return check_launch("degrade_kernel");
}

extern "C" int edvr_philox_words_u32(uint32_t *dst, uint32_t key_lo, uint32_t key_hi, uint32_t ctr_t, int H, int W, edvr_stream_t stream) {
  using namespace edvr;
  EDVR_REQUIRE(dst && H > 0 && W > 0 && (int64_t)H * W <= (int64_t)1 << 29, "philox_words: bad arguments");
  EDVR_REQUIRE(reinterpret_cast<uintptr_t>(dst) % 16 == 0, "philox_words: dst is not 16-byte aligned");
  const int64_t total = (int64_t)H * W;
  const unsigned blocks = (unsigned)std::min<int64_t>(cdiv64(total, 256), 65535);
  hipLaunchKernelGGL(philox_words_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), dst, key_lo, key_hi, ctr_t, H, W);
  return check_launch("philox_words_kernel");
}
