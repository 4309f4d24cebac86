// conv2d_s.hip - the direct implicit-GEMM convolution of conv2d.hip with SPLIT fp32 operands on the f16 matrix pipe (gfx950): the
// 3x3 / stride-2 convs of the pyramid, conv_first (3 input channels) and the 1x1 convs below the streaming kernel's 320 channels -
// every conv that no Winograd / streaming kernel takes and that ran on v_mfma_f32_32x32x2_f32 until now.
//
// Same structure as conv2d_mfma_kernel: 256 threads own TH x TW output pixels x 32 MT output channels, the input halo of a chunk of
// channels is staged in LDS, the global loads of chunk c + 1 are issued before the MFMA block of chunk c.  What changes is the
// arithmetic (conv1x1_s.hip, winograd_f4s.hip): every operand travels as ONE dword (f16 hi | f16 lo << 16) of x * s, s a power of two -
//   * weights: packed once per parameter version as [channel quad][tap][co'][4 channels] dwords of w * s_W behind a 64-byte header
//     (s_W from max |w|; with one tap this is conv1x1_s.hip's layout: one packing routine serves both).  A chunk's slab is copied to
//     LDS as it is; a lane's A operand - four channels x (hi, lo) of its output channel - is ONE ds_read_b128;
//   * activations: the thread that prefetched the 8 channels of a halo position splits them when the chunk is committed (two
//     instructions per element; s_X from `x_amax`) and writes two 16-byte cells [quad][position][4]; the B operand of a tap is ONE
//     ds_read_b128, and the second MFMA of a pair takes B rotated by 16 bits ((lo, hi): the cross terms).
//   * stride 2: even and odd halo columns lie in separate runs of a row, so the 32 lanes of a tap read consecutive cells.
// Per 8 channels, tap and wave 2 MT NS v_mfma_f32_32x32x16_f16 of 32 cycles where the fp32 kernel issues 4 MT NS
// v_mfma_f32_32x32x2_f32 of 64.  1 / (s_W s_X) leaves in the bias fma of the epilogue; `y_amax` (optional) receives max |y|.
#include <algorithm>

#include "common.h"
#include "conv_launch.h"
#include "pack.h"

namespace edvr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int cds_i32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 cds_f16x8 __attribute__((ext_vector_type(8)));

struct ConvSArgs {
  edvr_conv2d_desc d;
  const unsigned *wq;  // header (16 dwords: s_W, 1 / s_W) + [channel quad][tap][cop][4] dwords
  int ci, cop, ho, wo, tiles_x, tiles_y;
  int co_start;        // first output channel of this launch (the tail launch covers the last partial 128-block)
};

template <int KS, int STRIDE, int SW>
struct ConvSGeom {
  static constexpr int CK = (KS == 1) ? 32 : 8;  // input channels staged per chunk
  // LDS row pitch in 16-byte cells.  With 16-pixel rows the lanes 16-31 of a tap read the next output row: that row must start a
  // multiple of 16 cells (256 bytes = all banks) further on, or the two rows of one ds_read_b128 lane group share banks.
  static constexpr int IW = (SW - 1) * STRIDE + KS;
  static constexpr int RSP = (SW == 16 && KS > 1) ? (IW + 16 / STRIDE - 1) / (16 / STRIDE) * (16 / STRIDE) : IW;
};

template <int KS, int STRIDE, int MT, int SW, int NS>
__global__ __launch_bounds__(256, 2) void conv2d_split_kernel(const ConvSArgs a) {
  using G = ConvSGeom<KS, STRIDE, SW>;
  constexpr int SH = 32 / SW;      // rows of one 32-pixel subtile
  constexpr int TW = SW;           // output tile width
  constexpr int TH = 4 * NS * SH;  // output tile height (4 waves)
  constexpr int IW = G::IW, IH = (TH - 1) * STRIDE + KS;
  constexpr int IWH = (IW + 1) / 2;  // stride 2: cells of the even-column run of a row
  constexpr int RSP = G::RSP;
  constexpr int NPOS = IH * IW;      // halo positions (what the threads enumerate)
  constexpr int NCELL = IH * RSP;    // cells of one channel quad
  constexpr int CK = G::CK, NQ = CK / 4, OCT = CK / 8;
  constexpr int KK = KS * KS, PAD = KS / 2;
  constexpr int MB = 32 * MT;
  constexpr int WPIECES = NQ * KK * MB;         // 16-byte pieces of a chunk's weight slab
  constexpr int NW = (WPIECES + 255) / 256;
  constexpr int NIT = (NPOS * OCT + 255) / 256;  // (position, channel octet) items per thread

  __shared__ __attribute__((aligned(16))) unsigned smem[(NQ * NCELL + WPIECES) * 4];
  unsigned *xs = smem;                    // [quad][cell][4]
  unsigned *wsm = smem + NQ * NCELL * 4;  // [quad][tap][co' MB][4]

  const edvr_conv2d_desc &d = a.d;
  const float s_x = split_scale(__builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, *d.x_amax))));
  const float inv_sw = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane((int)a.wq[1]));
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, half = lane >> 5, j = lane & 31;
  int tile = blockIdx.x, blk_y = blockIdx.y, img = blockIdx.z;
  if constexpr (KS > 1) xcd_block_index(tile, blk_y, img);  // neighbouring tiles share one XCD's L2 (common.h); 1x1 has no halo
  const int ty0 = (tile / a.tiles_x) * TH, tx0 = (tile % a.tiles_x) * TW;
  const int co_blk = a.co_start + blk_y * MB;

  const float *x1 = d.x1 + (int64_t)img * d.x1_img_stride;
  const float *x2 = nullptr;
  if (d.x2) {
    const int i2 = d.x2_div > 0 ? (img / d.x2_div) * d.x2_mul + d.x2_add : img;
    x2 = d.x2 + (int64_t)i2 * d.x2_img_stride;
  }
  const int hw = d.h * d.w;

  // per-lane LDS read bases (dwords): B operand (cell of the subtile's pixel at tap (0, 0)) and A operand, both of channel quad `half`
  int bbase[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int r = (wave * NS + s) * SH + j / SW, c = j % SW;
    bbase[s] = (half * NCELL + (r * STRIDE) * RSP + c) * 4;
  }
  const int abase = (half * KK * MB + j) * 4;

  f32x16 acc[MT][NS];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][s][r] = 0.f;

  const int iy0 = ty0 * STRIDE - PAD, ix0 = tx0 * STRIDE - PAD;

  // ---- software pipeline as in conv2d_mfma_kernel: unconditional clamped loads.  The values are selected (0 outside the image / past
  // the last channel) only when the chunk is committed: a select next to its load makes the compiler wait for every load in turn
  int xoff[NIT], xcell[NIT], xoct[NIT];  // offset inside a channel plane (-1: outside the image / no item), LDS cell, channel octet
#pragma unroll
  for (int k = 0; k < NIT; ++k) {
    const int it = tid + k * 256;
    const int oct = OCT == 1 ? 0 : it / NPOS, p = it - oct * NPOS;
    const int iy = p / IW, ix = p - iy * IW;
    const int gy = iy0 + iy, gx = ix0 + ix;
    xoff[k] = (it < NPOS * OCT && gy >= 0 && gy < d.h && gx >= 0 && gx < d.w) ? gy * d.w + gx : -1;
    xcell[k] = iy * RSP + (STRIDE == 2 ? (ix & 1) * IWH + (ix >> 1) : ix);
    xoct[k] = oct;
  }
  float xr[NIT][8];
  cds_i32x4 wr[NW];
  auto prefetch = [&](int c0) {
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int e = tid + i * 256;
      const bool ok = (i + 1) * 256 <= WPIECES || e < WPIECES;
      const int row = ok ? e / MB : 0, col = ok ? e - row * MB : 0;  // row = quad * KK + tap of the chunk
      wr[i] = *reinterpret_cast<const cds_i32x4 *>(a.wq + 16 + ((int64_t)((c0 >> 2) * KK + row) * a.cop + co_blk + col) * 4);
    }
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = c0 + xoct[k] * 8 + e;
        const int cc = c < a.ci ? c : 0;
        const float *src = (cc < d.c1) ? (x1 + (int64_t)cc * hw) : (x2 + (int64_t)(cc - d.c1) * hw);
        xr[k][e] = src[(c < a.ci && xoff[k] >= 0) ? xoff[k] : 0];
      }
    }
  };
  auto commit = [&](int c0) {
#pragma unroll
    for (int i = 0; i < NW; ++i)
      if ((i + 1) * 256 <= WPIECES || tid + i * 256 < WPIECES) *reinterpret_cast<cds_i32x4 *>(wsm + (tid + i * 256) * 4) = wr[i];
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      if ((k + 1) * 256 <= NPOS * OCT || tid + k * 256 < NPOS * OCT) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          float v4[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v4[e] = (c0 + xoct[k] * 8 + 4 * q + e < a.ci && xoff[k] >= 0) ? xr[k][4 * q + e] : 0.f;
          unsigned pk[4];
          split4_f16x2(v4, s_x, pk);
          *reinterpret_cast<cds_i32x4 *>(xs + ((xoct[k] * 2 + q) * NCELL + xcell[k]) * 4) = cds_i32x4{(int)pk[0], (int)pk[1], (int)pk[2], (int)pk[3]};
        }
      }
    }
  };

  prefetch(0);
  commit(0);
  __syncthreads();
  for (int c0 = 0; c0 < a.ci; c0 += CK) {
    const bool more = (c0 + CK) < a.ci;
    if (more) prefetch(c0 + CK);
    // ---- MFMA over (8 channels, tap): every operand one ds_read_b128 at base + immediate
#pragma unroll
    for (int s8 = 0; s8 < OCT; ++s8) {
#pragma unroll
      for (int t = 0; t < KK; ++t) {
        const int kh = t / KS, kw = t % KS;
        const int tapcell = kh * RSP + (STRIDE == 2 ? (kw & 1) * IWH + (kw >> 1) : kw);
        cds_i32x4 av[MT], bv[NS], br[NS];
#pragma unroll
        for (int m = 0; m < MT; ++m) av[m] = *reinterpret_cast<const cds_i32x4 *>(wsm + abase + ((2 * s8 * KK + t) * MB + m * 32) * 4);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          bv[s] = *reinterpret_cast<const cds_i32x4 *>(xs + bbase[s] + (2 * s8 * NCELL + tapcell) * 4);
#pragma unroll
          for (int q = 0; q < 4; ++q) br[s][q] = (int)__builtin_amdgcn_alignbit((unsigned)bv[s][q], (unsigned)bv[s][q], 16);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int s = 0; s < NS; ++s)
            acc[m][s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(cds_f16x8, av[m]), __builtin_bit_cast(cds_f16x8, bv[s]), acc[m][s], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int s = 0; s < NS; ++s)
            acc[m][s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(cds_f16x8, av[m]), __builtin_bit_cast(cds_f16x8, br[s]), acc[m][s], 0, 0, 0);
      }
    }
    if (more) {
      __syncthreads();  // every wave is done reading this chunk
      commit(c0 + CK);
      __syncthreads();
    }
  }

  // ---- epilogue on the accumulators: un-scale + bias, activation (uniform switch hoisted), residuals, store, max |y|
  {
    const float unscale = inv_sw / s_x;
    float bvals[MT * 16];
#pragma unroll
    for (int i = 0; i < MT * 16; ++i) bvals[i] = 0.f;
    if (d.bias) {  // unconditional clamped loads (a predicated load would serialise: one basic block + wait per element)
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = co_blk + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          bvals[m * 16 + r] = d.bias[co < d.co ? co : d.co - 1];
        }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[m][s][r] = __builtin_fmaf(acc[m][s][r], unscale, bvals[m * 16 + r]);
  }
  if (d.act != EDVR_ACT_NONE) {
    const int rel_from = d.act_from - co_blk - 4 * half;  // activation applies where (m*32 + row(r)) >= rel_from
#define EDVR_ACT_LOOP(EXPR)                                             \
  _Pragma("unroll") for (int m = 0; m < MT; ++m)                        \
  _Pragma("unroll") for (int r = 0; r < 16; ++r) {                      \
    if (m * 32 + (r & 3) + 8 * (r >> 2) >= rel_from) {                  \
      _Pragma("unroll") for (int s = 0; s < NS; ++s) {                  \
        const float v = acc[m][s][r];                                   \
        acc[m][s][r] = (EXPR);                                          \
      }                                                                 \
    }                                                                   \
  }
    if (d.act == EDVR_ACT_LRELU) {
      EDVR_ACT_LOOP(v > 0.f ? v : 0.1f * v)
    } else if (d.act == EDVR_ACT_RELU) {
      EDVR_ACT_LOOP(fmaxf(v, 0.f))
    } else {
      EDVR_ACT_LOOP(__builtin_amdgcn_rcpf(1.f + __expf(-v)))
    }
#undef EDVR_ACT_LOOP
  }
  // per-image offsets fit 32 bits (co * ho * wo < 2^31); uniform conditions are hoisted out of the store loops
  const int plane = a.ho * a.wo;
  float *y = d.y + (int64_t)img * d.y_img_stride;
  const float *r1 = d.res1 ? d.res1 + (int64_t)img * d.res1_img_stride : nullptr;
  const float *r2 = d.res2 ? d.res2 + (int64_t)img * d.res2_img_stride : nullptr;
  const int co_lane = co_blk + 4 * half;
  unsigned vmax = 0u;  // max |y| as a bit pattern: non-negative floats order as integers, NaNs above +inf (sticky for the host's overflow guard)
#define EDVR_STORE_LOOP(BODY)                                                      \
  _Pragma("unroll") for (int s = 0; s < NS; ++s) {                                 \
    const int oy = ty0 + (wave * NS + s) * SH + j / SW, ox = tx0 + j % SW;         \
    if (oy < a.ho && ox < a.wo) {                                                  \
      const int pix = oy * a.wo + ox;                                              \
      _Pragma("unroll") for (int m = 0; m < MT; ++m) {                             \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                           \
          const int co = co_lane + m * 32 + (r & 3) + 8 * (r >> 2);                \
          if (co < d.co) {                                                         \
            float v = acc[m][s][r];                                                \
            const int o = co * plane + pix;                                        \
            BODY                                                                   \
            y[o] = v;                                                              \
            vmax = max(vmax, __builtin_bit_cast(unsigned, v) & 0x7fffffffu);       \
          }                                                                        \
        }                                                                          \
      }                                                                            \
    }                                                                              \
  }
  if (r1 && r2) {
    EDVR_STORE_LOOP({ v += r1[o] + r2[o]; })
  } else if (r1) {
    EDVR_STORE_LOOP({ v += r1[o]; })
  } else {
    EDVR_STORE_LOOP({})
  }
#undef EDVR_STORE_LOOP
  if (d.y_amax) {  // max |y| for the next layer's bound: at most one atomic per wave
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) vmax = max(vmax, (unsigned)__shfl_xor((int)vmax, sh));
    if (lane == 0) publish_amax(d.y_amax, vmax);  // (conv_first: 90 k unconditional atomics on the one slot cost more than the convolution)
  }
}

// ---- weight packing, shared with conv1x1_s.hip (kk = 1)
// header[0] = s_W = 2^e with max|w| s_W in [2^14, 2^15), header[1] = 1 / s_W
__global__ __launch_bounds__(1024) void conv_split_scale_kernel(const float *__restrict__ w, unsigned *__restrict__ wq, int64_t total) {
  __shared__ float red[16];
  float m = 0.f;
  for (int64_t i = threadIdx.x; i < total; i += 1024) m = fmaxf(m, fabsf(w[i]));
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) m = fmaxf(m, __shfl_xor(m, sh));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 16; ++i) m = fmaxf(m, red[i]);
    const unsigned field = f4s_weight_scale_field(__builtin_bit_cast(unsigned, m));
    wq[0] = field << 23;
    wq[1] = (254u - field) << 23;
    for (int i = 2; i < 16; ++i) wq[i] = 0u;
  }
}

// w (co, ci, k, k) -> [channel quad][tap][cop][4 channels] dwords (hi | lo << 16) of w * s_W, zero beyond co / ci
__global__ void conv_split_pack_kernel(const float *__restrict__ w, unsigned *__restrict__ wq, int co, int ci, int kk, int cop, int quads) {
  const float s_w = __builtin_bit_cast(float, wq[0]);
  const int64_t total = (int64_t)quads * kk * cop;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int o = (int)(i % cop), t = (int)((i / cop) % kk), q = (int)(i / ((int64_t)cop * kk));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * q + e;
      wq[16 + i * 4 + e] = (o < co && c < ci) ? split_f16x2(w[((int64_t)o * ci + c) * kk + t], s_w) : 0u;
    }
  }
}

int conv_split_pack(const float *w, unsigned *wq, int co, int ci, int kk, int cop, int quads, hipStream_t stream) {
  hipLaunchKernelGGL(conv_split_scale_kernel, dim3(1), dim3(1024), 0, stream, w, wq, (int64_t)co * ci * kk);
  const int64_t total = (int64_t)quads * kk * cop;
  hipLaunchKernelGGL(conv_split_pack_kernel, dim3((unsigned)std::min<int64_t>(cdiv64(total, 256), 2048)), dim3(256), 0, stream, w, wq, co, ci, kk,
                     cop, quads);
  return check_launch("conv_split_pack_kernel");
}

static inline int ds_quads(int ci, int ks) { return round_up(ci, ks == 1 ? 32 : 8) / 4; }  // whole chunks: the slab copy never leaves the buffer

struct SplitLaunch {  // conv_launch.h
  template <int KS, int STRIDE, int MT, int SW, int NS>
  static int launch(dim3 grid, const ConvSArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL((conv2d_split_kernel<KS, STRIDE, MT, SW, NS>), grid, dim3(256), 0, stream, a);
    return check_launch("conv2d_split_kernel");
  }
};

bool conv2d_split_eligible(const edvr_conv2d_desc &d) {
  if (!d.wpk_ds || !d.x_amax || d.algo == EDVR_CONV_DIRECT) return false;
  if ((reinterpret_cast<uintptr_t>(d.wpk_ds) & 15) != 0) return false;
  if (!((d.ks == 3 && (d.stride == 1 || d.stride == 2)) || (d.ks == 1 && d.stride == 1))) return false;
  if (d.out_mode != EDVR_OUT_NCHW || d.gate || d.pre || d.abs_sum) return false;
  if (d.y_scale != 0.f && d.y_scale != 1.f) return false;
  if (d.x2 && (d.c1 & 3)) return false;  // a channel quad must not straddle x1 / x2
  return true;
}

int conv2d_split_launch(const edvr_conv2d_desc &d, hipStream_t stream) {
  ConvSArgs a;
  a.d = d;
  a.wq = reinterpret_cast<const unsigned *>(d.wpk_ds);
  a.ci = d.c1 + d.c2;
  a.cop = round_up(d.co, 32);
  const int pad = d.ks / 2;
  a.ho = (d.h + 2 * pad - d.ks) / d.stride + 1;
  a.wo = (d.w + 2 * pad - d.ks) / d.stride + 1;
  a.tiles_x = a.tiles_y = 0;
  a.co_start = 0;
  return launch_direct<SplitLaunch>(a, stream);
}

}  // namespace edvr

extern "C" {

size_t edvr_conv2d_packed_weight_ds_elems(int co, int ci, int ks) {
  if (co <= 0 || ci <= 0 || (ks != 1 && ks != 3)) return 0;
  return 16 + (size_t)edvr::ds_quads(ci, ks) * ks * ks * edvr::round_up(co, 32) * 4;
}

int edvr_conv2d_pack_weight_ds_f32(const float *w, void *wpk_ds, int co, int ci, int ks, edvr_stream_t stream) {
  using namespace edvr;
  EDVR_REQUIRE(w && wpk_ds && co > 0 && ci > 0 && (ks == 1 || ks == 3), "pack_weight_ds: bad arguments");
  EDVR_REQUIRE((reinterpret_cast<uintptr_t>(wpk_ds) & 15) == 0, "pack_weight_ds: wpk_ds must be 16-byte aligned");
  return conv_split_pack(w, static_cast<unsigned *>(wpk_ds), co, ci, ks * ks, round_up(co, 32), ds_quads(ci, ks), as_stream(stream));
}

}  // extern "C"
