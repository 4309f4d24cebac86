// tsa_front_s.hip - the head of TSA fusion in ONE pass over the aligned features (gfx950): temporal attention and the two 1x1 convs
// that read its product (feat_fusion, spatial_attn1; edvr_arch.py:171-193).
//
// Three launches did this before: tsa_temporal_kernel wrote mod = aligned * sigmoid(<emb_j, emb_ref>) (as large as `aligned`), and
// conv1x1_split_kernel read it twice.  Nothing else reads `mod` in inference, so 4.4 of the 8.2 GB the three moved on the 10 x 5 x
// 128 x 180x320 layer only carried it from launch to launch.  Here a wave of conv1x1_split_kernel's frame (256 threads, a wave owns
// 32 pixels, weight slabs double-buffered in LDS, the activations streamed through a rotating register set) first takes the t
// probabilities of its pixels, then scales every value of `aligned` on its way into the split: `mod` lives in a register.
//
// Bit for bit what the three launches give:
//   * a probability is sigmoidf of the fma chain over the channels in their order, as tsa_temporal_body evaluates it; the pass leaves
//     them in LDS, [frame][pixel of the block] (which lane takes which chain - two mappings, below - does not change a chain);
//   * mod = aligned * prob is ONE fp32 multiply, then split with the scale conv1x1_split_kernel derives from `x_amax`;
//   * the products of a (pixel, output channel) enter its accumulator in that kernel's order: k-steps of 8 channels of cat_t(frames),
//     lane (half, j) owning channels 8 s + 4 half + i.  (The slabs here are 32 channels, not 64, so that both heads' weights fit the
//     LDS of two workgroups per CU; the steps past the last channel multiply zeros in either kernel and leave the sums alone.)
// Each head keeps its own packed buffer (edvr_conv2d_pack_weight_1x1s_f32) and scale; the epilogue is conv1x1_split_kernel's.
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "pack.h"

namespace edvr {

typedef float tf_f32x16 __attribute__((ext_vector_type(16)));
typedef int tf_i32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 tf_f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float tf_sigmoidf(float v) { return 1.f / (1.f + __expf(-v)); }  // elementwise.hip's sigmoidf, letter for letter

constexpr int TF_MAX_T = 16;

struct TsaFrontArgs {
  const float *emb, *emb_ref, *aligned;  // (b, t, c, hw), (b, c, hw) with its own image stride, (b, t, c, hw)
  int64_t ref_img_stride;
  const float *x_amax;
  const unsigned *wq[2];                 // per head: header (16 dwords: s_W, 1 / s_W) + [channel quad][128][4] dwords
  const float *bias[2];
  float *y[2];                           // (b, co, hw)
  float *y_amax[2];
  int act[2];
  int t, c, hw, co;
  int ci;                                // t * c rounded up to the 32-channel slab
  int seg_shift;                         // channels of `aligned` are addressed in segments of 1 << seg_shift planes (conv1x1.hip)
};

template <int MT, bool V4>  // 32-channel tiles per head: co <= 32 MT; V4: the attention pass on 16-byte loads (hw % 4 == 0, aligned planes)
__global__ __launch_bounds__(256, 2) void tsa_front_split_kernel(const TsaFrontArgs a) {
  constexpr int CK = 32, MB = 32 * MT, MB2 = 2 * MB, DEPTH = 8, COP = 128;
  constexpr int NW = (CK / 4) * MB2 / 256;  // 16-byte pieces per thread and slab
  constexpr int RSRC_FLAGS = 0x00020000;
  constexpr int OOB = (int)0x80000000;
  __shared__ __attribute__((aligned(16))) unsigned wsm[2][CK * MB2];
  __shared__ __attribute__((aligned(16))) float prob_s[TF_MAX_T][128];  // [frame][pixel of the block]
  const float s_x = split_scale(__builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, *a.x_amax))));
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, j = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hw = a.hw, t = a.t, c = a.c;
  const int img = blockIdx.z;
  const int p = (blockIdx.x * 4 + wave) * 32 + j;  // this lane's pixel
  const bool p_ok = p < hw;

  auto uniform_ptr = [&](const float *ptr) {
    const uint64_t pv = reinterpret_cast<uint64_t>(ptr);
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(pv >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)pv);
  };
  auto rsrc_at = [&](uint64_t base) { return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(base), (short)0, 0x7fffffff, RSRC_FLAGS); };
  const int64_t plane_bytes = (int64_t)hw * 4;
  const int64_t frame_bytes = (int64_t)c * plane_bytes;  // (2 frame_bytes < 2 GB: tsa_front_supported)

  // ---- weight slab staging: packed [channel quad][128][4] of either head -> slab [quad 8][head 2][MB][4]
  tf_i32x4 wr[NW];
  auto w_load = [&](int c0) {
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int e = tid + i * 256, q = e / MB2, col = e - q * MB2, hd = col / MB, cc = col - hd * MB;
      wr[i] = *reinterpret_cast<const tf_i32x4 *>(a.wq[hd] + 16 + ((int64_t)(c0 / 4 + q) * COP + cc) * 4);  // (zeros past the last channel: the packing fills whole 64-channel slabs)
    }
  };
  auto w_commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NW; ++i) *reinterpret_cast<tf_i32x4 *>(&wsm[buf][(tid + i * 256) * 4]) = wr[i];
  };

  // ---- temporal attention -> prob_s[frame][pixel of the block].  Every chain runs over the channels in their order.
  const uint64_t eb = uniform_ptr(a.emb + (int64_t)img * t * c * hw);
  const __amdgpu_buffer_rsrc_t ref_rs = rsrc_at(uniform_ptr(a.emb_ref + (int64_t)img * a.ref_img_stride));
  if constexpr (V4) {
    // hw % 4 == 0, 16-byte aligned planes: lane l of a half-wave takes the FOUR pixels 4 l .. 4 l + 3 of the block's 128 (one 16-byte
    // load per plane, 512 contiguous bytes per half-wave: the 128-byte rows of the operand layout below reach half the rate), the half-wave
    // (wave w, half) the frames 8 r + 2 w + half
    typedef float tf_f32x4 __attribute__((ext_vector_type(4)));
    const int px = blockIdx.x * 128 + 4 * j;
    const bool q_ok = px < hw;
    const int v_ref = q_ok ? px * 4 : OOB;
    for (int f0 = 2 * wave; f0 < t; f0 += 8) {
      const __amdgpu_buffer_rsrc_t rs = rsrc_at(eb + (uint64_t)(f0 * frame_bytes));
      const bool f_ok = f0 + half < t;
      const int v_emb = (q_ok && f_ok) ? (int)(half * frame_bytes) + px * 4 : OOB;
      tf_f32x4 dot = {0.f, 0.f, 0.f, 0.f};
      tf_f32x4 ra[8], ea[8], rb[8], eb2[8];
      auto load_grp = [&](int ch, tf_f32x4 (&r)[8], tf_f32x4 (&e)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          r[i] = __builtin_bit_cast(tf_f32x4, __builtin_amdgcn_raw_buffer_load_b128(ref_rs, v_ref, (ch + i) * hw * 4, 0));
          e[i] = __builtin_bit_cast(tf_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, v_emb, (ch + i) * hw * 4, 0));
        }
      };
      auto fma_grp = [&](const tf_f32x4 (&r)[8], const tf_f32x4 (&e)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int v = 0; v < 4; ++v) dot[v] = __builtin_fmaf(e[i][v], r[i][v], dot[v]);
      };
      load_grp(0, ra, ea);
      for (int ch = 0; ch < c; ch += 16) {  // c is a multiple of 8: groups of 8 channels, the next one in flight
        const bool second = ch + 8 < c;
        if (second) load_grp(ch + 8, rb, eb2);
        fma_grp(ra, ea);
        if (ch + 16 < c) load_grp(ch + 16, ra, ea);
        if (second) fma_grp(rb, eb2);
      }
      if (f_ok) {
        tf_f32x4 pr;
#pragma unroll
        for (int v = 0; v < 4; ++v) pr[v] = tf_sigmoidf(dot[v]);
        *reinterpret_cast<tf_f32x4 *>(&prob_s[f0 + half][4 * j]) = pr;
      }
    }
  } else {
    // any hw: lane (half, j) takes the frames 2 k + half of ITS pixel (the two halves of a wave would otherwise repeat each other's loads)
    const int npairs = (t + 1) >> 1;
    const int v_ref = p_ok ? p * 4 : OOB;
    const int v_emb = p_ok ? (int)(half * frame_bytes) + p * 4 : OOB;
    const bool last_ok = 2 * (npairs - 1) + half < t;  // odd t: the upper half has no frame in the last pair
    float dot[TF_MAX_T / 2];
#pragma unroll
    for (int k = 0; k < TF_MAX_T / 2; ++k) dot[k] = 0.f;
    float ra[8], rb[8], ea[TF_MAX_T / 2][8], eb2[TF_MAX_T / 2][8];
    auto load_grp = [&](int ch, float (&r)[8], float (&e)[TF_MAX_T / 2][8]) {
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ref_rs, v_ref, (ch + i) * hw * 4, 0));
#pragma unroll
      for (int k = 0; k < TF_MAX_T / 2; ++k)
        if (k < npairs) {
          const __amdgpu_buffer_rsrc_t rs = rsrc_at(eb + (uint64_t)(2 * k * frame_bytes));
          const int vo = (k + 1 < npairs || last_ok) ? v_emb : OOB;
#pragma unroll
          for (int i = 0; i < 8; ++i) e[k][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, vo, (ch + i) * hw * 4, 0));
        }
    };
    auto fma_grp = [&](const float (&r)[8], const float (&e)[TF_MAX_T / 2][8]) {
#pragma unroll
      for (int k = 0; k < TF_MAX_T / 2; ++k)
        if (k < npairs) {
#pragma unroll
          for (int i = 0; i < 8; ++i) dot[k] = __builtin_fmaf(e[k][i], r[i], dot[k]);
        }
    };
    load_grp(0, ra, ea);
    for (int ch = 0; ch < c; ch += 16) {
      const bool second = ch + 8 < c;
      if (second) load_grp(ch + 8, rb, eb2);
      fma_grp(ra, ea);
      if (ch + 16 < c) load_grp(ch + 16, ra, ea);
      if (second) fma_grp(rb, eb2);
    }
#pragma unroll
    for (int k = 0; k < TF_MAX_T / 2; ++k)
      if (k < npairs && (k + 1 < npairs || last_ok)) prob_s[2 * k + half][wave * 32 + j] = tf_sigmoidf(dot[k]);
  }

  // ---- the two 1x1 convs over cat_t(aligned_j * prob_j)
  const uint64_t ab = uniform_ptr(a.aligned + (int64_t)img * t * c * hw);
  const int voff = p_ok ? (4 * half * hw + p) * 4 : OOB;  // channel quad `half` of the eight; out-of-range pixels read as 0
  const int real_steps = t * c / 8;
  const int seg_mask = (1 << a.seg_shift) - 1;
  auto load_b = [&](int s, float (&v)[4]) {  // branch-free and all-scalar: a k-step past the last channel reads through an EMPTY resource (zeros)
    const int sc = __builtin_amdgcn_readfirstlane(s);
    const int cc = 8 * sc;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(ab + (uint64_t)((int64_t)(cc & ~seg_mask) * plane_bytes)), (short)0,
                                                                        sc < real_steps ? 0x7fffffff : 0, RSRC_FLAGS);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      v[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff, __builtin_amdgcn_readfirstlane(((cc & seg_mask) + i) * hw * 4), 0));
  };

  tf_f32x16 acc[2][MT];
#pragma unroll
  for (int hd = 0; hd < 2; ++hd)
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[hd][m][r] = 0.f;
  float bq[DEPTH][4];
  w_load(0);  // (ahead of the activation loads: the wait in front of its stores then leaves those in flight)
#pragma unroll
  for (int k = 0; k < DEPTH; ++k) load_b(k, bq[k]);
  w_commit(0);
  __syncthreads();  // (also: every wave's probabilities are in LDS)

  const int spf = c / 8;  // k-steps per frame
  int frame = 0, sf = 0;
  float pf = prob_s[0][wave * 32 + j];
  const int chunks = a.ci / CK;
  // one 32-channel slab = 4 k-steps = half of the rotating register set: slabs go in pairs so that every register index is a constant
  auto slab = [&](auto parity, int ch) {
    constexpr int P = decltype(parity)::value;
    const int buf = P;
    const bool more = ch + 1 < chunks;
    const unsigned *ws = wsm[buf] + (half * MB2 + j) * 4;
#pragma unroll
    for (int s = 0; s < CK / 8; ++s) {
      // next slab: asked for at the top of this one, stored into the idle buffer at its end.  Loads return in order, so the wait in front of
      // the stores also waits for every activation load issued before the request - those of the next four k-steps, due soon anyway; a
      // store any earlier would drain the activation stream's lookahead with it
      if (more && s == 0) w_load((ch + 1) * CK);
      if (sf == spf) {  // the next frame's probability (the steps past the last frame multiply zeros: any finite factor)
        sf = 0;
        frame = min(frame + 1, t - 1);
        pf = prob_s[frame][wave * 32 + j];
      }
      ++sf;
      const int slot = P * (CK / 8) + s;  // (a constant once unrolled)
      float mv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) mv[i] = bq[slot][i] * pf;  // mod: one fp32 multiply, never stored
      unsigned pk[4];
      split4_f16x2(mv, s_x, pk);
      load_b(ch * (CK / 8) + s + DEPTH, bq[slot]);  // same registers, DEPTH k-steps ahead
      tf_i32x4 b, br;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        b[q] = (int)pk[q];
        br[q] = (int)__builtin_amdgcn_alignbit(pk[q], pk[q], 16);
      }
#pragma unroll
      for (int hd = 0; hd < 2; ++hd) {
        tf_i32x4 av[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) av[m] = *reinterpret_cast<const tf_i32x4 *>(ws + ((2 * s) * MB2 + hd * MB + m * 32) * 4);
#pragma unroll
        for (int m = 0; m < MT; ++m)
          acc[hd][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(tf_f16x8, av[m]), __builtin_bit_cast(tf_f16x8, b), acc[hd][m], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < MT; ++m)
          acc[hd][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(tf_f16x8, av[m]), __builtin_bit_cast(tf_f16x8, br), acc[hd][m], 0, 0, 0);
      }
    }
    if (more) w_commit(buf ^ 1);
    // LDS-only barrier (the loads in flight target registers)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  };
  static_assert(DEPTH == 2 * (CK / 8), "two slabs rotate through the register set");
  for (int ch = 0; ch < chunks; ch += 2) {
    slab(std::integral_constant<int, 0>{}, ch);
    if (ch + 1 < chunks) slab(std::integral_constant<int, 1>{}, ch + 1);
  }

  // ---- epilogue of conv1x1_split_kernel, per head: lane (half, j) holds pixel p and channels m*32 + (r&3) + 8*(r>>2) + 4*half
#pragma unroll
  for (int hd = 0; hd < 2; ++hd) {
    const float inv_sw = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane((int)a.wq[hd][1]));
    const float unscale = inv_sw / s_x;
    const int act = a.act[hd];
    const float slope = act == EDVR_ACT_LRELU ? 0.1f : (act == EDVR_ACT_RELU ? 0.f : 1.f);
    const bool sig = act == EDVR_ACT_SIGMOID;
    float *y = a.y[hd] + (int64_t)img * a.co * hw;
    const float *bias = a.bias[hd];
    unsigned vmax = 0u;  // max |y| as a bit pattern: NaNs order above +inf (sticky for the host's overflow guard)
    if (p_ok) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          if (co < a.co) {
            float v = __builtin_fmaf(acc[hd][m][r], unscale, bias[co]);
            v = sig ? __builtin_amdgcn_rcpf(1.f + __expf(-v)) : fmaxf(v, slope * v);
            y[(int64_t)co * hw + p] = v;
            vmax = max(vmax, __builtin_bit_cast(unsigned, v) & 0x7fffffffu);
          }
        }
    }
    if (a.y_amax[hd]) {
#pragma unroll
      for (int sh = 32; sh > 0; sh >>= 1) vmax = max(vmax, (unsigned)__shfl_xor((int)vmax, sh));
      if (lane == 0) publish_amax(a.y_amax[hd], vmax);
    }
  }
}

// what the kernel itself takes
static bool tsa_front_supported(int b, int t, int c, int h, int w, int co) {
  if (b <= 0 || t <= 0 || c <= 0 || h <= 0 || w <= 0 || co <= 0) return false;
  if (b > 65535 || t > TF_MAX_T || (c & 7) || co > 128) return false;
  const int64_t hw = (int64_t)h * w;
  return 2 * (int64_t)c * hw * 4 < ((int64_t)1 << 31) && hw * 32 < ((int64_t)1 << 31);  // a frame pair / 8 planes inside a 32-bit buffer offset
}

static bool tsa_front_enabled() {
  static const bool on = []() {
    const char *e = getenv("EDVR_TSA_FRONT");  // "0": the three launches instead
    return !(e && e[0] == '0');
  }();
  return on;
}

}  // namespace edvr

extern "C" {

int edvr_tsa_front_supported(int b, int t, int c, int h, int w, int co) { return edvr::tsa_front_supported(b, t, c, h, w, co) ? 1 : 0; }

int edvr_tsa_front_applies(int needs_grad, int b, int t, int c, int h, int w, int co_feat, int co_attn, int ks_feat, int ks_attn, int has_bias_feat,
                           int has_bias_attn, const void *wq_feat, const void *wq_attn, const float *x_amax) {
  using namespace edvr;
  if (!tsa_front_enabled() || needs_grad || co_feat != co_attn || ks_feat != 1 || ks_attn != 1 || !has_bias_feat || !has_bias_attn) return 0;
  if (!wq_feat || !wq_attn || !x_amax || !tsa_front_supported(b, t, c, h, w, co_feat)) return 0;
  if ((reinterpret_cast<uintptr_t>(wq_feat) & 15) || (reinterpret_cast<uintptr_t>(wq_attn) & 15)) return 0;
  // ... and only where each of the two convs would run on conv1x1_split_kernel: this kernel reproduces THAT kernel's sums
  edvr_conv2d_desc d = {};
  d.c1 = t * c; d.n = b; d.h = h; d.w = w; d.co = co_feat; d.ks = 1; d.stride = 1;
  d.out_mode = EDVR_OUT_NCHW; d.algo = EDVR_CONV_AUTO;
  d.wpk_f4s = wq_feat; d.x_amax = x_amax;
  return conv2d_select(d) == CONV_1X1_SPLIT ? 1 : 0;
}

int edvr_tsa_front_f32(const float *emb, const float *emb_ref, int64_t emb_ref_img_stride, const float *aligned, const float *x_amax,
                       const void *wq_feat, const float *bias_feat, int act_feat, float *feat, float *feat_amax, const void *wq_attn,
                       const float *bias_attn, int act_attn, float *attn, float *attn_amax, int b, int t, int c, int h, int w, int co,
                       edvr_stream_t stream) {
  using namespace edvr;
  EDVR_REQUIRE(emb && emb_ref && aligned && x_amax && wq_feat && wq_attn && bias_feat && bias_attn && feat && attn, "tsa_front: null pointer");
  EDVR_REQUIRE(tsa_front_supported(b, t, c, h, w, co), "tsa_front: unsupported shape (b %d, t %d <= 16, c %d %% 8 == 0, %d x %d, co %d <= 128)", b, t, c, h, w, co);
  EDVR_REQUIRE((reinterpret_cast<uintptr_t>(wq_feat) & 15) == 0 && (reinterpret_cast<uintptr_t>(wq_attn) & 15) == 0,
               "tsa_front: packed weights must be 16-byte aligned");
  EDVR_REQUIRE(emb_ref_img_stride >= (int64_t)c * h * w || b == 1, "tsa_front: emb_ref image stride %lld", (long long)emb_ref_img_stride);
  TsaFrontArgs a;
  a.emb = emb; a.emb_ref = emb_ref; a.aligned = aligned;
  a.ref_img_stride = emb_ref_img_stride;
  a.x_amax = x_amax;
  a.wq[0] = static_cast<const unsigned *>(wq_feat); a.wq[1] = static_cast<const unsigned *>(wq_attn);
  a.bias[0] = bias_feat; a.bias[1] = bias_attn;
  a.y[0] = feat; a.y[1] = attn;
  a.y_amax[0] = feat_amax; a.y_amax[1] = attn_amax;
  a.act[0] = act_feat; a.act[1] = act_attn;
  a.t = t; a.c = c; a.hw = h * w; a.co = co;
  a.ci = (t * c + 31) / 32 * 32;
  a.seg_shift = 30;
  while (((int64_t)1 << a.seg_shift) * a.hw * 4 >= ((int64_t)1 << 31)) --a.seg_shift;
  if (a.seg_shift < 3) a.seg_shift = 3;
  const dim3 grid(cdiv(a.hw, 128), 1, b);
  const bool v4 = (a.hw & 3) == 0 && (emb_ref_img_stride & 3) == 0 && ((reinterpret_cast<uintptr_t>(emb) | reinterpret_cast<uintptr_t>(emb_ref)) & 15) == 0;
  if (co <= 64) {
    if (v4) hipLaunchKernelGGL((tsa_front_split_kernel<2, true>), grid, dim3(256), 0, as_stream(stream), a);
    else hipLaunchKernelGGL((tsa_front_split_kernel<2, false>), grid, dim3(256), 0, as_stream(stream), a);
  } else {
    if (v4) hipLaunchKernelGGL((tsa_front_split_kernel<4, true>), grid, dim3(256), 0, as_stream(stream), a);
    else hipLaunchKernelGGL((tsa_front_split_kernel<4, false>), grid, dim3(256), 0, as_stream(stream), a);
  }
  return check_launch("tsa_front_split_kernel");
}

}  // extern "C"
