// telecine.hip - inverse telecine on the device, on the byte planes, BEFORE colour conversion: the two kernels behind
// y4m.inverse_telecined / restore_y4m(deinterlace='film').  Film shown as interlaced video (2:3 pulldown: 24000/1001 frames/s stretched to
// 60000/1001 fields/s) holds every film frame in full, split over two or three fields; the metrics kernel measures, per frame, which
// neighbouring field completes its first field and how much it repeats the frame before, the host decides (edvr_amd/telecine.py), and
// the weave kernel puts the matching fields back together: the output is the film frame, bit for bit.  Replaces nothing in the
// reference: it is the `ffmpeg -vf fieldmatch,decimate` pass people otherwise run in front of the pipe.
//
// Definition (integers only; no bit-compatibility with fieldmatch / decimate or TIVTC is claimed).  q: the row parity
// of a frame's first field (0 top field first, 1 bottom field first), L_i: the luma plane of frame i (R rows, C columns), sh = depth - 8.
//   T1  candidates: W_c(i) = L_i; W_p(i): rows of parity q from L_i, the others from L_(i-1); W_p = W_c where frame i - 1 does not exist
//   T2  comb, 1 <= y <= R - 2: d1 = W[y,x] - W[y-1,x], d2 = W[y,x] - W[y+1,x]; k = min(|d1|, |d2|) where both are > 0 or both < 0, else 0
//   T3  S(W) = sum of max(k - (nt << sh), 0)
//   T4  blocks of 16 x 16 luma samples anchored at (0, 0): cnt = #{k > (ct << sh)}, mic(W) = the largest cnt of any block
//   T5  A_i = sum of |L_i - L_(i-1)| over the rows of parity q, B_i over the rows of parity 1 - q, C_i = sum of |L_i - L_(i-2)| over the
//       rows of parity 1 - q; a term whose earlier frame does not exist is 0
// T6 - T8 (match, duplicate score, decimation) are host arithmetic on the table; T9 is the weave.
//
// field_match_kernel: one launch for all n frames (blockIdx.z), luma only.  A lane owns 16 adjacent samples of one row; a wave is 16 rows
// x 4 lanes - four whole 16 x 16 blocks of T4, whose counts are complete after four xor-shuffles (no LDS, no barrier per tile) - and the
// four waves of a workgroup lie side by side: a tile of 16 rows x 256 columns on the block grid.  A workgroup walks its strip of 16 rows
// tile by tile (blockIdx.y of gridDim.y), carries five 64-bit sums and two running maxima, and ends with ONE 64-bit integer atomic add
// per non-zero sum and one integer atomic max per non-zero mic.  Per lane: rows y - 1, y, y + 1 of L_i, row y of L_(i-1), and either rows
// y - 1, y + 1 of L_(i-1) (y of parity q) or row y of L_(i-2): the plane crosses HBM once, its row neighbours and the two earlier frames
// come from the cache.  Whole 16-sample accesses of any alignment where the run lies inside the row, clamped single samples at its end.
// Integer sums: the result does not depend on the batching or on the grid.  192 bytes of LDS, no float, 0 bytes of scratch.
//
// field_weave_kernel: one launch for a list of output frames (blockIdx.y), all three planes, row by row: a lane moves 16 BYTES of a row
// (sample size does not matter to a copy) - whole where they lie inside the row, byte by byte at its end.
#include <algorithm>
#include <cstdint>

#include "common.h"

namespace edvr {

constexpr int FM_RUN = 16;        // samples of a lane
constexpr int FM_TILE_W = 256;    // columns of a workgroup's tile: 4 waves x 4 lanes x 16 samples
constexpr int FM_TILE_H = 16;     // rows of a wave, of a tile and of a T4 block
constexpr int FM_COLS = 7;        // S_c, S_p, mic_c, mic_p, A, B, C
constexpr int FM_TARGET_WGS = 2048;

struct MatchArgs {
  const uint8_t *yuv, *prev, *prev2;  // the batch; frame -1, frame -2 (dense) or null
  unsigned long long *table;          // (n, 7), cleared before the launch
  int64_t in_stride;                  // BYTES between the frames of the batch
  int R, C, gx;                       // luma rows, columns, tiles per strip
  int q, nt, ct;                      // first field's row parity; nt << sh, ct << sh
};

// 16 samples row[x] ... row[x + 15], packed little-endian as memory holds them: one access of any alignment where all lie inside the
// row, otherwise one by one with the column clamped to the row
template <typename T>
__device__ __forceinline__ void fm_load(const T *__restrict__ row, int x, int C, bool inside, uint32_t (&v)[FM_RUN * (int)sizeof(T) / 4]) {
  constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  if (inside) {
    __builtin_memcpy(v, row + x, FM_RUN * sizeof(T));
  } else {
#pragma unroll
    for (int m = 0; m < FM_RUN; ++m) {
      const uint32_t s = (uint32_t)row[min(x + m, C - 1)] << (BITS * (m % PER));
      v[m / PER] = (m % PER) == 0 ? s : (v[m / PER] | s);
    }
  }
}

template <typename T>
__device__ __forceinline__ int fm_get(const uint32_t *v, int m) {
  constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  return (int)((v[m / PER] >> (BITS * (m % PER))) & ((1u << BITS) - 1u));
}

// T2
__device__ __forceinline__ int fm_comb(int up, int mid, int dn) {
  const int d1 = mid - up, d2 = mid - dn;
  const int lo = min(d1, d2), hi = max(d1, d2);
  return lo > 0 ? lo : (hi < 0 ? -hi : 0);
}

template <typename T>
__global__ __launch_bounds__(256) void field_match_kernel(const MatchArgs a) {
  constexpr int WORDS = FM_RUN * (int)sizeof(T) / 4;
  const int i = blockIdx.z;
  const uint8_t *cur = a.yuv + (int64_t)i * a.in_stride;
  const uint8_t *p1 = i >= 1 ? cur - a.in_stride : a.prev;
  const uint8_t *p2 = i >= 2 ? cur - 2 * a.in_stride : (i == 1 ? a.prev : a.prev2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int R = a.R, C = a.C;
  const int y = blockIdx.x * FM_TILE_H + (lane >> 2);
  const bool same = (y & 1) == a.q;            // a row of the first field
  const bool interior = y >= 1 && y <= R - 2;  // T2: the first and last row have k = 0
  const int64_t ry = (int64_t)min(y, R - 1) * C, ru = (int64_t)max(min(y, R - 1) - 1, 0) * C, rd = (int64_t)min(y + 1, R - 1) * C;
  auto at = [](const uint8_t *f, int64_t off) { return reinterpret_cast<const T *>(f) + off; };

  unsigned long long sum[5] = {0, 0, 0, 0, 0};  // S_c, S_p, A, B, C
  int mic = 0;                                  // mic_c | mic_p << 16
  for (int tx = blockIdx.y; tx < a.gx; tx += gridDim.y) {
    const int x0 = tx * FM_TILE_W + (wave * 4 + (lane & 3)) * FM_RUN;
    uint32_t sc = 0, sp = 0, sa = 0, sb = 0, s2 = 0;  // at most 16 x 65535 each
    int cnt = 0;                                      // cnt_c | cnt_p << 16, at most 16 each
    if (y < R && x0 < C) {
      const bool inside = x0 + FM_RUN <= C;
      uint32_t u[WORDS], m[WORDS], d[WORDS], e[WORDS], f[WORDS], g[WORDS], h[WORDS];
      fm_load<T>(at(cur, ru), x0, C, inside, u);
      fm_load<T>(at(cur, ry), x0, C, inside, m);
      fm_load<T>(at(cur, rd), x0, C, inside, d);
      // without an earlier frame its samples read as the current frame's: W_p = W_c and every difference is 0
#pragma unroll
      for (int w = 0; w < WORDS; ++w) e[w] = m[w], f[w] = u[w], g[w] = d[w], h[w] = m[w];
      if (p1) {
        fm_load<T>(at(p1, ry), x0, C, inside, e);
        if (same) {
          fm_load<T>(at(p1, ru), x0, C, inside, f);
          fm_load<T>(at(p1, rd), x0, C, inside, g);
        }
      }
      if (p2 && !same) fm_load<T>(at(p2, ry), x0, C, inside, h);
#pragma unroll
      for (int s = 0; s < FM_RUN; ++s) {
        const int cu = fm_get<T>(u, s), cm = fm_get<T>(m, s), cd = fm_get<T>(d, s), pm = fm_get<T>(e, s);
        // T1: W_p keeps the first field's rows and takes the others from the frame before
        const int kc = fm_comb(cu, cm, cd);
        const int kp = same ? fm_comb(fm_get<T>(f, s), cm, fm_get<T>(g, s)) : fm_comb(cu, pm, cd);
        const bool ok = inside || x0 + s < C;
        const bool comb = ok && interior;
        sc += comb ? (uint32_t)max(kc - a.nt, 0) : 0u;
        sp += comb ? (uint32_t)max(kp - a.nt, 0) : 0u;
        cnt += (comb && kc > a.ct ? 1 : 0) + (comb && kp > a.ct ? 1 << 16 : 0);
        const uint32_t ab = ok ? (uint32_t)abs(cm - pm) : 0u;
        sa += same ? ab : 0u;
        sb += same ? 0u : ab;
        s2 += ok && !same ? (uint32_t)abs(cm - fm_get<T>(h, s)) : 0u;
      }
    }
    // T4: the 16 lanes of a block column - lanes that differ in bits 2 ... 5 - hold one 16 x 16 block
#pragma unroll
    for (int b = 4; b < 64; b <<= 1) cnt += __shfl_xor(cnt, b, 64);
    mic = max(mic & 0xffff, cnt & 0xffff) | (max(mic >> 16, cnt >> 16) << 16);
    sum[0] += sc, sum[1] += sp, sum[2] += sa, sum[3] += sb, sum[4] += s2;
  }

  __shared__ unsigned long long wave_sum[4][5];
  __shared__ int wave_mic[4][2];
  int mc = mic & 0xffff, mp = mic >> 16;
#pragma unroll
  for (int b = 32; b > 0; b >>= 1) {
#pragma unroll
    for (int k = 0; k < 5; ++k) sum[k] += __shfl_down(sum[k], b, 64);
    mc = max(mc, __shfl_down(mc, b, 64)), mp = max(mp, __shfl_down(mp, b, 64));
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) wave_sum[wave][k] = sum[k];
    wave_mic[wave][0] = mc, wave_mic[wave][1] = mp;
  }
  __syncthreads();
  unsigned long long *row = a.table + (int64_t)i * FM_COLS;
  const int t = threadIdx.x;
  if (t < 5) {
    const unsigned long long s = wave_sum[0][t] + wave_sum[1][t] + wave_sum[2][t] + wave_sum[3][t];
    if (s) atomicAdd(row + (t < 2 ? t : t + 2), s);
  } else if (t < 7) {
    const int v = max(max(wave_mic[0][t - 5], wave_mic[1][t - 5]), max(wave_mic[2][t - 5], wave_mic[3][t - 5]));
    if (v) atomicMax(row + 2 + (t - 5), (unsigned long long)v);
  }
}

struct WeaveArgs {
  const uint8_t *yuv, *prev;      // the batch; frame -1 (dense) or null
  uint8_t *out;
  const int *table;               // per output frame: input frame index, match (0: c, 1: p)
  int64_t in_stride, out_stride;  // BYTES between frames
  int64_t cb_at, cr_at;           // BYTES from a frame's start to its chroma planes
  int n, q;
  int wb, wcb;                    // BYTES of a luma / chroma row
  int gwy, gwc, luma_items, chroma_items, items;  // 16-byte groups per luma / chroma row, lanes per luma plane / chroma plane / frame
};

constexpr int FW_RUN = 16;  // bytes of a lane

__global__ __launch_bounds__(256) void field_weave_kernel(const WeaveArgs a) {
  int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= a.items) return;
  int rb = a.wb, gw = a.gwy;
  int64_t plane = 0;
  if (t >= a.luma_items) {
    t -= a.luma_items;
    const int second = t >= a.chroma_items;
    if (second) t -= a.chroma_items;
    rb = a.wcb, gw = a.gwc;
    plane = second ? a.cr_at : a.cb_at;
  }
  const int y = t / gw, x0 = (t - y * gw) * FW_RUN;
  const int j = blockIdx.y;
  const int src = a.table[2 * j], match = a.table[2 * j + 1];
  if (src < 0 || src >= a.n) return;  // (the host never sends one)
  // T9: the first field's rows from frame src; the others from it too (c) or from the frame before (p)
  const uint8_t *from = a.yuv + (int64_t)src * a.in_stride;
  if (match && (y & 1) != a.q) from = src ? from - a.in_stride : a.prev;
  if (!from) return;
  const int64_t off = plane + (int64_t)y * rb + x0;
  const uint8_t *s = from + off;
  uint8_t *d = a.out + (int64_t)j * a.out_stride + off;
  if (x0 + FW_RUN <= rb) {
    uint32_t v[FW_RUN / 4];
    __builtin_memcpy(v, s, FW_RUN);
    __builtin_memcpy(d, v, FW_RUN);
  } else {
    for (int b = 0; x0 + b < rb; ++b) d[b] = s[b];
  }
}

static inline bool tc_even(const void *p) { return reinterpret_cast<uintptr_t>(p) % 2 == 0; }

static int tc_format(const char *what, int H, int W, int sub_x, int sub_y, int depth) {
  EDVR_REQUIRE(W >= 1, "%s: bad arguments", what);
  EDVR_REQUIRE(H >= 4, "%s: %d rows: a frame needs at least 4, so that every plane has 2", what, H);
  EDVR_REQUIRE(depth >= 8 && depth <= 16, "%s: a depth of %d bits is outside 8 ... 16", what, depth);
  EDVR_REQUIRE((sub_x == 1 && sub_y == 1) || (sub_x == 1 && sub_y == 0) || (sub_x == 0 && sub_y == 0),
               "%s: chroma subsampling (%d, %d) is none of 4:2:0 (1, 1), 4:2:2 (1, 0), 4:4:4 (0, 0)", what, sub_x, sub_y);
  EDVR_REQUIRE((int64_t)H * W <= INT32_MAX / 4, "%s: a %d x %d frame is too large", what, H, W);
  return EDVR_OK;
}

}  // namespace edvr

extern "C" int edvr_field_match(const uint8_t *yuv, const uint8_t *prev, const uint8_t *prev2, int64_t *table, int n, int H, int W, int sub_x,
                                int sub_y, int depth, int64_t in_stride, int bottom_first, int nt, int ct, edvr_stream_t stream) {
  using namespace edvr;
  const char *what = "field_match";
  EDVR_REQUIRE(yuv && table && n >= 1, "%s: bad arguments", what);
  if (const int rc = tc_format(what, H, W, sub_x, sub_y, depth)) return rc;
  EDVR_REQUIRE(bottom_first == 0 || bottom_first == 1, "%s: bottom_first is 0 or 1", what);
  EDVR_REQUIRE(nt >= 0 && nt <= 255 && ct >= 0 && ct <= 255, "%s: nt and ct are 8-bit levels, got %d and %d", what, nt, ct);
  EDVR_REQUIRE(n <= 32767, "%s: %d frames are too many for one launch", what, n);
  const int bps = depth > 8 ? 2 : 1, Hc = (H + sub_y) >> sub_y, Wc = (W + sub_x) >> sub_x;
  const int64_t framesize = ((int64_t)H * W + 2 * (int64_t)Hc * Wc) * bps;
  EDVR_REQUIRE(n == 1 || in_stride >= framesize, "%s: frames %lld bytes apart do not hold the %lld bytes of a %d x %d frame", what,
               (long long)in_stride, (long long)framesize, H, W);
  EDVR_REQUIRE(bps == 1 || (tc_even(yuv) && tc_even(prev) && tc_even(prev2) && (n == 1 || in_stride % 2 == 0)),
               "%s: 16-bit samples need even addresses and an even frame stride (%lld)", what, (long long)in_stride);
  hipStream_t s = as_stream(stream);
  const hipError_t e = hipMemsetAsync(table, 0, sizeof(int64_t) * FM_COLS * (size_t)n, s);
  if (e != hipSuccess) {
    set_error("%s: clearing the table: %s", what, hipGetErrorString(e));
    return EDVR_ERR_LAUNCH;
  }
  MatchArgs a;
  a.yuv = yuv, a.prev = prev, a.prev2 = prev2, a.table = reinterpret_cast<unsigned long long *>(table);
  a.in_stride = n == 1 ? 0 : in_stride;
  a.R = H, a.C = W, a.gx = cdiv(W, FM_TILE_W);
  a.q = bottom_first, a.nt = nt << (depth - 8), a.ct = ct << (depth - 8);
  const int gy = cdiv(H, FM_TILE_H);
  // enough workgroups to fill the chip, as few atomics as that allows: a strip of 16 rows is shared by at most gx workgroups
  const int64_t per = (int64_t)gy * n;
  const int split = (int)std::min<int64_t>(a.gx, std::max<int64_t>(1, FM_TARGET_WGS / per));
  const dim3 grid(gy, split, n), block(256);
  if (bps == 1) hipLaunchKernelGGL((field_match_kernel<uint8_t>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((field_match_kernel<uint16_t>), grid, block, 0, s, a);
  return check_launch("field_match_kernel");
}

extern "C" int edvr_field_weave(const uint8_t *yuv, const uint8_t *prev, uint8_t *out, const int32_t *table, int n, int n_out, int H, int W,
                                int sub_x, int sub_y, int depth, int64_t in_stride, int64_t out_stride, int bottom_first, edvr_stream_t stream) {
  using namespace edvr;
  const char *what = "field_weave";
  EDVR_REQUIRE(yuv && out && table && n >= 1 && n_out >= 1, "%s: bad arguments", what);
  if (const int rc = tc_format(what, H, W, sub_x, sub_y, depth)) return rc;
  EDVR_REQUIRE(bottom_first == 0 || bottom_first == 1, "%s: bottom_first is 0 or 1", what);
  EDVR_REQUIRE(n <= 32767 && n_out <= 32767, "%s: %d -> %d frames are too many for one launch", what, n, n_out);
  const int bps = depth > 8 ? 2 : 1, Hc = (H + sub_y) >> sub_y, Wc = (W + sub_x) >> sub_x;
  const int64_t framesize = ((int64_t)H * W + 2 * (int64_t)Hc * Wc) * bps;
  EDVR_REQUIRE(n == 1 || in_stride >= framesize, "%s: frames %lld bytes apart do not hold the %lld bytes of a %d x %d frame", what,
               (long long)in_stride, (long long)framesize, H, W);
  EDVR_REQUIRE(n_out == 1 || out_stride >= framesize, "%s: output frames %lld bytes apart do not hold the %lld bytes of a %d x %d frame", what,
               (long long)out_stride, (long long)framesize, H, W);
  WeaveArgs a;
  a.yuv = yuv, a.prev = prev, a.out = out, a.table = table;
  a.in_stride = n == 1 ? 0 : in_stride, a.out_stride = n_out == 1 ? 0 : out_stride;
  a.n = n, a.q = bottom_first;
  a.wb = W * bps, a.wcb = Wc * bps;
  a.cb_at = (int64_t)H * a.wb, a.cr_at = a.cb_at + (int64_t)Hc * a.wcb;
  a.gwy = cdiv(a.wb, FW_RUN), a.gwc = cdiv(a.wcb, FW_RUN);
  const int64_t items = (int64_t)H * a.gwy + 2 * (int64_t)Hc * a.gwc;
  EDVR_REQUIRE(items <= INT32_MAX - 256, "%s: a %d x %d frame is too large", what, H, W);
  a.luma_items = H * a.gwy, a.chroma_items = Hc * a.gwc, a.items = (int)items;
  const dim3 grid(cdiv(a.items, 256), n_out), block(256);
  hipLaunchKernelGGL(field_weave_kernel, grid, block, 0, as_stream(stream), a);
  return check_launch("field_weave_kernel");
}
