// bars.hip - letterbox / pillarbox bars on the device, on the byte planes, BEFORE colour conversion: the two kernels behind
// y4m.cropped / restore_y4m(crop=...).  A 2.35:1 film on a 16:9 disc is about 360 picture rows out of 480; the profile kernel measures
// how dark every row and column of every frame is, the host decides in integers (edvr_amd/bars.py) and the crop kernel copies the
// picture's rect of all three planes: everything behind it sees a smaller video.  Replaces nothing in the reference: it is the
// `ffmpeg -vf cropdetect,crop` pass people otherwise run in front of the pipe.
//
// Definition (integers only; no bit-compatibility with cropdetect is claimed).  L_i: the luma plane of frame i (R rows,
// C columns).
//   B1  P_i[y] = sum over x of L_i[y, x], Q_i[x] = sum over y of L_i[y, x]
// B2 - B6 (dark rows and columns, boxes, the aligned rect, belief) are host arithmetic on the table; B7 is the crop.
//
// bar_profile_kernel: one launch for all n frames (blockIdx.z), luma only, every sample read exactly once and reduced along both axes
// in that pass.  A lane owns 16 adjacent samples of one row; 16 lanes lie side by side - 256 columns - and a wave is 4 such rows, the
// four waves of a workgroup 16 rows: a tile of 16 rows x 256 columns.  The 16 lanes of a row add their row partials by four
// xor-shuffles and one of them adds the sum to P with ONE 64-bit integer atomic.  A workgroup keeps its column tile (blockIdx.x) and
// walks down the rows tile by tile (blockIdx.y of gridDim.y) with 16 column accumulators per lane; at the end the four rows of a wave
// fold by shuffles, the four waves through 4 KB of LDS, and every column of the tile gets ONE 64-bit atomic into Q.  u32 partials: a
// lane adds at most BP_MAX_STEPS samples of 16 bits to an accumulator and four lanes fold before the sums widen.  Whole 16-sample
// accesses of any alignment where the run lies inside the row, clamped single samples at its end.  Integer sums: the result does not
// depend on the batching or on the grid.  No float, 0 bytes of scratch.
//
// yuv_crop_kernel: one launch for all n frames (blockIdx.y), all three planes, row by row: a lane moves 16 BYTES of an output row
// (sample size does not matter to a copy) from a source row that starts at any byte offset - whole where they lie inside the row,
// byte by byte at its end.
#include <algorithm>
#include <cstdint>

#include "common.h"

namespace edvr {

constexpr int BP_RUN = 16;         // samples of a lane
constexpr int BP_TILE_W = 256;     // columns of a workgroup's tile: 16 lanes x 16 samples
constexpr int BP_TILE_H = 16;      // rows of a tile: 4 waves x 4 rows
constexpr int BP_MAX_STEPS = 4096; // tiles a workgroup walks at most: 4 lanes x 4096 x 65535 < 2^32
constexpr int BP_TARGET_WGS = 1024;

struct ProfileArgs {
  const uint8_t *yuv;         // the batch
  unsigned long long *table;  // (n, R + C), cleared before the launch: P then Q
  int64_t in_stride;          // BYTES between the frames of the batch
  int R, C, gy;               // luma rows, columns, row tiles
};

// 16 samples row[x] ... row[x + 15], packed little-endian as memory holds them: one access of any alignment where all lie inside the
// row, otherwise one by one with the column clamped to the row (as fm_load of telecine.hip)
template <typename T>
__device__ __forceinline__ void bp_load(const T *__restrict__ row, int x, int C, bool inside, uint32_t (&v)[BP_RUN * (int)sizeof(T) / 4]) {
  constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  if (inside) {
    __builtin_memcpy(v, row + x, BP_RUN * sizeof(T));
  } else {
#pragma unroll
    for (int m = 0; m < BP_RUN; ++m) {
      const uint32_t s = (uint32_t)row[min(x + m, C - 1)] << (BITS * (m % PER));
      v[m / PER] = (m % PER) == 0 ? s : (v[m / PER] | s);
    }
  }
}

template <typename T>
__device__ __forceinline__ uint32_t bp_get(const uint32_t *v, int m) {
  constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  return (v[m / PER] >> (BITS * (m % PER))) & ((1u << BITS) - 1u);
}

template <typename T>
__global__ __launch_bounds__(256) void bar_profile_kernel(const ProfileArgs a) {
  constexpr int WORDS = BP_RUN * (int)sizeof(T) / 4;
  const int i = blockIdx.z;
  const T *luma = reinterpret_cast<const T *>(a.yuv + (int64_t)i * a.in_stride);
  unsigned long long *P = a.table + (int64_t)i * ((int64_t)a.R + a.C), *Q = P + a.R;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int R = a.R, C = a.C;
  const int x0 = blockIdx.x * BP_TILE_W + (lane & 15) * BP_RUN;
  const bool inside = x0 + BP_RUN <= C;

  uint32_t col[BP_RUN];
#pragma unroll
  for (int m = 0; m < BP_RUN; ++m) col[m] = 0u;
  for (int ty = blockIdx.y; ty < a.gy; ty += gridDim.y) {
    const int y = ty * BP_TILE_H + wave * 4 + (lane >> 4);
    uint32_t rs = 0u;  // at most 16 x 65535, 256 x 65535 after the shuffles
    if (y < R && x0 < C) {
      uint32_t v[WORDS];
      bp_load<T>(luma + (int64_t)y * C, x0, C, inside, v);
#pragma unroll
      for (int m = 0; m < BP_RUN; ++m) {
        const uint32_t s = inside || x0 + m < C ? bp_get<T>(v, m) : 0u;
        col[m] += s;
        rs += s;
      }
    }
    // B1, rows: the 16 lanes of a row differ in bits 0 ... 3
#pragma unroll
    for (int b = 1; b < 16; b <<= 1) rs += __shfl_xor(rs, b, 64);
    if ((lane & 15) == 0 && y < R && rs) atomicAdd(P + y, (unsigned long long)rs);
  }

  // B1, columns: the 4 rows of a wave differ in bits 4 and 5, the waves meet in LDS
  __shared__ uint32_t part[4][BP_TILE_W];
#pragma unroll
  for (int m = 0; m < BP_RUN; ++m) {
    col[m] += __shfl_xor(col[m], 16, 64);
    col[m] += __shfl_xor(col[m], 32, 64);
  }
  if (lane < 16) {
#pragma unroll
    for (int m = 0; m < BP_RUN; ++m) part[wave][m * 16 + lane] = col[m];  // column lane * 16 + m of the tile, lanes on distinct banks
  }
  __syncthreads();
  const int t = threadIdx.x, x = blockIdx.x * BP_TILE_W + t;
  if (x < C) {
    const int at = (t & 15) * 16 + (t >> 4);
    const unsigned long long s = (unsigned long long)part[0][at] + part[1][at] + part[2][at] + part[3][at];
    if (s) atomicAdd(Q + x, s);
  }
}

struct CropArgs {
  const uint8_t *yuv;
  uint8_t *out;
  int64_t in_stride, out_stride;  // BYTES between frames
  int64_t src_at[3], dst_at[3];   // BYTES from a frame's start to the rect's first sample / to the output plane, per plane
  int in_wb[3], wb[3];            // BYTES of an input / output row, per plane
  int gw[3];                      // 16-byte groups per output row, per plane
  int luma_items, chroma_items, items;  // lanes per luma plane / chroma plane / frame
};

constexpr int YC_RUN = 16;  // bytes of a lane

__global__ __launch_bounds__(256) void yuv_crop_kernel(const CropArgs a) {
  int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= a.items) return;
  int p = 0;
  if (t >= a.luma_items) {
    t -= a.luma_items;
    p = t >= a.chroma_items ? 2 : 1;
    if (p == 2) t -= a.chroma_items;
  }
  // (selects, not indexed loads of the argument block: the three planes' numbers stay in scalar registers)
  const int gw = p == 0 ? a.gw[0] : (p == 1 ? a.gw[1] : a.gw[2]);
  const int wb = p == 0 ? a.wb[0] : (p == 1 ? a.wb[1] : a.wb[2]);
  const int in_wb = p == 0 ? a.in_wb[0] : (p == 1 ? a.in_wb[1] : a.in_wb[2]);
  const int64_t src_at = p == 0 ? a.src_at[0] : (p == 1 ? a.src_at[1] : a.src_at[2]);
  const int64_t dst_at = p == 0 ? a.dst_at[0] : (p == 1 ? a.dst_at[1] : a.dst_at[2]);
  const int y = t / gw, x0 = (t - y * gw) * YC_RUN;
  const int j = blockIdx.y;
  // B7: output row y of the plane is input row y0 + y from byte x0 sizeof(T) on
  const uint8_t *s = a.yuv + (int64_t)j * a.in_stride + src_at + (int64_t)y * in_wb + x0;
  uint8_t *d = a.out + (int64_t)j * a.out_stride + dst_at + (int64_t)y * wb + x0;
  if (x0 + YC_RUN <= wb) {
    uint32_t v[YC_RUN / 4];
    __builtin_memcpy(v, s, YC_RUN);
    __builtin_memcpy(d, v, YC_RUN);
  } else {
    for (int b = 0; x0 + b < wb; ++b) d[b] = s[b];
  }
}

static inline bool bars_even(const void *p) { return reinterpret_cast<uintptr_t>(p) % 2 == 0; }

static int bars_format(const char *what, int H, int W, int sub_x, int sub_y, int depth) {
  EDVR_REQUIRE(H >= 1 && W >= 1, "%s: a frame has at least one row and column, got %d x %d", what, H, W);
  EDVR_REQUIRE(depth >= 8 && depth <= 16, "%s: a depth of %d bits is outside 8 ... 16", what, depth);
  EDVR_REQUIRE((sub_x == 1 && sub_y == 1) || (sub_x == 1 && sub_y == 0) || (sub_x == 0 && sub_y == 0),
               "%s: chroma subsampling (%d, %d) is none of 4:2:0 (1, 1), 4:2:2 (1, 0), 4:4:4 (0, 0)", what, sub_x, sub_y);
  EDVR_REQUIRE((int64_t)H * W <= INT32_MAX / 4, "%s: a %d x %d frame is too large", what, H, W);
  return EDVR_OK;
}

}  // namespace edvr

extern "C" int edvr_bar_profile(const uint8_t *yuv, int64_t *table, int n, int H, int W, int sub_x, int sub_y, int depth, int64_t in_stride,
                                edvr_stream_t stream) {
  using namespace edvr;
  const char *what = "bar_profile";
  EDVR_REQUIRE(yuv && table && n >= 1, "%s: bad arguments", what);
  if (const int rc = bars_format(what, H, W, sub_x, sub_y, depth)) return rc;
  EDVR_REQUIRE(n <= 32767, "%s: %d frames are too many for one launch", what, n);
  const int bps = depth > 8 ? 2 : 1, Hc = (H + sub_y) >> sub_y, Wc = (W + sub_x) >> sub_x;
  const int64_t framesize = ((int64_t)H * W + 2 * (int64_t)Hc * Wc) * bps;
  EDVR_REQUIRE(n == 1 || in_stride >= framesize, "%s: frames %lld bytes apart do not hold the %lld bytes of a %d x %d frame", what,
               (long long)in_stride, (long long)framesize, H, W);
  EDVR_REQUIRE(bps == 1 || (bars_even(yuv) && (n == 1 || in_stride % 2 == 0)), "%s: 16-bit samples need an even address and an even frame stride (%lld)",
               what, (long long)in_stride);
  hipStream_t s = as_stream(stream);
  const hipError_t e = hipMemsetAsync(table, 0, sizeof(int64_t) * ((size_t)H + (size_t)W) * (size_t)n, s);
  if (e != hipSuccess) {
    set_error("%s: clearing the table: %s", what, hipGetErrorString(e));
    return EDVR_ERR_LAUNCH;
  }
  ProfileArgs a;
  a.yuv = yuv, a.table = reinterpret_cast<unsigned long long *>(table);
  a.in_stride = n == 1 ? 0 : in_stride;
  a.R = H, a.C = W, a.gy = cdiv(H, BP_TILE_H);
  const int gx = cdiv(W, BP_TILE_W);
  // every tile a workgroup of its own until the chip is full (one 480 x 720 frame is 90 tiles: all of them run at once); beyond that
  // a workgroup walks down several tiles of its columns, which saves the column atomics; never more than BP_MAX_STEPS (u32 partials)
  const int64_t per = (int64_t)gx * n;
  const int64_t want = std::max<int64_t>(1, BP_TARGET_WGS / per), least = cdiv(a.gy, BP_MAX_STEPS);
  const int split = (int)std::min<int64_t>(a.gy, std::max(want, least));
  const dim3 grid(gx, split, n), block(256);
  if (bps == 1) hipLaunchKernelGGL((bar_profile_kernel<uint8_t>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((bar_profile_kernel<uint16_t>), grid, block, 0, s, a);
  return check_launch("bar_profile_kernel");
}

extern "C" int edvr_yuv_crop(const uint8_t *yuv, uint8_t *out, int n, int H, int W, int sub_x, int sub_y, int depth, int64_t in_stride,
                             int64_t out_stride, int y0, int x0, int h, int w, edvr_stream_t stream) {
  using namespace edvr;
  const char *what = "yuv_crop";
  EDVR_REQUIRE(yuv && out && n >= 1, "%s: bad arguments", what);
  if (const int rc = bars_format(what, H, W, sub_x, sub_y, depth)) return rc;
  EDVR_REQUIRE(n <= 32767, "%s: %d frames are too many for one launch", what, n);
  EDVR_REQUIRE(y0 >= 0 && x0 >= 0 && h >= 1 && w >= 1 && h <= H - y0 && w <= W - x0, "%s: the rect (%d, %d, %d, %d) does not lie inside the %d x %d frame",
               what, y0, x0, h, w, H, W);
  const int my = (1 << sub_y) - 1, mx = (1 << sub_x) - 1;
  EDVR_REQUIRE(!((y0 | h) & my) && !((x0 | w) & mx), "%s: the rect (%d, %d, %d, %d) is off the chroma steps (%d, %d)", what, y0, x0, h, w, my + 1, mx + 1);
  const int bps = depth > 8 ? 2 : 1, Hc = (H + sub_y) >> sub_y, Wc = (W + sub_x) >> sub_x;
  const int hc = h >> sub_y, wc = w >> sub_x;  // (h + sub_y) >> sub_y: h is on the step
  const int64_t framesize = ((int64_t)H * W + 2 * (int64_t)Hc * Wc) * bps, outsize = ((int64_t)h * w + 2 * (int64_t)hc * wc) * bps;
  EDVR_REQUIRE(n == 1 || in_stride >= framesize, "%s: frames %lld bytes apart do not hold the %lld bytes of a %d x %d frame", what,
               (long long)in_stride, (long long)framesize, H, W);
  EDVR_REQUIRE(n == 1 || out_stride >= outsize, "%s: output frames %lld bytes apart do not hold the %lld bytes of a %d x %d frame", what,
               (long long)out_stride, (long long)outsize, h, w);
  CropArgs a;
  a.yuv = yuv, a.out = out;
  a.in_stride = n == 1 ? 0 : in_stride, a.out_stride = n == 1 ? 0 : out_stride;
  const int64_t in_cb = (int64_t)H * W * bps, in_cr = in_cb + (int64_t)Hc * Wc * bps;
  const int cy = y0 >> sub_y, cx = x0 >> sub_x;
  a.in_wb[0] = W * bps, a.in_wb[1] = a.in_wb[2] = Wc * bps;
  a.wb[0] = w * bps, a.wb[1] = a.wb[2] = wc * bps;
  a.src_at[0] = ((int64_t)y0 * W + x0) * bps;
  a.src_at[1] = in_cb + ((int64_t)cy * Wc + cx) * bps, a.src_at[2] = in_cr + ((int64_t)cy * Wc + cx) * bps;
  a.dst_at[0] = 0, a.dst_at[1] = (int64_t)h * w * bps, a.dst_at[2] = a.dst_at[1] + (int64_t)hc * wc * bps;
  for (int p = 0; p < 3; ++p) a.gw[p] = cdiv(a.wb[p], YC_RUN);
  const int64_t items = (int64_t)h * a.gw[0] + 2 * (int64_t)hc * a.gw[1];
  EDVR_REQUIRE(items <= INT32_MAX - 256, "%s: a %d x %d rect is too large", what, h, w);
  a.luma_items = h * a.gw[0], a.chroma_items = hc * a.gw[1], a.items = (int)items;
  const dim3 grid(cdiv(a.items, 256), n), block(256);
  hipLaunchKernelGGL(yuv_crop_kernel, grid, block, 0, as_stream(stream), a);
  return check_launch("yuv_crop_kernel");
}
