// ensemble.hip - self-ensemble (flip / D4 test-time augmentation) of the whole-video path (edvr_amd/video.py) for gfx950.  The video is
// restored under each symmetry of the square, the symmetry is undone and the results are averaged; a symmetry is the same shape of work
// as a tile - a different VIEW of the source on the way in, a different PLACE in the output on the way out:
//
//   edvr_crop_pad_frames_d4_*   the rectangle edvr_crop_pad_frames_* delivers, as the dense tile g_k(rectangle)
//   edvr_*_rect_d4_*            the four rectangle tails of video.hip storing g_k^-1(tile result), accumulating over the elements
//   edvr_*_rect_blend_*         the same four tails cross-fading neighbouring tiles over a band around each cut (BLEND below)
//
// Element k = 4 t + 2 v + h on the last two axes:  g_k(x) = x.transpose(-1, -2) if t; then .flip(-2) if v; then .flip(-1) if h.
// Both directions are ONE index map between a pixel (r, q) of the frame's orientation and (i, j) of the transformed (R, C) image:
//   (a, b) = t ? (q, r) : (r, q);   i = v ? R - 1 - a : a;   j = h ? C - 1 - b : b                        (frame_to_tile below)
// g_k(x)[i][j] = x[r][q] and g_k^-1(y)[r][q] = y[i][j] (flips are their own inverses, and they are applied in mirrored order).
//
// Non-transposing elements keep the four-pixels-per-thread shape of video.hip: reversed rows, reversed groups, reversed order inside a
// group.  Transposing elements go through a 32 x 32 LDS tile so that both the global reads and the global stores of a wave run along
// rows.  The tile's rows are padded to 33 dwords: the row-wise side writes [row][lane] (32 consecutive dwords: 32 banks), the
// column-wise side reads [lane][row] with ds_read_b32, whose bank is (address / 4) % 32 = (33 lane + row) % 32 = (lane + row) % 32 -
// distinct over the 32 lanes of each half wave, the group such a read is served in: conflict-free on both sides.
//
// The values are the very expressions of video.hip (`y + upsample_at<4>(base, ..)` on the tile's own, transformed y and base; to_u8 and
// div255 of pixel.h); the accumulation is written with __fadd_rn / __fmul_rn so that no add is contracted into a neighbour.
// Every destination pixel has one writer per launch and the launches of a chunk are ordered on the stream: no atomics.
#include <algorithm>

#include "common.h"
#include "pixel.h"

namespace edvr {
namespace d4 {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TS = 32;       // LDS tile edge of the transposing kernels
constexpr int TP = TS + 1;   // its padded row, in dwords

__device__ __forceinline__ int pad_index(int j, int n, int reflect) { return j < n ? j : (reflect ? 2 * (n - 1) - j : n - 1); }

// pixel (r, q) of the frame's orientation -> (i, j) of the transformed (R, C) image
__device__ __forceinline__ void frame_to_tile(int k, int r, int q, int R, int C, int &i, int &j) {
  const int a = (k & 4) ? q : r, b = (k & 4) ? r : q;
  i = (k & 2) ? R - 1 - a : a;
  j = (k & 1) ? C - 1 - b : b;
}

// ------------------------------------------------------------------------------------------------ oriented source read
struct CropArgs {
  const void *src;
  float *dst;
  int64_t src_img_stride;  // float source: floats between images (the uint8 source is dense)
  int n, H, W, y0, x0, th, tw, reflect;
  int src_vec;             // source groups of 4 pixels that lie inside the frame may be read by aligned wide loads
  int elem;
};

// t = 0.  VEC (tw % 4 == 0, dst 16-byte aligned): thread = 4 consecutive pixels of one DESTINATION row = a group of 4 source pixels of
// row (v ? th - 1 - r : r), the mirrored group read in reverse under h; generic: thread = one pixel.  U8: uint8 HWC source, one thread
// converts all three channels; else float CHW, thread = one plane's group.
template <bool U8, bool VEC>
__global__ __launch_bounds__(256) void crop_pad_frames_flip_kernel(const CropArgs a) {
  constexpr int P = VEC ? 4 : 1;
  const int hf = a.elem & 1, vf = a.elem & 2;
  const int wq = a.tw / P;
  const int64_t plane = (int64_t)a.th * a.tw, splane = (int64_t)a.H * a.W;
  const int64_t total = (int64_t)a.n * (U8 ? 1 : 3) * a.th * wq;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int g = (int)(idx % wq);
    const int r = (int)((idx / wq) % a.th);
    const int64_t pl = idx / ((int64_t)wq * a.th);  // U8: image; else image * 3 + channel
    const int sy = pad_index(a.y0 + (vf ? a.th - 1 - r : r), a.H, a.reflect);
    const int sx = a.x0 + (hf ? a.tw - P - P * g : P * g);  // first source pixel of the group (x0 and tw multiples of 4: alignment kept)
    if (U8) {
      const uint8_t *row = static_cast<const uint8_t *>(a.src) + (pl * a.H + sy) * (int64_t)a.W * 3;
      uint32_t px[P];  // px[i] = the three bytes of source pixel sx + i
      if (VEC && a.src_vec && sx + 3 < a.W) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(row + (int64_t)sx * 3);
        const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
        px[0] = w0 & 0xffffffu;
        if (VEC) px[1 % P] = (w0 >> 24) | ((w1 & 0xffffu) << 8), px[2 % P] = (w1 >> 16) | ((w2 & 0xffu) << 16), px[3 % P] = w2 >> 8;
      } else {
#pragma unroll
        for (int i = 0; i < P; ++i) {
          const uint8_t *p = row + (int64_t)pad_index(sx + i, a.W, a.reflect) * 3;
          px[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float *o = a.dst + (pl * 3 + c) * plane + (int64_t)r * a.tw + P * g;
        if (VEC) {
          f32x4 v;
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = div255(((hf ? px[(3 - i) % P] : px[i % P]) >> (8 * c)) & 0xffu);
          *reinterpret_cast<f32x4 *>(o) = v;
        } else {
          o[0] = div255((px[0] >> (8 * c)) & 0xffu);
        }
      }
    } else {
      const float *row = static_cast<const float *>(a.src) + (pl / 3) * a.src_img_stride + (pl % 3) * splane + (int64_t)sy * a.W;
      float *o = a.dst + pl * plane + (int64_t)r * a.tw + P * g;
      if (VEC) {
        f32x4 s, v;
        if (a.src_vec && sx + 3 < a.W) {
          s = *reinterpret_cast<const f32x4 *>(row + sx);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) s[i] = row[pad_index(sx + i, a.W, a.reflect)];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = hf ? s[3 - i] : s[i];
        *reinterpret_cast<f32x4 *>(o) = v;
      } else {
        o[0] = row[pad_index(sx, a.W, a.reflect)];
      }
    }
  }
}

// t = 1: grid (32 x 32 tiles of the source rectangle, images (U8) or planes).  Lane = threadIdx.x % 32, row group = threadIdx.x / 32
// (8 of them, 4 rows each).  Source side: lanes along a source row (contiguous pixels, pad_index per pixel) -> lds[row][lane].
// Destination side: destination (tw, th) pixel (i, j) = source (r, q) with i = v ? tw - 1 - q : q, j = h ? th - 1 - r : r - lanes along
// the source ROWS r (mirrored under h, so that j ascends with the lane): each wave stores two runs of 32 consecutive floats.
template <bool U8>
__global__ __launch_bounds__(256) void crop_pad_frames_transpose_kernel(const CropArgs a) {
  constexpr int CH = U8 ? 3 : 1;
  __shared__ float lds[CH][TS * TP];
  const int hf = a.elem & 1, vf = a.elem & 2;
  const int tiles_q = (a.tw + TS - 1) / TS;
  const int r0 = (int)(blockIdx.x / tiles_q) * TS, q0 = (int)(blockIdx.x % tiles_q) * TS;
  const int64_t pl = blockIdx.y;
  const int lane = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int64_t splane = (int64_t)a.H * a.W, plane = (int64_t)a.th * a.tw;
  {
    const int q = q0 + lane;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int rl = grp + 8 * p, r = r0 + rl;
      if (r < a.th && q < a.tw) {
        const int sy = pad_index(a.y0 + r, a.H, a.reflect), sx = pad_index(a.x0 + q, a.W, a.reflect);
        if (U8) {
          const uint8_t *px = static_cast<const uint8_t *>(a.src) + ((pl * a.H + sy) * (int64_t)a.W + sx) * 3;
#pragma unroll
          for (int c = 0; c < CH; ++c) lds[c][rl * TP + lane] = div255(px[c]);
        } else {
          lds[0][rl * TP + lane] = static_cast<const float *>(a.src)[(pl / 3) * a.src_img_stride + (pl % 3) * splane + (int64_t)sy * a.W + sx];
        }
      }
    }
  }
  __syncthreads();
  {
    const int rl = hf ? TS - 1 - lane : lane, r = r0 + rl;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int ql = grp + 8 * p, q = q0 + ql;
      if (r < a.th && q < a.tw) {
        const int i = vf ? a.tw - 1 - q : q, j = hf ? a.th - 1 - r : r;
#pragma unroll
        for (int c = 0; c < CH; ++c) a.dst[(pl * CH + c) * plane + (int64_t)i * a.th + j] = lds[c][rl * TP + ql];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ oriented, accumulating tails
constexpr int MODE_FIRST = 1, MODE_LAST = 2;  // EDVR_D4_FIRST, EDVR_D4_LAST

struct RectArgs {
  const float *y, *base;
  float *acc;
  uint8_t *dst;                                 // U8 tails: the bytes a LAST launch stores (never touched otherwise)
  int64_t y_img_stride, a_row, a_plane, a_img;  // accumulator strides in floats
  int64_t d_row, d_img;                         // byte destination strides
  int n, h, w, ky, kx, kh, kw;                  // (h, w): y's orientation (y is (n, 3, 4h, 4w) with UP); (ky, kx, kh, kw): the frame's
  int a_vec, d_vec;                             // 16-byte accesses to acc / three-dword stores to dst allowed
  int elem, mode;
  float scale;
  int by0, by1, bx0, bx1;                       // BLEND: low / high band lengths of the rectangle per axis, output pixels (0: no band)
};

// what a launch leaves for one pixel: first -> value; else acc + value; last -> that times scale
__device__ __forceinline__ float accumulate(float value, float acc, int mode, float scale) {
  const float s = (mode & MODE_FIRST) ? value : __fadd_rn(acc, value);
  return (mode & MODE_LAST) ? __fmul_rn(s, scale) : s;
}

// ---- BLEND (tile_blend of edvr_amd/video.py): the rectangle is a tile's EXTENDED rectangle, whose first by0 / bx0 and last by1 / bx1 rows
// / columns are bands it shares with the neighbouring tile on that side.  The j-th pixel of a band of B has weight r(j) = fl((2 j + 1) /
// (2 B)) (IEEE division) for the higher-index tile and fl(1 - r(j)) for the lower-index one, 1 outside the bands; w = fl(w_y * w_x).
// A pixel in a low band has an earlier contributor (this launch is not its first), one in a high band a later one (not its last).
__device__ __forceinline__ float axis_weight(int p, int len, int lo, int hi, bool &first, bool &last) {
  if (p < lo) {
    first = false;
    return (float)(2 * p + 1) / (float)(2 * lo);
  }
  if (p >= len - hi) {
    last = false;
    return 1.f - (float)(2 * (p - (len - hi)) + 1) / (float)(2 * hi);
  }
  return 1.f;
}

// first -> w * value; else acc + w * value; last -> that times scale.  The product is rounded on its own: the empty asm keeps
// -ffp-contract=fast from fusing it into the add (__fmul_rn is a plain `*` to the compiler).
__device__ __forceinline__ float accumulate_weighted(float value, float w, float acc, int mode, float scale) {
  float p = __fmul_rn(w, value);
  asm volatile("" : "+v"(p));
  return accumulate(p, acc, mode, scale);
}

// t = 0.  VEC (kx % 4 == 0, kw % 4 == 0, 16-byte aligned rows of y): thread = 4 consecutive pixels of a kept DESTINATION row = one
// 16-byte load of y per channel at the mirrored group, reversed under h.  BLEND + VEC: bx0 and bx1 are multiples of 4 as well, so that
// the four pixels of a group agree on first / last.
template <bool UP, bool U8, bool VEC, bool BLEND>
__global__ __launch_bounds__(256) void rect_flip_kernel(const RectArgs a) {
  constexpr int P = VEC ? 4 : 1;
  const int hy = UP ? 4 * a.h : a.h, wy = UP ? 4 * a.w : a.w;
  const int hf = a.elem & 1, vf = a.elem & 2;
  const int wq = a.kw / P;
  const int64_t total = (int64_t)a.n * a.kh * wq, yplane = (int64_t)hy * wy;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int q = (int)(idx % wq) * P;
    const int r = (int)((idx / wq) % a.kh);
    const int64_t img = idx / ((int64_t)wq * a.kh);
    int mode = a.mode;  // of this thread's pixels
    float wgt[P];
    if constexpr (BLEND) {
      bool first = true, last = true;
      const float wr = axis_weight(r, a.kh, a.by0, a.by1, first, last);
#pragma unroll
      for (int i = 0; i < P; ++i) wgt[i] = __fmul_rn(wr, axis_weight(q + i, a.kw, a.bx0, a.bx1, first, last));
      mode &= ~((first ? 0 : MODE_FIRST) | (last ? 0 : MODE_LAST));
    }
    const bool bytes = U8 && (mode & MODE_LAST);
    const int oy = vf ? hy - 1 - (a.ky + r) : a.ky + r;
    const int ox = hf ? wy - P - (a.kx + q) : a.kx + q;  // first y column of the group; destination pixel i <- column (hf ? ox + P - 1 - i : ox + i)
    float v[3][P];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float *yp = a.y + img * a.y_img_stride + c * yplane + (int64_t)oy * wy + ox;
      if (VEC) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(yp);
#pragma unroll
        for (int i = 0; i < P; ++i) v[c][i] = hf ? t[P - 1 - i] : t[i];
      } else {
        v[c][0] = yp[0];
      }
      if (UP) {
        const float *bp = a.base + (img * 3 + c) * (int64_t)a.h * a.w;
#pragma unroll
        for (int i = 0; i < P; ++i) v[c][i] = v[c][i] + upsample_at<4>(bp, a.h, a.w, oy, hf ? ox + P - 1 - i : ox + i);
      }
      float *ap = a.acc + img * a.a_img + c * a.a_plane + (int64_t)r * a.a_row + q;
      float old[P];
      if (!(mode & MODE_FIRST)) {
        if (VEC && a.a_vec) {
          const f32x4 t = *reinterpret_cast<const f32x4 *>(ap);
#pragma unroll
          for (int i = 0; i < P; ++i) old[i] = t[i];
        } else {
#pragma unroll
          for (int i = 0; i < P; ++i) old[i] = ap[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < P; ++i) old[i] = 0.f;
      }
#pragma unroll
      for (int i = 0; i < P; ++i) {
        if constexpr (BLEND) v[c][i] = accumulate_weighted(v[c][i], wgt[i], old[i], mode, a.scale);
        else v[c][i] = accumulate(v[c][i], old[i], mode, a.scale);
      }
      if (bytes) {
#pragma unroll
        for (int i = 0; i < P; ++i) v[c][i] = to_u8(v[c][i]);
      } else if (VEC && a.a_vec) {
        f32x4 t;
#pragma unroll
        for (int i = 0; i < P; ++i) t[i] = v[c][i];
        *reinterpret_cast<f32x4 *>(ap) = t;
      } else {
#pragma unroll
        for (int i = 0; i < P; ++i) ap[i] = v[c][i];
      }
    }
    if (bytes) {
      uint8_t *o = a.dst + img * a.d_img + (int64_t)r * a.d_row + (int64_t)q * 3;
      if constexpr (VEC) {
        store_px4(o, v, a.d_vec);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (uint8_t)(unsigned)v[c][0];
      }
    }
  }
}

// t = 1: grid (32 x 32 tiles of the kept rectangle, images).  Destination pixel (r, q) of the kept rectangle is (ky + r, kx + q) of the
// frame's orientation = y's (i, j) with i = v ? hy - 1 - (kx + q) : kx + q and j = h ? wy - 1 - (ky + r) : ky + r.  Value side: lanes
// along y's rows (the destination's r, mirrored under h so that j ascends with the lane) compute the value -> lds[q][r].  Accumulator
// side: lanes along the destination's rows read lds[q][r] column-wise and do the read-modify-write (or the byte store) there.
template <bool UP, bool U8, bool BLEND>
__global__ __launch_bounds__(256) void rect_transpose_kernel(const RectArgs a) {
  __shared__ float lds[3][TS * TP];
  const int hy = UP ? 4 * a.h : a.h, wy = UP ? 4 * a.w : a.w;
  const int hf = a.elem & 1, vf = a.elem & 2;
  const int tiles_q = (a.kw + TS - 1) / TS;
  const int r0 = (int)(blockIdx.x / tiles_q) * TS, q0 = (int)(blockIdx.x % tiles_q) * TS;
  const int64_t img = blockIdx.y, yplane = (int64_t)hy * wy;
  const int lane = threadIdx.x & 31, grp = threadIdx.x >> 5;
  {
    const int rl = hf ? TS - 1 - lane : lane, r = r0 + rl;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int ql = grp + 8 * p, q = q0 + ql;
      if (r < a.kh && q < a.kw) {
        int i, j;
        frame_to_tile(a.elem, a.ky + r, a.kx + q, hy, wy, i, j);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float val = a.y[img * a.y_img_stride + c * yplane + (int64_t)i * wy + j];
          if (UP) val = val + upsample_at<4>(a.base + (img * 3 + c) * (int64_t)a.h * a.w, a.h, a.w, i, j);
          lds[c][ql * TP + rl] = val;
        }
      }
    }
  }
  __syncthreads();
  {
    const int q = q0 + lane;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int rl = grp + 8 * p, r = r0 + rl;
      if (r < a.kh && q < a.kw) {
        int mode = a.mode;
        float wgt = 1.f;
        if constexpr (BLEND) {
          bool first = true, last = true;
          const float wr = axis_weight(r, a.kh, a.by0, a.by1, first, last);
          wgt = __fmul_rn(wr, axis_weight(q, a.kw, a.bx0, a.bx1, first, last));
          mode &= ~((first ? 0 : MODE_FIRST) | (last ? 0 : MODE_LAST));
        }
        const bool bytes = U8 && (mode & MODE_LAST);
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float *ap = a.acc + img * a.a_img + c * a.a_plane + (int64_t)r * a.a_row + q;
          const float old = (mode & MODE_FIRST) ? 0.f : ap[0];
          if constexpr (BLEND) v[c] = accumulate_weighted(lds[c][lane * TP + rl], wgt, old, mode, a.scale);
          else v[c] = accumulate(lds[c][lane * TP + rl], old, mode, a.scale);
          if (!bytes) ap[0] = v[c];
        }
        if (bytes) {
          uint8_t *o = a.dst + img * a.d_img + (int64_t)r * a.d_row + (int64_t)q * 3;
#pragma unroll
          for (int c = 0; c < 3; ++c) o[c] = (uint8_t)(unsigned)to_u8(v[c]);
        }
      }
    }
  }
}

static inline int grid_blocks(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>(cdiv64(n, 256), 1), 65536); }
static inline bool aligned_to(const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

static int crop_pad_launch(bool u8, const void *src, float *dst, int n, int H, int W, int64_t src_img_stride, int y0, int x0, int th, int tw,
                           int pad_mode, int elem, edvr_stream_t stream) {
  const char *name = u8 ? "crop_pad_frames_d4_u8" : "crop_pad_frames_d4_f32";
  EDVR_REQUIRE(src && dst && n > 0 && H > 0 && W > 0 && th > 0 && tw > 0 && y0 >= 0 && x0 >= 0 && y0 < H && x0 < W && elem >= 0 && elem < 8 &&
                   (pad_mode == EDVR_PAD_REFLECT || pad_mode == EDVR_PAD_REPLICATE) && (u8 || n == 1 || src_img_stride >= 3 * (int64_t)H * W),
               "%s: bad arguments", name);
  EDVR_REQUIRE(pad_mode != EDVR_PAD_REFLECT || (y0 + th - 1 <= 2 * (H - 1) && x0 + tw - 1 <= 2 * (W - 1)),
               "%s: a %d x %d rectangle at (%d, %d) reaches beyond the reflection of a %d x %d frame", name, th, tw, y0, x0, H, W);
  CropArgs a;
  a.src = src, a.dst = dst, a.src_img_stride = src_img_stride, a.n = n, a.H = H, a.W = W, a.y0 = y0, a.x0 = x0, a.th = th, a.tw = tw;
  a.reflect = pad_mode == EDVR_PAD_REFLECT, a.elem = elem;
  a.src_vec = W % 4 == 0 && x0 % 4 == 0 && (u8 ? aligned_to(src, 4) : (aligned_to(src, 16) && src_img_stride % 4 == 0));
  if (elem & 4) {
    const int64_t tiles = cdiv64(th, TS) * cdiv64(tw, TS), planes = (int64_t)n * (u8 ? 1 : 3);
    EDVR_REQUIRE(tiles <= 0x7fffffff && planes <= 65535, "%s: %lld tiles of %lld images / planes do not fit one grid", name, (long long)tiles,
                 (long long)planes);
    const dim3 grid((unsigned)tiles, (unsigned)planes);
    if (u8) hipLaunchKernelGGL(crop_pad_frames_transpose_kernel<true>, grid, dim3(256), 0, as_stream(stream), a);
    else hipLaunchKernelGGL(crop_pad_frames_transpose_kernel<false>, grid, dim3(256), 0, as_stream(stream), a);
    return check_launch(name);
  }
  const bool vec = tw % 4 == 0 && aligned_to(dst, 16);
  const dim3 grid(grid_blocks((int64_t)n * (u8 ? 1 : 3) * th * (vec ? tw / 4 : tw)));
  if (u8) {
    if (vec) hipLaunchKernelGGL((crop_pad_frames_flip_kernel<true, true>), grid, dim3(256), 0, as_stream(stream), a);
    else hipLaunchKernelGGL((crop_pad_frames_flip_kernel<true, false>), grid, dim3(256), 0, as_stream(stream), a);
  } else {
    if (vec) hipLaunchKernelGGL((crop_pad_frames_flip_kernel<false, true>), grid, dim3(256), 0, as_stream(stream), a);
    else hipLaunchKernelGGL((crop_pad_frames_flip_kernel<false, false>), grid, dim3(256), 0, as_stream(stream), a);
  }
  return check_launch(name);
}

struct Bands {
  int y0, y1, x0, x1;
};

template <bool UP, bool U8, bool BLEND = false>
static int rect_launch(const char *name, const float *y, const float *base, float *acc, uint8_t *dst, int n, int h, int w, int64_t y_img_stride,
                       int ky, int kx, int kh, int kw, int64_t a_row, int64_t a_plane, int64_t a_img, int64_t d_row, int64_t d_img, int elem, int mode,
                       float scale, edvr_stream_t stream, Bands bands = Bands{0, 0, 0, 0}) {
  const int hy = UP ? 4 * h : h, wy = UP ? 4 * w : w;
  EDVR_REQUIRE(elem >= 0 && elem < 8 && mode >= 0 && mode <= (MODE_FIRST | MODE_LAST), "%s: element %d, mode %d", name, elem, mode);
  const int fh = (elem & 4) ? wy : hy, fw = (elem & 4) ? hy : wy;  // the result in the frame's orientation
  const bool bytes = U8 && (mode & MODE_LAST);
  if (BLEND) {  // every band has the one width B, the bands of an axis do not meet
    const int B = std::max(std::max(bands.y0, bands.y1), std::max(bands.x0, bands.x1));
    const auto ok = [B](int v) { return v == 0 || v == B; };
    EDVR_REQUIRE(ok(bands.y0) && ok(bands.y1) && ok(bands.x0) && ok(bands.x1) && B >= 0 && (int64_t)bands.y0 + bands.y1 <= kh &&
                     (int64_t)bands.x0 + bands.x1 <= kw,
                 "%s: bands (%d, %d, %d, %d) of a %d x %d rectangle", name, bands.y0, bands.y1, bands.x0, bands.x1, kh, kw);
  }
  EDVR_REQUIRE(y && (base || !UP) && acc && (dst || !bytes) && n > 0 && h > 0 && w > 0 && ky >= 0 && kx >= 0 && kh > 0 && kw > 0 && ky + kh <= fh &&
                   kx + kw <= fw && (n == 1 || y_img_stride >= 3 * (int64_t)hy * wy) && a_row >= kw && a_plane >= (kh - 1) * a_row + kw &&
                   (n == 1 || a_img >= 2 * a_plane + (kh - 1) * a_row + kw) &&
                   (!bytes || (d_row >= 3 * (int64_t)kw && (n == 1 || d_img >= (kh - 1) * d_row + 3 * (int64_t)kw))),
               "%s: bad arguments", name);
  RectArgs a;
  a.y = y, a.base = base, a.acc = acc, a.dst = dst, a.y_img_stride = y_img_stride, a.a_row = a_row, a.a_plane = a_plane, a.a_img = a_img;
  a.d_row = d_row, a.d_img = d_img, a.n = n, a.h = h, a.w = w, a.ky = ky, a.kx = kx, a.kh = kh, a.kw = kw;
  a.elem = elem, a.mode = mode, a.scale = scale;
  a.by0 = bands.y0, a.by1 = bands.y1, a.bx0 = bands.x0, a.bx1 = bands.x1;
  a.a_vec = aligned_to(acc, 16) && a_row % 4 == 0 && a_plane % 4 == 0 && a_img % 4 == 0;
  a.d_vec = bytes && aligned_to(dst, 4) && d_row % 4 == 0 && d_img % 4 == 0;
  if (elem & 4) {
    const int64_t tiles = cdiv64(kh, TS) * cdiv64(kw, TS);
    EDVR_REQUIRE(tiles <= 0x7fffffff && n <= 65535, "%s: %lld tiles of %d images do not fit one grid", name, (long long)tiles, n);
    hipLaunchKernelGGL((rect_transpose_kernel<UP, U8, BLEND>), dim3((unsigned)tiles, (unsigned)n), dim3(256), 0, as_stream(stream), a);
    return check_launch(name);
  }
  const bool vec = kx % 4 == 0 && kw % 4 == 0 && wy % 4 == 0 && y_img_stride % 4 == 0 && aligned_to(y, 16) && bands.x0 % 4 == 0 && bands.x1 % 4 == 0;
  const dim3 grid(grid_blocks((int64_t)n * kh * (vec ? kw / 4 : kw)));
  if (vec) hipLaunchKernelGGL((rect_flip_kernel<UP, U8, true, BLEND>), grid, dim3(256), 0, as_stream(stream), a);
  else hipLaunchKernelGGL((rect_flip_kernel<UP, U8, false, BLEND>), grid, dim3(256), 0, as_stream(stream), a);
  return check_launch(name);
}

}  // namespace d4
}  // namespace edvr

extern "C" int edvr_crop_pad_frames_d4_u8(const uint8_t *src, float *dst, int n, int H, int W, int y0, int x0, int th, int tw, int pad_mode,
                                          int elem, edvr_stream_t stream) {
  return edvr::d4::crop_pad_launch(true, src, dst, n, H, W, 0, y0, x0, th, tw, pad_mode, elem, stream);
}

extern "C" int edvr_crop_pad_frames_d4_f32(const float *src, float *dst, int n, int H, int W, int64_t src_img_stride, int y0, int x0, int th,
                                           int tw, int pad_mode, int elem, edvr_stream_t stream) {
  return edvr::d4::crop_pad_launch(false, src, dst, n, H, W, src_img_stride, y0, x0, th, tw, pad_mode, elem, stream);
}

extern "C" int edvr_upsample4x_add_rect_d4_f32(const float *y, const float *base, float *acc, int n, int h, int w, int ky, int kx, int kh, int kw,
                                               int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride, int elem, int mode,
                                               float scale, edvr_stream_t stream) {
  return edvr::d4::rect_launch<true, false>("upsample4x_add_rect_d4_f32", y, base, acc, nullptr, n, h, w, 48 * (int64_t)h * w, ky, kx, kh, kw,
                                            acc_row_stride, acc_plane_stride, acc_img_stride, 0, 0, elem, mode, scale, stream);
}

extern "C" int edvr_upsample4x_add_rect_d4_u8(const float *y, const float *base, float *acc, uint8_t *dst, int n, int h, int w, int ky, int kx,
                                              int kh, int kw, int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride,
                                              int64_t dst_row_stride, int64_t dst_img_stride, int elem, int mode, float scale,
                                              edvr_stream_t stream) {
  return edvr::d4::rect_launch<true, true>("upsample4x_add_rect_d4_u8", y, base, acc, dst, n, h, w, 48 * (int64_t)h * w, ky, kx, kh, kw,
                                           acc_row_stride, acc_plane_stride, acc_img_stride, dst_row_stride, dst_img_stride, elem, mode, scale,
                                           stream);
}

extern "C" int edvr_f32_to_u8_hwc_rect_d4(const float *x, float *acc, uint8_t *dst, int n, int h, int w, int64_t x_img_stride, int ky, int kx,
                                          int kh, int kw, int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride,
                                          int64_t dst_row_stride, int64_t dst_img_stride, int elem, int mode, float scale, edvr_stream_t stream) {
  return edvr::d4::rect_launch<false, true>("f32_to_u8_hwc_rect_d4", x, nullptr, acc, dst, n, h, w, x_img_stride, ky, kx, kh, kw, acc_row_stride,
                                            acc_plane_stride, acc_img_stride, dst_row_stride, dst_img_stride, elem, mode, scale, stream);
}

extern "C" int edvr_copy_rect_d4_f32(const float *x, float *acc, int n, int h, int w, int64_t x_img_stride, int ky, int kx, int kh, int kw,
                                     int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride, int elem, int mode, float scale,
                                     edvr_stream_t stream) {
  return edvr::d4::rect_launch<false, false>("copy_rect_d4_f32", x, nullptr, acc, nullptr, n, h, w, x_img_stride, ky, kx, kh, kw, acc_row_stride,
                                             acc_plane_stride, acc_img_stride, 0, 0, elem, mode, scale, stream);
}

extern "C" int edvr_upsample4x_add_rect_blend_f32(const float *y, const float *base, float *acc, int n, int h, int w, int ky, int kx, int kh,
                                                  int kw, int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride, int elem,
                                                  int mode, float scale, int band_y_lo, int band_y_hi, int band_x_lo, int band_x_hi,
                                                  edvr_stream_t stream) {
  return edvr::d4::rect_launch<true, false, true>("upsample4x_add_rect_blend_f32", y, base, acc, nullptr, n, h, w, 48 * (int64_t)h * w, ky, kx, kh,
                                                  kw, acc_row_stride, acc_plane_stride, acc_img_stride, 0, 0, elem, mode, scale, stream,
                                                  edvr::d4::Bands{band_y_lo, band_y_hi, band_x_lo, band_x_hi});
}

extern "C" int edvr_upsample4x_add_rect_blend_u8(const float *y, const float *base, float *acc, uint8_t *dst, int n, int h, int w, int ky, int kx,
                                                 int kh, int kw, int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride,
                                                 int64_t dst_row_stride, int64_t dst_img_stride, int elem, int mode, float scale, int band_y_lo,
                                                 int band_y_hi, int band_x_lo, int band_x_hi, edvr_stream_t stream) {
  return edvr::d4::rect_launch<true, true, true>("upsample4x_add_rect_blend_u8", y, base, acc, dst, n, h, w, 48 * (int64_t)h * w, ky, kx, kh, kw,
                                                 acc_row_stride, acc_plane_stride, acc_img_stride, dst_row_stride, dst_img_stride, elem, mode,
                                                 scale, stream, edvr::d4::Bands{band_y_lo, band_y_hi, band_x_lo, band_x_hi});
}

extern "C" int edvr_f32_to_u8_hwc_rect_blend(const float *x, float *acc, uint8_t *dst, int n, int h, int w, int64_t x_img_stride, int ky, int kx,
                                             int kh, int kw, int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride,
                                             int64_t dst_row_stride, int64_t dst_img_stride, int elem, int mode, float scale, int band_y_lo,
                                             int band_y_hi, int band_x_lo, int band_x_hi, edvr_stream_t stream) {
  return edvr::d4::rect_launch<false, true, true>("f32_to_u8_hwc_rect_blend", x, nullptr, acc, dst, n, h, w, x_img_stride, ky, kx, kh, kw,
                                                  acc_row_stride, acc_plane_stride, acc_img_stride, dst_row_stride, dst_img_stride, elem, mode,
                                                  scale, stream, edvr::d4::Bands{band_y_lo, band_y_hi, band_x_lo, band_x_hi});
}

extern "C" int edvr_copy_rect_blend_f32(const float *x, float *acc, int n, int h, int w, int64_t x_img_stride, int ky, int kx, int kh, int kw,
                                        int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride, int elem, int mode, float scale,
                                        int band_y_lo, int band_y_hi, int band_x_lo, int band_x_hi, edvr_stream_t stream) {
  return edvr::d4::rect_launch<false, false, true>("copy_rect_blend_f32", x, nullptr, acc, nullptr, n, h, w, x_img_stride, ky, kx, kh, kw,
                                                   acc_row_stride, acc_plane_stride, acc_img_stride, 0, 0, elem, mode, scale, stream,
                                                   edvr::d4::Bands{band_y_lo, band_y_hi, band_x_lo, band_x_hi});
}
