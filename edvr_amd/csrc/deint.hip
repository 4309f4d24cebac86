// deint.hip - deinterlacing of interlaced Y4M frames on the device, on the byte planes, BEFORE colour conversion: every field of a woven
// clip becomes a full progressive frame ('field' rate: 2 n frames from n) or every first field does ('frame' rate: n frames), so that a
// 25i tape reaches VideoRestorer as the 50 pictures per second it really is.  Replaces nothing in the reference: it is the
// `ffmpeg -vf yadif` pass people otherwise run in front of the pipe, which quantises once more and usually drops half the fields.
//
// Definition (integers only; no bit-compatibility with any other deinterlacer is claimed).  A clip of n frames is
// the fields F_k, k = 0 ... 2 n - 1: field k lives in frame k >> 1 on the rows of parity q_k = (k + b) & 1, b = 0 top field first, 1 bottom
// field first.  Every plane (R rows, C columns) is treated alike.  S(k, r, x) = row fold_R(r), column clamp(x, 0, C - 1) of the frame
// that holds field fold_T(k); fold_R reflects into [0, R - 1] (repeatedly); fold_T reflects k about 0 and about 2 n - 1 - except on a
// side where a context frame is given (prev: fields -2, -1; next: fields 2 n, 2 n + 1), which is read instead.  Both keep the parity.
//   D1  rows of parity q_k: copied from frame k >> 1
//   D2  a missing row y: c = S(k, y - 1, x), e = S(k, y + 1, x), p = S(k - 1, y, x), nx = S(k + 1, y, x), dmid = (p + nx) >> 1
//   D3  t0 = |p - nx|, t1 = (|S(k - 2, y - 1, x) - c| + |S(k - 2, y + 1, x) - e|) >> 1, t2 likewise at k + 2, diff = max(t0 >> 1, t1, t2)
//   D4  j in (0, -1, +1, -2, +2): score(j) = sum over u in (-1, 0, 1) of |S(k, y - 1, x + j + u) - S(k, y + 1, x - j + u)| + (j != 0),
//       pred(j) = (S(k, y - 1, x + j) + S(k, y + 1, x - j)) >> 1; the j of least score, the first of equals in that order
//   D5  bb = (S(k - 1, y - 2, x) + S(k + 1, y - 2, x)) >> 1, ff likewise at y + 2; hi = max(dmid - e, dmid - c, min(bb - c, ff - e)),
//       lo = min(dmid - e, dmid - c, max(bb - c, ff - e)); diff = max(diff, lo, -hi)
//   D6  out = min(max(pred, dmid - diff), dmid + diff)      (between pred and dmid, hence a sample)
// The rule does not depend on the depth; sums of 16-bit samples are formed in 32 bits.
//
// Kernel shape: one launch for all output frames (blockIdx.y) and all three planes.  A lane owns 8 adjacent samples of one plane row.
// A kept row is a copy.  A missing row reads 12 row segments - the two rows of the current field with 3 samples of halo on either side
// (one 16-sample segment from 4 samples left of the lane's own) and ten of 8 samples - and writes one.  The frames behind the five field
// indices, the four folded row indices and the column range are resolved once per lane; the taps index registers.  A lane whose 16-sample
// window lies inside the row moves whole segments with accesses of any alignment (a Y4M buffer starts 6 bytes in and an odd width
// misaligns every other row: the planes are read where the decoder wrote them); the lanes at a row's ends, and every lane of a
// plane narrower than 16, load sample by sample with the column clamped and guard their stores.  The samples stay packed as loaded
// (4 bytes or 2 words per register) until a tap reads one.  No LDS, 0 bytes of scratch.
#include <cstdint>

#include "common.h"

namespace edvr {

struct DeintArgs {
  const uint8_t *yuv, *prev, *next;  // the batch; one dense frame before / after it or null
  uint8_t *out;
  int64_t in_stride, out_stride;  // BYTES between the frames of the batch / of the output
  int n, H, W, Hc, Wc;
  int gwy, gwc, luma_items, chroma_items, items;  // 8-sample groups per luma / chroma row, lanes per luma plane / chroma plane / frame
  int bottom_first, field_rate;
};

constexpr int DEINT_RUN = 8;  // samples of a lane

// the frame that holds field k, k in [-2, 2 n + 1]: at most two reflections (n = 1 without context), then a frame or a context frame
__device__ __forceinline__ const uint8_t *deint_frame(const DeintArgs &a, int k) {
  const int last = 2 * a.n - 1;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (k < 0 && !a.prev) k = -k;
    else if (k > last && !a.next) k = 2 * last - k;
  }
  const int f = k >> 1;
  return f < 0 ? a.prev : f >= a.n ? a.next : a.yuv + (int64_t)f * a.in_stride;
}

// r in [-2, R + 1] reflected into [0, R - 1], R >= 2: low, high, low covers R = 2 and R = 3, where one reflection overshoots
__device__ __forceinline__ int deint_fold(int r, int R) {
  if (r < 0) r = -r;
  if (r > R - 1) r = 2 * (R - 1) - r;
  if (r < 0) r = -r;
  return r;
}

// CNT samples row[x] ... row[x + CNT - 1], packed little-endian as memory holds them: whole accesses of any alignment where all of them
// lie inside the row, otherwise one by one with the column clamped to the row
template <typename T, int CNT>
__device__ __forceinline__ void deint_load(const T *__restrict__ row, int x, int C, bool inside, uint32_t (&q)[CNT * (int)sizeof(T) / 4]) {
  constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  if (inside) {
    __builtin_memcpy(q, row + x, CNT * sizeof(T));
  } else {
#pragma unroll
    for (int m = 0; m < CNT; ++m) {
      const uint32_t v = (uint32_t)row[min(max(x + m, 0), C - 1)] << (BITS * (m % PER));
      q[m / PER] = (m % PER) == 0 ? v : (q[m / PER] | v);
    }
  }
}

template <typename T>
__device__ __forceinline__ int deint_get(const uint32_t *q, int m) {
  constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
  return (int)((q[m / PER] >> (BITS * (m % PER))) & ((1u << BITS) - 1u));
}

// the lane's 8 samples to row[x] ...: one whole access, or one by one where the column exists
template <typename T>
__device__ __forceinline__ void deint_store(T *__restrict__ row, int x, int C, bool inside, const uint32_t (&q)[DEINT_RUN * (int)sizeof(T) / 4]) {
  if (inside) {
    __builtin_memcpy(row + x, q, DEINT_RUN * sizeof(T));
  } else {
#pragma unroll
    for (int m = 0; m < DEINT_RUN; ++m)
      if (x + m < C) row[x + m] = (T)deint_get<T>(q, m);
  }
}

__device__ __forceinline__ int deint_abs(int v) { return v < 0 ? -v : v; }

template <typename T>
__global__ __launch_bounds__(256) void deinterlace_kernel(const DeintArgs a) {
  constexpr int N = DEINT_RUN, WORDS = N * (int)sizeof(T) / 4;
  int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= a.items) return;
  // the plane, its row and the lane's columns
  int R = a.H, C = a.W, gw = a.gwy;
  int64_t plane = 0;  // samples from the frame's start
  if (t >= a.luma_items) {
    t -= a.luma_items;
    const int second = t >= a.chroma_items;
    if (second) t -= a.chroma_items;
    R = a.Hc, C = a.Wc, gw = a.gwc;
    plane = (int64_t)a.H * a.W + (int64_t)second * a.Hc * a.Wc;
  }
  const int y = t / gw, x0 = (t - y * gw) * N;
  const int j = blockIdx.y, k = a.field_rate ? j : 2 * j;
  const bool inside = x0 >= 4 && x0 + 12 <= C;  // the 16-sample window from x0 - 4 lies in the row
  T *orow = reinterpret_cast<T *>(a.out + (int64_t)j * a.out_stride) + plane + (int64_t)y * C;
  const uint8_t *f0 = a.yuv + (int64_t)(k >> 1) * a.in_stride;

  if ((y & 1) == ((k + a.bottom_first) & 1)) {  // D1
    uint32_t q[WORDS];
    deint_load<T, N>(reinterpret_cast<const T *>(f0) + plane + (int64_t)y * C, x0, C, inside, q);
    deint_store<T>(orow, x0, C, inside, q);
    return;
  }

  const uint8_t *fm1 = deint_frame(a, k - 1), *fp1 = deint_frame(a, k + 1), *fm2 = deint_frame(a, k - 2), *fp2 = deint_frame(a, k + 2);
  const int64_t ra = plane + (int64_t)deint_fold(y - 1, R) * C, rb = plane + (int64_t)deint_fold(y + 1, R) * C;
  const int64_t raa = plane + (int64_t)deint_fold(y - 2, R) * C, rbb = plane + (int64_t)deint_fold(y + 2, R) * C;
  const int64_t ry = plane + (int64_t)y * C;
  auto at = [](const uint8_t *f, int64_t off) { return reinterpret_cast<const T *>(f) + off; };

  uint32_t c[2 * WORDS], e[2 * WORDS];  // sample m: column x0 - 4 + m
  deint_load<T, 2 * N>(at(f0, ra), x0 - 4, C, inside, c);
  deint_load<T, 2 * N>(at(f0, rb), x0 - 4, C, inside, e);
  uint32_t p[WORDS], nx[WORDS], m2a[WORDS], m2b[WORDS], p2a[WORDS], p2b[WORDS], pbb[WORDS], nbb[WORDS], pff[WORDS], nff[WORDS];
  deint_load<T, N>(at(fm1, ry), x0, C, inside, p);
  deint_load<T, N>(at(fp1, ry), x0, C, inside, nx);
  deint_load<T, N>(at(fm2, ra), x0, C, inside, m2a);
  deint_load<T, N>(at(fm2, rb), x0, C, inside, m2b);
  deint_load<T, N>(at(fp2, ra), x0, C, inside, p2a);
  deint_load<T, N>(at(fp2, rb), x0, C, inside, p2b);
  deint_load<T, N>(at(fm1, raa), x0, C, inside, pbb);
  deint_load<T, N>(at(fp1, raa), x0, C, inside, nbb);
  deint_load<T, N>(at(fm1, rbb), x0, C, inside, pff);
  deint_load<T, N>(at(fp1, rbb), x0, C, inside, nff);

  uint32_t o[WORDS];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int cc = deint_get<T>(c, i + 4), ee = deint_get<T>(e, i + 4);
    const int pp = deint_get<T>(p, i), nn = deint_get<T>(nx, i);
    const int dmid = (pp + nn) >> 1;
    // D3
    const int t1 = (deint_abs(deint_get<T>(m2a, i) - cc) + deint_abs(deint_get<T>(m2b, i) - ee)) >> 1;
    const int t2 = (deint_abs(deint_get<T>(p2a, i) - cc) + deint_abs(deint_get<T>(p2b, i) - ee)) >> 1;
    int diff = max(max(deint_abs(pp - nn) >> 1, t1), t2);
    // D4: j = 0, then -1, +1, -2, +2; a later one wins only with a smaller score
    int best = 0, pred = (cc + ee) >> 1;
#pragma unroll
    for (int u = -1; u <= 1; ++u) best += deint_abs(deint_get<T>(c, i + 4 + u) - deint_get<T>(e, i + 4 + u));
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int d = (s & 1 ? 1 : -1) * (1 + (s >> 1));
      int score = 1;
#pragma unroll
      for (int u = -1; u <= 1; ++u) score += deint_abs(deint_get<T>(c, i + 4 + d + u) - deint_get<T>(e, i + 4 - d + u));
      if (score < best) best = score, pred = (deint_get<T>(c, i + 4 + d) + deint_get<T>(e, i + 4 - d)) >> 1;
    }
    // D5
    const int bb = (deint_get<T>(pbb, i) + deint_get<T>(nbb, i)) >> 1, ff = (deint_get<T>(pff, i) + deint_get<T>(nff, i)) >> 1;
    const int hi = max(max(dmid - ee, dmid - cc), min(bb - cc, ff - ee));
    const int lo = min(min(dmid - ee, dmid - cc), max(bb - cc, ff - ee));
    diff = max(max(diff, lo), -hi);
    // D6
    const uint32_t v = (uint32_t)min(max(pred, dmid - diff), dmid + diff);
    constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    o[i / PER] = (i % PER) == 0 ? v : (o[i / PER] | (v << (BITS * (i % PER))));
  }
  deint_store<T>(orow, x0, C, inside, o);
}

static inline bool deint_even(const void *p) { return reinterpret_cast<uintptr_t>(p) % 2 == 0; }

}  // namespace edvr

extern "C" int edvr_deinterlace(const uint8_t *yuv, const uint8_t *prev, const uint8_t *next, uint8_t *out, int n, int H, int W, int sub_x,
                                int sub_y, int depth, int64_t in_stride, int64_t out_stride, int bottom_first, int field_rate,
                                edvr_stream_t stream) {
  using namespace edvr;
  const char *what = "deinterlace";
  EDVR_REQUIRE(yuv && out && n >= 1 && W >= 1, "%s: bad arguments", what);
  EDVR_REQUIRE(H >= 4, "%s: %d rows: a frame needs at least 4, so that every plane has 2", what, H);
  EDVR_REQUIRE(depth >= 8 && depth <= 16, "%s: a depth of %d bits is outside 8 ... 16", what, depth);
  EDVR_REQUIRE((sub_x == 1 && sub_y == 1) || (sub_x == 1 && sub_y == 0) || (sub_x == 0 && sub_y == 0),
               "%s: chroma subsampling (%d, %d) is none of 4:2:0 (1, 1), 4:2:2 (1, 0), 4:4:4 (0, 0)", what, sub_x, sub_y);
  EDVR_REQUIRE((bottom_first == 0 || bottom_first == 1) && (field_rate == 0 || field_rate == 1), "%s: bottom_first and field_rate are 0 or 1", what);
  EDVR_REQUIRE((int64_t)H * W <= INT32_MAX / 4, "%s: a %d x %d frame is too large", what, H, W);
  EDVR_REQUIRE(n <= 32767, "%s: %d frames are too many for one launch", what, n);
  const int bps = depth > 8 ? 2 : 1, n_out = field_rate ? 2 * n : n;
  DeintArgs a;
  a.n = n, a.H = H, a.W = W, a.Hc = (H + sub_y) >> sub_y, a.Wc = (W + sub_x) >> sub_x;
  const int64_t framesize = ((int64_t)H * W + 2 * (int64_t)a.Hc * a.Wc) * bps;
  EDVR_REQUIRE(n == 1 || in_stride >= framesize, "%s: frames %lld bytes apart do not hold the %lld bytes of a %d x %d frame", what,
               (long long)in_stride, (long long)framesize, H, W);
  EDVR_REQUIRE(n_out == 1 || out_stride >= framesize, "%s: output frames %lld bytes apart do not hold the %lld bytes of a %d x %d frame", what,
               (long long)out_stride, (long long)framesize, H, W);
  EDVR_REQUIRE(bps == 1 || (deint_even(yuv) && deint_even(prev) && deint_even(next) && deint_even(out) && (n == 1 || in_stride % 2 == 0) &&
                            (n_out == 1 || out_stride % 2 == 0)),
               "%s: 16-bit samples need even addresses and even frame strides (%lld, %lld)", what, (long long)in_stride, (long long)out_stride);
  a.gwy = cdiv(W, DEINT_RUN), a.gwc = cdiv(a.Wc, DEINT_RUN);
  const int64_t items = (int64_t)H * a.gwy + 2 * (int64_t)a.Hc * a.gwc;
  EDVR_REQUIRE(items <= INT32_MAX - 256, "%s: a %d x %d frame is too large", what, H, W);
  a.luma_items = H * a.gwy, a.chroma_items = a.Hc * a.gwc, a.items = (int)items;
  a.yuv = yuv, a.prev = prev, a.next = next, a.out = out;
  a.in_stride = n == 1 ? 0 : in_stride, a.out_stride = n_out == 1 ? 0 : out_stride;
  a.bottom_first = bottom_first, a.field_rate = field_rate;
  const dim3 grid(cdiv(a.items, 256), n_out), block(256);
  if (bps == 1) hipLaunchKernelGGL((deinterlace_kernel<uint8_t>), grid, block, 0, as_stream(stream), a);
  else hipLaunchKernelGGL((deinterlace_kernel<uint16_t>), grid, block, 0, as_stream(stream), a);
  return check_launch("deinterlace_kernel");
}
