// lq_window.h - what the windowed forms of resize.hip and bd.hip share: the per-image record of edvr_*_u8_windows, the view of a source
// that is a window of its frame, and the host-side geometry of one axis (edvr_amd/data.py: lq_window states the same rule in Python).
//
// A training sample is a p x p crop of the LQ frame at a random (top, left).  Its source is not the GT frame but a window of it: the GT
// samples the crop's taps read with non-zero weight, AFTER the frame's boundary rule has folded out-of-frame taps back in.  The kernels
// compute weights from the ABSOLUTE output index (top + y, left + x), apply the boundary rule in FRAME coordinates and only then
// subtract the window's origin - so every output is the same chain of fmas on the same bytes as in the full-frame launch.  A tap of
// weight zero may fall outside the window: view_index clamps it into the window (its value is multiplied by 0.f).
#pragma once
#include <algorithm>
#include <cstdint>

#include "common.h"

namespace edvr {

// record of image i: table[8 * i + ...], int32
enum { LQW_Y0 = 0, LQW_X0 = 1, LQW_H = 2, LQW_W = 3, LQW_TOP = 4, LQW_LEFT = 5, LQW_REC = EDVR_LQ_WINDOW_RECORD_INTS };
enum { LQW_BI = 0, LQW_BD = 1 };

// index `i` of the frame (already folded by the boundary rule) -> index inside a view of `vn` samples that starts at frame sample `v0`
template <bool WIN>
__device__ __forceinline__ int view_index(int i, int v0, int vn) {
  return WIN ? min(max(i - v0, 0), vn - 1) : i;
}

// origin of a window read from the table: any int32 gives indices that stay inside the slot
__device__ __forceinline__ int window_origin(int v) { return min(max(v, 0), 1 << 28); }

// ---- host: one axis.  LQ sample i (0-based) of a frame of n GT samples reads, with non-zero weight, the unreflected GT samples
//   BI (imresize by 1 / s, antialiased): strictly inside (u - 2 s, u + 2 s), u = s (i + 1) + (1 - s) / 2, 1-based;
//   BD: i s - r .. i s + r, r = int(1.6 s + 0.5)
static inline int lqw_floor_div(int a, int b) { return a / b - (a % b != 0 && (a % b < 0) != (b < 0)); }
static inline int lqw_bd_radius(int s) { return (int)(1.6 * s + 0.5); }
static inline void lqw_taps(int kind, int s, int i, int *a, int *b) {
  if (kind == LQW_BI) {
    const int c = 2 * s * (i + 1) + 1;                          // 2 u + s
    *a = lqw_floor_div(c - 5 * s, 2);                           // 0-based first: floor(u - 2 s) + 1 - 1
    *b = -lqw_floor_div(-(c + 3 * s), 2) - 2;                   // 0-based last: ceil(u + 2 s) - 1 - 1
  } else {
    *a = i * s - lqw_bd_radius(s), *b = i * s + lqw_bd_radius(s);
  }
}
static inline int lqw_extent(int kind, int s, int size) {
  int a, b, a1, b1;
  lqw_taps(kind, s, 0, &a, &b), lqw_taps(kind, s, size - 1, &a1, &b1);
  return b1 - a + 1;
}
// [*lo, *hi] of the GT samples LQ samples [start, start + size) need; false where one reflection does not land inside the frame
static inline bool lqw_range(int kind, int s, int start, int size, int n, int *lo, int *hi) {
  int a, b, a1, b1;
  lqw_taps(kind, s, start, &a, &b1), lqw_taps(kind, s, start + size - 1, &a1, &b);
  const int ra = kind == LQW_BI ? -a - 1 : -a, rb = kind == LQW_BI ? 2 * n - 1 - b : 2 * (n - 1) - b;  // reflections of a < 0, b > n - 1
  if ((a < 0 && ra > n - 1) || (b > n - 1 && rb < 0)) return false;
  *lo = std::max(a, 0), *hi = std::min(b, n - 1);
  if (a < 0) *hi = std::max(*hi, ra);
  if (b > n - 1) *lo = std::min(*lo, rb);
  return true;
}
static inline bool lqw_scale_ok(int s) { return s >= 2 && s <= 4; }

// what the host can refuse without reading device memory, and - given a host copy of the table - every record
static inline const char *lqw_check(int kind, int s, int n, int p, int wh, int ww, int pitch, const void *src, const int32_t *table_host) {
  if (!lqw_scale_ok(s)) return "scale is not 2, 3 or 4";
  if (n <= 0 || n > 65535 || p <= 0 || p > 4096) return "bad image count or crop size";
  const int e = lqw_extent(kind, s, p);
  if (wh != e || ww != e) return "the window is not the extent lq_window gives for this crop size, scale and degradation";
  if (pitch % 16 != 0 || pitch < 3 * ww || reinterpret_cast<uintptr_t>(src) % 16 != 0) return "window rows do not start on 16-byte boundaries";
  if (table_host)
    for (int i = 0; i < n; ++i) {
      const int32_t *r = table_host + (size_t)LQW_REC * i;
      const int H = r[LQW_H], W = r[LQW_W];
      int lo, hi;
      if (H <= 0 || W <= 0 || H % s || W % s || H < wh || W < ww || H > (1 << 24) || W > (1 << 24)) return "a record's frame is not a multiple of the scale or is smaller than the window";
      if (r[LQW_TOP] < 0 || r[LQW_LEFT] < 0 || r[LQW_TOP] > H || r[LQW_LEFT] > W || (r[LQW_TOP] + p) * s > H || (r[LQW_LEFT] + p) * s > W)
        return "a record's crop leaves its frame";
      if (r[LQW_Y0] < 0 || r[LQW_X0] < 0 || r[LQW_Y0] > H - wh || r[LQW_X0] > W - ww) return "a record's window leaves its frame";
      if (!lqw_range(kind, s, r[LQW_TOP], p, H, &lo, &hi) || lo < r[LQW_Y0] || hi >= r[LQW_Y0] + wh ||
          !lqw_range(kind, s, r[LQW_LEFT], p, W, &lo, &hi) || lo < r[LQW_X0] || hi >= r[LQW_X0] + ww)
        return "a record's window does not hold what its crop reads";
    }
  return nullptr;
}

}  // namespace edvr
