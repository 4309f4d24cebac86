// conv_launch.h - host launch ladder shared by the two direct kernels (conv2d.hip: conv2d_mfma_kernel, conv2d_s.hip: conv2d_split_kernel).
// Both take <KS, STRIDE, MT, SW, NS> and an args struct with d / ho / wo / tiles_x / tiles_y / co_start.  K is a functor type with
//   template <int KS, int STRIDE, int MT, int SW, int NS> static int launch(dim3 grid, const Args &a, hipStream_t stream);
#pragma once
#include "common.h"

namespace edvr {

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

static inline bool use_sw16(int ho, int wo, int ns) {
  // pick the tile geometry (4ns x 32 or 8ns x 16) that wastes fewer lanes on this output size
  const int64_t w32 = (int64_t)cdiv(ho, 4 * ns) * 4 * ns * cdiv(wo, 32) * 32;
  const int64_t w16 = (int64_t)cdiv(ho, 8 * ns) * 8 * ns * cdiv(wo, 16) * 16;
  return w16 < w32;
}

template <class K, int KS, int STRIDE, int MT, int SW, class Args>
static int launch_one(const Args &a, int co_start, int co_blocks, hipStream_t stream) {
  constexpr int NS = MT >= 3 ? 1 : 2;
  constexpr int SH = 32 / SW, TH = 4 * NS * SH, TW = SW;
  Args b = a;
  b.tiles_x = cdiv(a.wo, TW);
  b.tiles_y = cdiv(a.ho, TH);
  b.co_start = co_start;
  return K::template launch<KS, STRIDE, MT, SW, NS>(dim3(b.tiles_x * b.tiles_y, co_blocks, a.d.n), b, stream);
}

template <class K, int KS, int STRIDE, int MT, class Args>
static int launch_sw(const Args &a, int co_start, int co_blocks, hipStream_t stream) {
  return use_sw16(a.ho, a.wo, MT >= 3 ? 1 : 2) ? launch_one<K, KS, STRIDE, MT, 16>(a, co_start, co_blocks, stream)
                                               : launch_one<K, KS, STRIDE, MT, 32>(a, co_start, co_blocks, stream);
}

template <class K, int KS, int STRIDE, class Args>
static int launch_mt(const Args &a, hipStream_t stream) {
  // full 128-channel blocks with MT = 4, then one exact-size tail launch (no masked MFMA work)
  const int full = a.d.co / 128, rem_tiles = cdiv(a.d.co - full * 128, 32);
  int rc = EDVR_OK;
  if (full > 0) rc = launch_sw<K, KS, STRIDE, 4>(a, 0, full, stream);
  if (rc || rem_tiles == 0) return rc;
  switch (rem_tiles) {
    case 1: return launch_sw<K, KS, STRIDE, 1>(a, full * 128, 1, stream);
    case 2: return launch_sw<K, KS, STRIDE, 2>(a, full * 128, 1, stream);
    case 3: return launch_sw<K, KS, STRIDE, 3>(a, full * 128, 1, stream);
    default: return launch_sw<K, KS, STRIDE, 4>(a, full * 128, 1, stream);  // 97..127 channels left
  }
}

// any KS / STRIDE the direct kernels are built for (callers have validated the pair)
template <class K, class Args>
static int launch_direct(const Args &a, hipStream_t stream) {
  if (a.d.ks == 3 && a.d.stride == 1) return launch_mt<K, 3, 1>(a, stream);
  if (a.d.ks == 3) return launch_mt<K, 3, 2>(a, stream);
  return launch_mt<K, 1, 1>(a, stream);
}

}  // namespace edvr
