// shots.hip - how much consecutive frames differ: the per-pair sum of absolute 8-bit luma differences a scene-cut detector thresholds
// (edvr_amd/shots.py; definition: DESIGN 4.13).  Integer-exact, so the number does not depend on how the frames were batched.
//
// Definition.  The bytes R, G, B of a pixel are the input's own (uint8 (n, H, W, 3)) or the tensor2img bytes to_u8 of pixel.h - clamp to
// [0, 1], x 255, round half to even, NaN -> 0 - of a float32 (n, 3, H, W) frame; in integers
//   Y8 = ((66 R + 129 G + 25 B + 128) >> 8) + 16          (16 ... 235)
//   sad[j] = sum over the H W pixels of |Y8 of frame j - Y8 of frame j - 1|,  j >= 1;   sad[0] likewise against `prev`, or 0 without one.
//
// Kernel shape: bytes in, one number per pair out.  grid = (blocks per frame, pairs): block (bx, j) walks the units bx, bx + gridDim.x, ...
// of pair j, a unit being 16 pixels (48 interleaved bytes: three 16-byte loads per frame) of the byte form and 4 pixels (one 16-byte load
// per plane and frame) of the float form.  The VEC instances need every frame of the call - the batch base, the image stride, `prev`, and
// for the float form the plane size H W - 16-byte aligned; the narrow instances load single bytes / floats and serve ANY base address and
// stride (a slice frames[1:] of 7 x 13 x 3-byte frames starts on an odd address).  Both guard the last, partial unit pixel by pixel: a
// pixel outside the frame is loaded from neither frame and contributes |0 - 0|.  Same values either way.
//
// Reduction: a thread sums its pixels in 32 bits (at most 2^31 / (1024 x 256) units of at most 16 x 219 each: < 2^25); everything that
// crosses threads is 64-bit - the wave's shuffles, the four wave sums in LDS and ONE global_atomic_add_x2 per block into sad[j], which the
// entry point clears on the same stream first.  Integer adds commute, so the order the blocks arrive in changes nothing, and the atomic
// spares the workspace, its size query and the second launch that block partials would need (n numbers leave: there is no contention
// to speak of - at most 1024 atomics per pair).  No float atomics, 64 bytes of LDS, 0 bytes of scratch.
#include <cstdint>

#include "common.h"
#include "pixel.h"

namespace edvr {

typedef uint32_t sad_u32x4 __attribute__((ext_vector_type(4)));
typedef float sad_f32x4 __attribute__((ext_vector_type(4)));

constexpr int SAD_THREADS = 256;
constexpr int SAD_MAX_BLOCKS = 1024;  // per frame pair

struct SadArgs {
  const void *x;         // frame j of the batch: x + j * img_stride elements
  const void *prev;      // the frame before frame 0, or null
  unsigned long long *sad;
  int64_t img_stride;    // elements (bytes / floats) between the frames of the batch
  int64_t P;             // H W
  int64_t units;         // ceil(P / pixels per unit)
  int first;             // pair of blockIdx.y == 0: 0 with prev, 1 without
};

__device__ __forceinline__ int sad_y8(int r, int g, int b) { return ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16; }

// the block's 256 32-bit sums -> one 64-bit atomic add
__device__ __forceinline__ void sad_block_add(uint32_t acc, unsigned long long *dst) {
  __shared__ unsigned long long wave_sum[SAD_THREADS / 64];
  unsigned long long v = acc;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_sum[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < SAD_THREADS / 64; ++k) s += wave_sum[k];
    atomicAdd(dst, s);
  }
}

// the 48 bytes of unit u (pixels 16 u ... 16 u + 15, interleaved) as twelve little-endian dwords; bytes of pixels >= P read as 0
template <bool VEC>
__device__ __forceinline__ void sad_load48(const uint8_t *__restrict__ f, int64_t u, int64_t P, uint32_t (&q)[12]) {
  const int64_t b0 = 48 * u;
  if (VEC && 16 * u + 16 <= P) {
    const sad_u32x4 *p = reinterpret_cast<const sad_u32x4 *>(f + b0);
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const sad_u32x4 w = p[s];
      q[4 * s] = w[0], q[4 * s + 1] = w[1], q[4 * s + 2] = w[2], q[4 * s + 3] = w[3];
    }
  } else {
    const int64_t end = 3 * P;
#pragma unroll
    for (int d = 0; d < 12; ++d) {
      q[d] = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t b = b0 + 4 * d + e;
        if (b < end) q[d] |= (uint32_t)f[b] << (8 * e);
      }
    }
  }
}

__device__ __forceinline__ int sad_byte(const uint32_t (&q)[12], int b) { return (int)((q[b >> 2] >> (8 * (b & 3))) & 0xffu); }

template <bool VEC>
__global__ __launch_bounds__(SAD_THREADS) void frame_sad_u8_kernel(const SadArgs a) {
  const int j = a.first + blockIdx.y;
  const uint8_t *x = static_cast<const uint8_t *>(a.x);
  const uint8_t *cur = x + (int64_t)j * a.img_stride;
  const uint8_t *prv = j == 0 ? static_cast<const uint8_t *>(a.prev) : x + (int64_t)(j - 1) * a.img_stride;
  uint32_t acc = 0;
  for (int64_t u = (int64_t)blockIdx.x * SAD_THREADS + threadIdx.x; u < a.units; u += (int64_t)gridDim.x * SAD_THREADS) {
    uint32_t qc[12], qp[12];
    sad_load48<VEC>(cur, u, a.P, qc);
    sad_load48<VEC>(prv, u, a.P, qp);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int yc = sad_y8(sad_byte(qc, 3 * i), sad_byte(qc, 3 * i + 1), sad_byte(qc, 3 * i + 2));
      const int yp = sad_y8(sad_byte(qp, 3 * i), sad_byte(qp, 3 * i + 1), sad_byte(qp, 3 * i + 2));
      acc += (uint32_t)abs(yc - yp);
    }
  }
  sad_block_add(acc, a.sad + j);
}

// channel c of pixels 4 u ... 4 u + 3 of a planar (3, P) frame as tensor2img bytes; pixels >= P read as 0
template <bool VEC>
__device__ __forceinline__ void sad_load4(const float *__restrict__ plane, int64_t u, int64_t P, int (&v)[4]) {
  if (VEC) {  // (P % 4 == 0: every unit is whole)
    const sad_f32x4 w = *reinterpret_cast<const sad_f32x4 *>(plane + 4 * u);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (int)to_u8(w[i]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = 4 * u + i < P ? (int)to_u8(plane[4 * u + i]) : 0;
  }
}

template <bool VEC>
__global__ __launch_bounds__(SAD_THREADS) void frame_sad_f32_kernel(const SadArgs a) {
  const int j = a.first + blockIdx.y;
  const float *x = static_cast<const float *>(a.x);
  const float *cur = x + (int64_t)j * a.img_stride;
  const float *prv = j == 0 ? static_cast<const float *>(a.prev) : x + (int64_t)(j - 1) * a.img_stride;
  uint32_t acc = 0;
  for (int64_t u = (int64_t)blockIdx.x * SAD_THREADS + threadIdx.x; u < a.units; u += (int64_t)gridDim.x * SAD_THREADS) {
    int c[3][4], p[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      sad_load4<VEC>(cur + k * a.P, u, a.P, c[k]);
      sad_load4<VEC>(prv + k * a.P, u, a.P, p[k]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) acc += (uint32_t)abs(sad_y8(c[0][i], c[1][i], c[2][i]) - sad_y8(p[0][i], p[1][i], p[2][i]));
  }
  sad_block_add(acc, a.sad + j);
}

static inline bool sad_aligned(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

template <bool U8>
static int frame_sad(const void *x, const void *prev, uint64_t *sad, int n, int H, int W, int64_t img_stride, edvr_stream_t stream) {
  const char *what = U8 ? "frame_sad_rgb_u8" : "frame_sad_rgb_f32";
  EDVR_REQUIRE(x && sad && n > 0 && H > 0 && W > 0, "%s: bad arguments", what);
  const int64_t P = (int64_t)H * W;
  EDVR_REQUIRE(P <= INT32_MAX, "%s: a %d x %d frame is too large", what, H, W);
  if (img_stride == 0) img_stride = 3 * P;
  EDVR_REQUIRE(n == 1 || img_stride >= 3 * P, "%s: frames %lld elements apart overlap", what, (long long)img_stride);
  hipStream_t s = as_stream(stream);
  const hipError_t e = hipMemsetAsync(sad, 0, sizeof(uint64_t) * (size_t)n, s);
  if (e != hipSuccess) {
    set_error("%s: clearing the result: %s", what, hipGetErrorString(e));
    return EDVR_ERR_LAUNCH;
  }
  SadArgs a;
  a.x = x, a.prev = prev, a.sad = reinterpret_cast<unsigned long long *>(sad), a.img_stride = img_stride, a.P = P;
  a.first = prev ? 0 : 1;
  const int pairs = n - a.first;
  if (pairs == 0) return EDVR_OK;  // one frame and nothing before it: sad[0] = 0
  const int px = U8 ? 16 : 4;
  a.units = (P + px - 1) / px;
  const int64_t elem = U8 ? 1 : 4;
  const bool vec = sad_aligned(x) && (!prev || sad_aligned(prev)) && (n == 1 || img_stride * elem % 16 == 0) && (U8 || P % 4 == 0);
  const int64_t want = (a.units + SAD_THREADS - 1) / SAD_THREADS;
  const dim3 grid((unsigned)(want < SAD_MAX_BLOCKS ? want : SAD_MAX_BLOCKS), (unsigned)pairs), block(SAD_THREADS);
  if (U8) {
    if (vec) hipLaunchKernelGGL((frame_sad_u8_kernel<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((frame_sad_u8_kernel<false>), grid, block, 0, s, a);
  } else {
    if (vec) hipLaunchKernelGGL((frame_sad_f32_kernel<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((frame_sad_f32_kernel<false>), grid, block, 0, s, a);
  }
  return check_launch(U8 ? "frame_sad_u8_kernel" : "frame_sad_f32_kernel");
}

}  // namespace edvr

extern "C" int edvr_frame_sad_rgb_u8(const uint8_t *x, const uint8_t *prev, uint64_t *sad, int n, int H, int W, int64_t img_stride,
                                     edvr_stream_t stream) {
  return edvr::frame_sad<true>(x, prev, sad, n, H, W, img_stride, stream);
}

extern "C" int edvr_frame_sad_rgb_f32(const float *x, const float *prev, uint64_t *sad, int n, int H, int W, int64_t img_stride,
                                      edvr_stream_t stream) {
  return edvr::frame_sad<false>(x, prev, sad, n, H, W, img_stride, stream);
}
