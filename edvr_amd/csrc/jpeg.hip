// jpeg.hip - the baseline JPEG round trip on the device: what an 8-bit RGB frame looks like after a JPEG encoder and decoder, i.e. block-DCT
// compression artifacts for LQ frames and training crops.  Definition: DESIGN 4.16 - libjpeg's integer pipeline end to end (colour
// conversion, edge padding, 4:2:0 chroma by the alternating-bias 2 x 2 mean, the 13-bit Loeffler DCT both ways, Annex K tables scaled by
// the quality, triangle-filter chroma upsampling).  Entropy coding is lossless and is not performed.  All arithmetic is 32-bit integer:
// there is no evaluation order to preserve, and the result is the bytes PIL's libjpeg returns (tests/golden/jpeg_roundtrip.pt).
//
// ONE launch, grid (tiles, n), no workspace.  A workgroup of 256 lanes owns a 64 x 64 pixel tile of one image - whole MCUs of either
// subsampling - and keeps its planes in LDS as 32-bit integers:
//   0. the two quantisation tables of the image's quality, Q and the reciprocal M = floor(2^32 / 8Q) + 1, in LDS (one division per entry
//      and workgroup: k = (|c| + 4Q) / 8Q is then umulhi(|c| + 4Q, M), exact below 2^21);
//   1. load: a lane reads 4 pixels of a row (three dwords where rows are 4-byte aligned) - for '420' of a row PAIR, i.e. two chroma cells -
//      converts and writes Y, Cb, Cr.  '420' also covers the ring of one 8 x 8 chroma block around the tile's 4 x 4, which the triangle
//      filter of the upsampling reaches by one sample: 36 chroma blocks per plane instead of 16, from a 96 x 96 pixel window; blocks off
//      the frame are skipped, so the frame's edge - and a 64 x 64 training crop, which is all edge - pays nothing;
//   2. forward DCT rows: one row of one block per lane, in place;
//   3. forward DCT columns, quantisation, dequantisation and the inverse DCT's columns: one column of one block per lane, in place (the
//      inverse transform runs columns first, so the three steps need no exchange between them);
//   4. inverse DCT rows, + 128, clamp: one row per lane;
//   5. store: a lane upsamples the chroma of 4 pixels ('420'), converts back and writes 12 bytes.
// "Transposing" between 2, 3 and 4 is the change of which lane reads what: plane rows are 68 ('420' chroma: 52) words apart, = 4 and 20
// modulo the 32 banks, so the 8 lanes of a block's row pass (16-byte reads 4 r or 20 r banks apart: 8 distinct groups of 4) and of its
// column pass (consecutive words) never share a bank.
// Every product of the transforms has factors below 2^23 in magnitude, so they are 24-bit multiplies (v_mul_i32_i24).
#include "jpeg_dct.h"

namespace edvr {

struct JpegArgs {
  const uint8_t *src;
  uint8_t *dst;
  const int32_t *quality;  // per image, or null
  int quality_all;
  int H, W;
  int64_t src_stride, dst_stride;  // bytes between images
  int src_vec, dst_vec;            // every pixel quad of a row starts on a 4-byte boundary
};

constexpr int JT = 64;         // tile side, pixels
constexpr int JYS = JT + 4;    // words of a full-resolution plane row
constexpr int JCN = 48;        // '420': chroma samples per side of the tile's window (32 + the ring of 8 either side)
constexpr int JCS = JCN + 4;   // words of such a chroma row

__device__ __constant__ uint8_t jpeg_base[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

template <bool S420>
__global__ __launch_bounds__(256) void jpeg_roundtrip_kernel(const JpegArgs a) {
  constexpr int NPL = S420 ? JT * JYS + 2 * JCN * JCS : 3 * JT * JYS;
  constexpr int NBLK = S420 ? 64 + 2 * 36 : 3 * 64;
  __shared__ __attribute__((aligned(16))) int pl[NPL];  // Y [64][68], then '420': Cb, Cr [48][52] / '444': Cb, Cr [64][68]
  __shared__ int qt[2][64];                             // Q of luminance, chrominance
  __shared__ uint32_t qm[2][64];                        // floor(2^32 / 8Q) + 1
  const int tid = threadIdx.x, img = blockIdx.y;
  const int H = a.H, W = a.W;
  const int tiles_x = (W + JT - 1) / JT;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * JT, x0 = tx * JT;
  const int64_t pitch = 3 * (int64_t)W;
  const uint8_t *src = a.src + img * a.src_stride;
  uint8_t *dst = a.dst + img * a.dst_stride;
  const int q = a.quality ? min(max(a.quality[img], 0), 100) : a.quality_all;

  if (q == 0) {  // (uniform over the workgroup) the image passes through unchanged
    for (int item = tid; item < JT * (JT / 4); item += 256) {
      const int row = item >> 4, py = y0 + row, px = x0 + 4 * (item & 15);
      if (py >= H || px >= W) continue;
      int r[4], g[4], b[4];
      jpeg_load4(src + py * pitch, px, W, a.src_vec, r, g, b);
      const uint32_t v[4] = {(uint32_t)(r[0] | g[0] << 8 | b[0] << 16), (uint32_t)(r[1] | g[1] << 8 | b[1] << 16),
                             (uint32_t)(r[2] | g[2] << 8 | b[2] << 16), (uint32_t)(r[3] | g[3] << 8 | b[3] << 16)};
      jpeg_store4(dst + py * pitch, px, W, a.dst_vec, v);
    }
    return;
  }

  // ---- 0. quantisation tables
  if (tid < 128) {
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    const int Q = min(max(((int)jpeg_base[tid >> 6][tid & 63] * s + 50) / 100, 1), 255);
    qt[tid >> 6][tid & 63] = Q;
    qm[tid >> 6][tid & 63] = (uint32_t)(0x100000000ull / (uint32_t)(8 * Q)) + 1u;
  }

  int *const yp = pl;
  const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;  // the real chroma plane ('420')
  const int cy0 = (y0 >> 1) - 8, cx0 = (x0 >> 1) - 8;  // chroma sample at [0][0] of the '420' chroma window

  // ---- 1. load and convert
  if constexpr (S420) {
    int *const cbp = pl + JT * JYS, *const crp = cbp + JCN * JCS;
    for (int item = tid; item < JCN * (JCN / 2); item += 256) {
      const int cr_ = item / (JCN / 2), g_ = item - cr_ * (JCN / 2);
      const int cyA = cy0 + cr_, cxA = cx0 + 2 * g_;  // chroma row, and the first of two chroma columns (even)
      // a sample is wanted where its 8 x 8 block holds a real chroma sample
      if (cyA < 0 || cxA < 0 || (cyA & ~7) >= ch || (cxA & ~7) >= cw) continue;
      const int cyc = min(cyA, ch - 1);  // below the frame the encoder repeats the last chroma row ...
      const int ra = 2 * cyc, rb = min(2 * cyc + 1, H - 1);
      int r[2][4], g[2][4], b[2][4];
      jpeg_load4(src + ra * pitch, 2 * cxA, W, a.src_vec, r[0], g[0], b[0]);
      jpeg_load4(src + rb * pitch, 2 * cxA, W, a.src_vec, r[1], g[1], b[1]);
      int scb[2] = {1, 2}, scr[2] = {1, 2};  // the bias: 1 in even chroma columns, 2 in odd ones
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) scb[i >> 1] += jpeg_cb(r[j][i], g[j][i], b[j][i]), scr[i >> 1] += jpeg_cr(r[j][i], g[j][i], b[j][i]);
      cbp[cr_ * JCS + 2 * g_] = scb[0] >> 2, cbp[cr_ * JCS + 2 * g_ + 1] = scb[1] >> 2;
      crp[cr_ * JCS + 2 * g_] = scr[0] >> 2, crp[cr_ * JCS + 2 * g_ + 1] = scr[1] >> 2;
      if (cr_ >= 8 && cr_ < 40 && g_ >= 4 && g_ < 20) {  // inside the tile: luma, ... which repeats the last ROW (rb = H - 1 there)
        const int j0 = cyA > ch - 1 ? 1 : 0;
        int *o = yp + 2 * (cr_ - 8) * JYS + 4 * (g_ - 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = jpeg_y(r[j0][i], g[j0][i], b[j0][i]), o[JYS + i] = jpeg_y(r[1][i], g[1][i], b[1][i]);
      }
    }
  } else {
    for (int item = tid; item < JT * (JT / 4); item += 256) {
      const int row = item >> 4, col = 4 * (item & 15);
      if (((y0 + row) & ~7) >= H || x0 + (col & ~7) >= W) continue;
      int r[4], g[4], b[4];
      jpeg_load4(src + min(y0 + row, H - 1) * pitch, x0 + col, W, a.src_vec, r, g, b);
      int *o = yp + row * JYS + col;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        o[i] = jpeg_y(r[i], g[i], b[i]), o[JT * JYS + i] = jpeg_cb(r[i], g[i], b[i]), o[2 * JT * JYS + i] = jpeg_cr(r[i], g[i], b[i]);
    }
  }
  __syncthreads();

  // block `blk` of the workgroup: where it starts, its row stride, its table; false where no real sample lies in it
  auto block_at = [&](int blk, int *&p, int &stride, int &tbl) -> bool {
    if (!S420 || blk < 64) {
      const int plane = blk >> 6, by = (blk >> 3) & 7, bx = blk & 7;
      p = pl + plane * JT * JYS + 8 * by * JYS + 8 * bx, stride = JYS, tbl = plane ? 1 : 0;
      return y0 + 8 * by < H && x0 + 8 * bx < W;
    }
    const int c = blk - 64, plane = c >= 36 ? 1 : 0, rr = c - 36 * plane, by = rr / 6, bx = rr - 6 * by;
    p = pl + JT * JYS + plane * JCN * JCS + 8 * by * JCS + 8 * bx, stride = JCS, tbl = 1;
    const int oy = cy0 + 8 * by, ox = cx0 + 8 * bx;
    return oy >= 0 && ox >= 0 && oy < ch && ox < cw;
  };

  // ---- 2. forward DCT, rows
  for (int item = tid; item < NBLK * 8; item += 256) {
    int *p, stride, tbl;
    if (!block_at(item >> 3, p, stride, tbl)) continue;
    int4 *v = reinterpret_cast<int4 *>(p + (item & 7) * stride);
    const int4 lo = v[0], hi = v[1];
    int d[8] = {lo.x - 128, lo.y - 128, lo.z - 128, lo.w - 128, hi.x - 128, hi.y - 128, hi.z - 128, hi.w - 128};
    jpeg_fdct8<true>(d);
    v[0] = make_int4(d[0], d[1], d[2], d[3]), v[1] = make_int4(d[4], d[5], d[6], d[7]);
  }
  __syncthreads();

  // ---- 3. forward DCT columns, quantise, dequantise, inverse DCT columns
  for (int item = tid; item < NBLK * 8; item += 256) {
    int *p, stride, tbl;
    if (!block_at(item >> 3, p, stride, tbl)) continue;
    const int c = item & 7;
    p += c;
    int d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = p[i * stride];
    jpeg_fdct8<false>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int Q = qt[tbl][8 * i + c];
      const int k = (int)__umulhi((uint32_t)(abs(d[i]) + 4 * Q), qm[tbl][8 * i + c]) * Q;
      d[i] = d[i] < 0 ? -k : k;
    }
    jpeg_idct8<11>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i * stride] = d[i];
  }
  __syncthreads();

  // ---- 4. inverse DCT rows -> samples
  for (int item = tid; item < NBLK * 8; item += 256) {
    int *p, stride, tbl;
    if (!block_at(item >> 3, p, stride, tbl)) continue;
    int4 *v = reinterpret_cast<int4 *>(p + (item & 7) * stride);
    const int4 lo = v[0], hi = v[1];
    int d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    jpeg_idct8<18>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = clamp255(d[i] + 128);
    v[0] = make_int4(d[0], d[1], d[2], d[3]), v[1] = make_int4(d[4], d[5], d[6], d[7]);
  }
  __syncthreads();

  // ---- 5. chroma up, colour back, store
  for (int item = tid; item < JT * (JT / 4); item += 256) {
    const int row = item >> 4, col = 4 * (item & 15), py = y0 + row, px = x0 + col;
    if (py >= H || px >= W) continue;
    const int *yv = yp + row * JYS + col;
    uint32_t v[4];
    if constexpr (S420) {
      const int *cbp = pl + JT * JYS, *crp = cbp + JCN * JCS;
      const int cy = py >> 1, cx = px >> 1;
      const int rc = (cy - cy0) * JCS;
      if (cw <= 2) {  // the decoder replicates chroma planes no wider than 2 samples (W <= 4: cx = 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int xi = min(cx + (i >> 1), cw - 1) - cx0;
          v[i] = jpeg_rgb(yv[i], cbp[rc + xi], crp[rc + xi]);
        }
      } else {
        const int rn = (((py & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0)) - cy0) * JCS;
        int sb[4], sr[4];  // 3 c[cy][x] + c[neighbour row][x] at x = cx - 1 .. cx + 2, clamped to the plane
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int xi = min(max(cx - 1 + k, 0), cw - 1) - cx0;
          sb[k] = 3 * cbp[rc + xi] + cbp[rn + xi], sr[k] = 3 * crp[rc + xi] + crp[rn + xi];
        }
        v[0] = jpeg_rgb(yv[0], (3 * sb[1] + sb[0] + 8) >> 4, (3 * sr[1] + sr[0] + 8) >> 4);
        v[1] = jpeg_rgb(yv[1], (3 * sb[1] + sb[2] + 7) >> 4, (3 * sr[1] + sr[2] + 7) >> 4);
        v[2] = jpeg_rgb(yv[2], (3 * sb[2] + sb[1] + 8) >> 4, (3 * sr[2] + sr[1] + 8) >> 4);
        v[3] = jpeg_rgb(yv[3], (3 * sb[2] + sb[3] + 7) >> 4, (3 * sr[2] + sr[3] + 7) >> 4);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = jpeg_rgb(yv[i], yv[JT * JYS + i], yv[2 * JT * JYS + i]);
    }
    jpeg_store4(dst + py * pitch, px, W, a.dst_vec, v);
  }
}

}  // namespace edvr

extern "C" int edvr_jpeg_roundtrip_u8(const uint8_t *src, uint8_t *dst, const int32_t *quality, int quality_all, int n, int H, int W,
                                      int64_t src_image_stride, int64_t dst_image_stride, int subsampling, edvr_stream_t stream) {
  using namespace edvr;
  EDVR_REQUIRE(src && dst && n > 0 && n <= 65535 && H > 0 && W > 0, "jpeg_roundtrip: bad arguments");
  EDVR_REQUIRE(subsampling == EDVR_JPEG_420 || subsampling == EDVR_JPEG_444, "jpeg_roundtrip: subsampling %d is not EDVR_JPEG_420 or EDVR_JPEG_444",
               subsampling);
  EDVR_REQUIRE(quality || (quality_all >= 0 && quality_all <= 100), "jpeg_roundtrip: quality %d is outside 0 ... 100", quality_all);
  EDVR_REQUIRE((int64_t)H * W <= (int64_t)1 << 29, "jpeg_roundtrip: a %d x %d frame is too large", H, W);
  const int64_t frame = 3 * (int64_t)H * W;
  if (src_image_stride == 0) src_image_stride = frame;
  if (dst_image_stride == 0) dst_image_stride = frame;
  EDVR_REQUIRE(n == 1 || (src_image_stride >= frame && dst_image_stride >= frame), "jpeg_roundtrip: an image stride is shorter than a frame of %lld bytes",
               (long long)frame);
  JpegArgs a;
  a.src = src, a.dst = dst, a.quality = quality, a.quality_all = quality_all, a.H = H, a.W = W;
  a.src_stride = src_image_stride, a.dst_stride = dst_image_stride;
  a.src_vec = W % 4 == 0 && jpeg_aligned4(src, src_image_stride, n);
  a.dst_vec = W % 4 == 0 && jpeg_aligned4(dst, dst_image_stride, n);
  const dim3 grid((unsigned)(cdiv(W, JT) * cdiv(H, JT)), (unsigned)n);
  if (subsampling == EDVR_JPEG_420) hipLaunchKernelGGL((jpeg_roundtrip_kernel<true>), grid, dim3(256), 0, as_stream(stream), a);
  else hipLaunchKernelGGL((jpeg_roundtrip_kernel<false>), grid, dim3(256), 0, as_stream(stream), a);
  return check_launch("jpeg_roundtrip_kernel");
}
