// mpeg.hip - the MPEG-style round trip on the device: what a clip of 8-bit RGB frames looks like after an I / P video encoder and decoder,
// i.e. the inter-frame member of the family jpeg.hip is the intra-frame member of.  Definition: DESIGN 4.18 (M1 - M7) - the planes, DCT and
// colour steps of DESIGN 4.16, an intra frame quantised by the MPEG-2 default matrix, and predicted frames: a full search over
// [-R, R]^2 per 16 x 16 macroblock against the previous RECONSTRUCTION, a half-sample chroma vector, a flat dead-zone quantiser on the
// residual.  Entropy coding is lossless and is not performed; no stream compatibility is claimed.  All arithmetic is 32-bit integer.
//
// t + 2 launches per call, on planes kept as bytes in a workspace ([2][b t] frames of Hp Wp luma + two Hp/2 Wp/2 chroma bytes):
//   1. mpeg_planes_kernel: every frame -> its padded source planes (M1);
//   2. mpeg_frame_kernel<INTRA>, once per frame index, grid (32 x 32 tiles across, down, b): a workgroup of four waves, ONE WAVE PER MACROBLOCK.
//      Predicted: the wave keeps its macroblock's search window of the previous reconstruction as bytes in LDS, the clamp resolved
//      ((16 + 2R) rows of 48 bytes; aligned dword loads where nothing clamps, clamped byte loads at the plane's edge), and its source
//      luma as 64 dwords.  A lane takes 4 rows of the block for one dy and FOUR adjacent dx: v_qsad_pk_u16_u8 gives the four byte-SADs of a ref quad-word against a source dword in 16-bit lanes (4 x 16 x 255 fits);
//      the four row quarters sit in adjacent lanes and are added packed, the key of M4 is reduced with an integer min across the wave.
//      Then prediction, the six residual blocks in jpeg.hip's lane layout (a row, then a column, then a row of a block per lane), and
//      the reconstruction is stored.  Intra: the same with a prediction of 128 and the matrix quantiser;
//   3. mpeg_output_kernel: every reconstruction -> RGB (M7).
// The quantisers divide by multiplying with floor(2^32 / 8Q) + 1 from a table built at compile time (exact below 2^21): no lane divides.
#include "jpeg_dct.h"

namespace edvr {

struct MpegArgs {
  const uint8_t *src;
  uint8_t *dst;
  uint8_t *ws;             // source planes of the b t frames, then their reconstructions
  const int32_t *qscale;   // per clip, or null
  int qscale_all;
  int b, t, H, W, Hp, Wp;
  int frame;               // the frame index of a mpeg_frame_kernel launch
  uint32_t rcp_t;          // t >= 2: floor(2^32 / t) + 1 (for t = 1 it would not fit 32 bits: mpeg_clip_of)
  int R;
  int64_t src_clip, src_frame, dst_clip, dst_frame;  // bytes between clips / frames
  int src_vec, dst_vec;                              // every pixel quad of a row starts on a 4-byte boundary
};

constexpr int MWS = 12;              // dwords of a search window row: 16 + 2 * 15 bytes, and the 4 dx of the last lane group
constexpr int MWR = 16 + 2 * 15;     // rows of the largest window
constexpr int MYS = 20, MCS = 12;    // words of a luma / chroma row of the macroblock's planes (= 20, 12 mod 32 banks: see jpeg.hip)
constexpr int MPL = 16 * MYS + 2 * 8 * MCS;
constexpr int MPEG_QMAX = 161;       // the largest intra step: (83 * 31 + 8) >> 4

__device__ __constant__ uint8_t mpeg_intra_w[64] = {8,  16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34, 34, 38, 22, 22, 26, 27, 29, 34, 37, 40,
                                                    22, 26, 27, 29, 32, 35, 40, 48, 26, 27, 29, 32, 35, 40, 48, 58, 26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83};

struct MpegRcp {
  uint32_t v[MPEG_QMAX + 1];  // [Q] = floor(2^32 / 8Q) + 1
  constexpr MpegRcp() : v{} {
    for (int q = 1; q <= MPEG_QMAX; ++q) v[q] = (uint32_t)(0x100000000ull / (uint32_t)(8 * q)) + 1u;
  }
};
__device__ __constant__ MpegRcp mpeg_rcp = MpegRcp();

__device__ __forceinline__ int64_t mpeg_plane_bytes(const MpegArgs &a) { return (int64_t)a.Hp * a.Wp * 3 / 2; }
// frame f of the call -> its clip, f / t: for t >= 2 umulhi(f, floor(2^32 / t) + 1), exact while f t < 2^32 (f < 65535 here); t = 1: f itself
__device__ __forceinline__ int mpeg_clip_of(const MpegArgs &a, int f) { return a.t == 1 ? f : (int)__umulhi((uint32_t)f, a.rcp_t); }
__device__ __forceinline__ int mpeg_q(const MpegArgs &a, int clip) { return a.qscale ? min(max(a.qscale[clip], 0), 31) : a.qscale_all; }

// ---- M1: block (64, 4), grid (column groups / 64, row pairs / 4, b t); a lane converts 4 pixels of a row pair: 8 luma samples, two cells of either chroma plane
__global__ __launch_bounds__(256) void mpeg_planes_kernel(const MpegArgs a) {
  const int f = blockIdx.z, clip = mpeg_clip_of(a, f), fi = f - clip * a.t;
  if (mpeg_q(a, clip) == 0) return;
  const int H = a.H, W = a.W, Hp = a.Hp, Wp = a.Wp;
  const int cy = blockIdx.y * 4 + threadIdx.y, g = blockIdx.x * 64 + threadIdx.x;
  if (cy >= (Hp >> 1) || g >= (Wp >> 2)) return;
  const int ch = (H + 1) >> 1;
  const int cyc = min(cy, ch - 1);  // below the frame the last CHROMA row repeats ...
  const int ra = 2 * cyc, rb = min(2 * cyc + 1, H - 1);
  const uint8_t *src = a.src + clip * a.src_clip + fi * a.src_frame;
  const int64_t pitch = 3 * (int64_t)W;
  int r[2][4], gg[2][4], bb[2][4];
  jpeg_load4(src + ra * pitch, 4 * g, W, a.src_vec, r[0], gg[0], bb[0]);
  jpeg_load4(src + rb * pitch, 4 * g, W, a.src_vec, r[1], gg[1], bb[1]);
  int scb[2] = {1, 2}, scr[2] = {1, 2};  // the bias: 1 in even chroma columns, 2 in odd ones
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) scb[i >> 1] += jpeg_cb(r[j][i], gg[j][i], bb[j][i]), scr[i >> 1] += jpeg_cr(r[j][i], gg[j][i], bb[j][i]);
  uint8_t *yp = a.ws + f * mpeg_plane_bytes(a), *cbp = yp + (int64_t)Hp * Wp, *crp = cbp + (int64_t)(Hp >> 1) * (Wp >> 1);
  const int j0 = cy > ch - 1 ? 1 : 0;  // ... and the last luma ROW (rb = H - 1 there)
  uint32_t y0 = 0, y1 = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) y0 |= (uint32_t)jpeg_y(r[j0][i], gg[j0][i], bb[j0][i]) << (8 * i), y1 |= (uint32_t)jpeg_y(r[1][i], gg[1][i], bb[1][i]) << (8 * i);
  *reinterpret_cast<uint32_t *>(yp + (int64_t)(2 * cy) * Wp + 4 * g) = y0;
  *reinterpret_cast<uint32_t *>(yp + (int64_t)(2 * cy + 1) * Wp + 4 * g) = y1;
  const int64_t co = (int64_t)cy * (Wp >> 1) + 2 * g;
  *reinterpret_cast<uint16_t *>(cbp + co) = (uint16_t)((scb[0] >> 2) | ((scb[1] >> 2) << 8));
  *reinterpret_cast<uint16_t *>(crp + co) = (uint16_t)((scr[0] >> 2) | ((scr[1] >> 2) << 8));
}

// ---- M3 / M4 - M6: grid (32 x 32 tiles across, down, b), one wave per macroblock
template <bool INTRA>
__global__ __launch_bounds__(256) void mpeg_frame_kernel(const MpegArgs a) {
  __shared__ __attribute__((aligned(16))) int pl_all[4][MPL];  // per wave: Y [16][20], Cb, Cr [8][12]
  __shared__ uint32_t win_all[INTRA ? 1 : 4][INTRA ? 1 : MWR * MWS];
  __shared__ uint32_t cur_all[INTRA ? 1 : 4][INTRA ? 1 : 64];
  __shared__ uint8_t predc_all[INTRA ? 1 : 4][INTRA ? 1 : 128];
  __shared__ int qt[INTRA ? 64 : 1];
  __shared__ uint32_t qm[INTRA ? 64 : 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, clip = blockIdx.z;
  const int q = mpeg_q(a, clip);
  if (q == 0) return;  // (uniform over the workgroup) the clip passes through: mpeg_output_kernel copies it
  const int Hp = a.Hp, Wp = a.Wp, Hc = Hp >> 1, Wc = Wp >> 1, R = a.R;
  const int ty = blockIdx.y, tx = blockIdx.x;
  const int my = 32 * ty + 16 * (wave >> 1), mx = 32 * tx + 16 * (wave & 1);
  const bool active = my < Hp && mx < Wp;  // (uniform over the wave)
  const int64_t pb = mpeg_plane_bytes(a), nf = (int64_t)a.b * a.t, f = (int64_t)clip * a.t + a.frame;
  const uint8_t *sy = a.ws + f * pb, *scb = sy + (int64_t)Hp * Wp, *scr = scb + (int64_t)Hc * Wc;
  uint8_t *ry = a.ws + (nf + f) * pb, *rcb = ry + (int64_t)Hp * Wp, *rcr = rcb + (int64_t)Hc * Wc;
  const uint8_t *py = ry - pb, *pcb = rcb - pb, *pcr = rcr - pb;  // the previous frame's reconstruction (a predicted frame is never frame 0)
  int *const pl = pl_all[wave];
  uint32_t *const win = win_all[INTRA ? 0 : wave], *const cur = cur_all[INTRA ? 0 : wave];
  uint8_t *const predc = predc_all[INTRA ? 0 : wave];
  const uint8_t *const winb = reinterpret_cast<const uint8_t *>(win);

  const int ly = lane >> 2, lx = 4 * (lane & 3);  // luma: a lane owns 4 samples of a row
  const int cyl = lane >> 3, cxl = lane & 7;      // chroma: one sample of either plane
  uint32_t cw = 0;
  if (active) cw = *reinterpret_cast<const uint32_t *>(sy + (int64_t)(my + ly) * Wp + mx + lx);
  int dy = 0, dx = 0;

  if constexpr (INTRA) {
    if (tid < 64) {
      const int Q = tid == 0 ? 8 : max(1, ((int)mpeg_intra_w[tid] * q + 8) >> 4);
      qt[tid] = Q, qm[tid] = mpeg_rcp.v[Q];
    }
  } else {
    // ---- the search window of the previous reconstruction, the clamp resolved; the source luma
    if (active) {
      cur[lane] = cw;
      const int nitems = (16 + 2 * R) * MWS;
      const int wx0 = mx - R, ax0 = wx0 & ~3;  // the window's first column, and the dword it lies in (planes and rows are 4-byte aligned)
      if (my - R >= 0 && my + 15 + R < Hp && wx0 >= 0 && ax0 + 4 * (MWS + 1) <= Wp) {
        // (uniform over the wave) nothing clamps: two aligned dwords and v_alignbyte_b32 instead of four clamped byte loads
        const uint32_t sh = (uint32_t)(wx0 & 3);
        for (int item = lane; item < nitems; item += 64) {
          const int wy = item / MWS, wd = item - wy * MWS;
          const uint32_t *p = reinterpret_cast<const uint32_t *>(py + (int64_t)(my - R + wy) * Wp + ax0) + wd;
          win[item] = __builtin_amdgcn_alignbyte(p[1], p[0], sh);
        }
      } else {
        for (int item = lane; item < nitems; item += 64) {
          const int wy = item / MWS, wd = item - wy * MWS;
          const uint8_t *row = py + (int64_t)min(max(my - R + wy, 0), Hp - 1) * Wp;
          uint32_t v = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) v |= (uint32_t)row[min(max(wx0 + 4 * wd + k, 0), Wp - 1)] << (8 * k);
          win[item] = v;
        }
      }
    }
    __syncthreads();
    // ---- M4: full search.  A lane: rows 4 qr .. 4 qr + 3 of the block, one dy, dx = 4 g - R .. 4 g + 3 - R
    if (active) {
      const int lg = R < 2 ? 0 : R < 4 ? 1 : R < 8 ? 2 : 3;  // 2^lg groups of four dx cover 2R + 1 of them
      const int ncand = (2 * R + 1) << lg;
      const int qr = lane & 3;
      uint32_t cq[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) cq[r][j] = cur[(4 * qr + r) * 4 + j];
      uint32_t best = 0xffffffffu;
      for (int base = 0; base < ncand; base += 16) {
        const int cg = base + (lane >> 2);
        const bool valid = cg < ncand;
        const int dyo = valid ? cg >> lg : 0, g = valid ? cg & ((1 << lg) - 1) : 0;
        const uint32_t *wp = win + (dyo + 4 * qr) * MWS + g;
        uint64_t acc = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          uint32_t w[5];
#pragma unroll
          for (int j = 0; j < 5; ++j) w[j] = wp[r * MWS + j];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_qsad_pk_u16_u8((uint64_t)w[j] | ((uint64_t)w[j + 1] << 32), cq[r][j], acc);
        }
        // the four row quarters: adjacent lanes, added packed (a whole block's SAD is at most 65280)
        uint32_t lo = (uint32_t)acc, hi = (uint32_t)(acc >> 32);
        lo += (uint32_t)__shfl_xor((int)lo, 1), hi += (uint32_t)__shfl_xor((int)hi, 1);
        lo += (uint32_t)__shfl_xor((int)lo, 2), hi += (uint32_t)__shfl_xor((int)hi, 2);
        const uint32_t sad[4] = {lo & 0xffffu, lo >> 16, hi & 0xffffu, hi >> 16};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int dxo = 4 * g + k;
          const uint32_t cost = sad[k] + (uint32_t)(q * (abs(dyo - R) + abs(dxo - R)));
          const uint32_t key = (cost << 10) | (uint32_t)((dyo - R + 15) << 5) | (uint32_t)(dxo - R + 15);
          if (valid && dxo <= 2 * R) best = min(best, key);
        }
      }
#pragma unroll
      for (int off = 4; off < 64; off <<= 1) best = min(best, (uint32_t)__shfl_xor((int)best, off));
      dy = (int)((best >> 5) & 31) - 15, dx = (int)(best & 31) - 15;
    }
  }

  // ---- M5 and the residual (intra: sample - 128) into the macroblock's planes
  if (active) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pred = INTRA ? 128 : (int)winb[(ly + dy + R) * (4 * MWS) + lx + i + dx + R];
      pl[ly * MYS + lx + i] = (int)((cw >> (8 * i)) & 255) - pred;
    }
    const int64_t co = (int64_t)((my >> 1) + cyl) * Wc + (mx >> 1) + cxl;
    int pb_ = 128, pr_ = 128;
    if constexpr (!INTRA) {
      const int iy = dy >> 1, hy = dy & 1, ix = dx >> 1, hx = dx & 1;
      const int ya = min(max((my >> 1) + cyl + iy, 0), Hc - 1), yb = min(max((my >> 1) + cyl + iy + hy, 0), Hc - 1);
      const int xa = min(max((mx >> 1) + cxl + ix, 0), Wc - 1), xb = min(max((mx >> 1) + cxl + ix + hx, 0), Wc - 1);
      const int64_t oaa = (int64_t)ya * Wc + xa, oab = (int64_t)ya * Wc + xb, oba = (int64_t)yb * Wc + xa, obb = (int64_t)yb * Wc + xb;
      pb_ = ((int)pcb[oaa] + pcb[oab] + pcb[oba] + pcb[obb] + 2) >> 2;
      pr_ = ((int)pcr[oaa] + pcr[oab] + pcr[oba] + pcr[obb] + 2) >> 2;
      predc[lane] = (uint8_t)pb_, predc[64 + lane] = (uint8_t)pr_;
    }
    pl[16 * MYS + cyl * MCS + cxl] = (int)scb[co] - pb_;
    pl[16 * MYS + 8 * MCS + cyl * MCS + cxl] = (int)scr[co] - pr_;
  }
  __syncthreads();

  // block `blk` of the macroblock (4 luma, Cb, Cr): where it starts, its row stride
  int *bp = nullptr;
  int bs = 0;
  const bool work = active && lane < 48;
  {
    const int blk = lane >> 3;
    if (blk < 4) bp = pl + 8 * (blk >> 1) * MYS + 8 * (blk & 1), bs = MYS;
    else bp = pl + 16 * MYS + (blk - 4) * 8 * MCS, bs = MCS;
  }
  const int e = lane & 7;

  // ---- forward DCT, rows
  if (work) {
    int4 *v = reinterpret_cast<int4 *>(bp + e * bs);
    const int4 lo = v[0], hi = v[1];
    int d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    jpeg_fdct8<true>(d);
    v[0] = make_int4(d[0], d[1], d[2], d[3]), v[1] = make_int4(d[4], d[5], d[6], d[7]);
  }
  __syncthreads();

  // ---- forward DCT columns, quantise, dequantise, inverse DCT columns
  if (work) {
    int *p = bp + e;
    int d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = p[i * bs];
    jpeg_fdct8<false>(d);
    if constexpr (INTRA) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int Q = qt[8 * i + e];
        const int k = (int)__umulhi((uint32_t)(abs(d[i]) + 4 * Q), qm[8 * i + e]) * Q;
        d[i] = d[i] < 0 ? -k : k;
      }
    } else {
      const uint32_t m = mpeg_rcp.v[q];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = (int)__umulhi((uint32_t)abs(d[i]), m);  // |c| / (8 qscale): the dead zone
        const int v = k ? ((2 * k + 1) * q) >> 1 : 0;
        d[i] = d[i] < 0 ? -v : v;
      }
    }
    jpeg_idct8<11>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i * bs] = d[i];
  }
  __syncthreads();

  // ---- inverse DCT rows
  if (work) {
    int4 *v = reinterpret_cast<int4 *>(bp + e * bs);
    const int4 lo = v[0], hi = v[1];
    int d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    jpeg_idct8<18>(d);
    v[0] = make_int4(d[0], d[1], d[2], d[3]), v[1] = make_int4(d[4], d[5], d[6], d[7]);
  }
  __syncthreads();

  // ---- prediction + residual, clamp, store the reconstruction
  if (active) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pred = INTRA ? 128 : (int)winb[(ly + dy + R) * (4 * MWS) + lx + i + dx + R];
      o |= (uint32_t)clamp255(pred + pl[ly * MYS + lx + i]) << (8 * i);
    }
    *reinterpret_cast<uint32_t *>(ry + (int64_t)(my + ly) * Wp + mx + lx) = o;
    const int64_t co = (int64_t)((my >> 1) + cyl) * Wc + (mx >> 1) + cxl;
    const int pb_ = INTRA ? 128 : (int)predc[lane], pr_ = INTRA ? 128 : (int)predc[64 + lane];
    rcb[co] = (uint8_t)clamp255(pb_ + pl[16 * MYS + cyl * MCS + cxl]);
    rcr[co] = (uint8_t)clamp255(pr_ + pl[16 * MYS + 8 * MCS + cyl * MCS + cxl]);
  }
}

// ---- M7: block (64, 4), grid (pixel quads / 64, rows / 4, b t); a lane upsamples the chroma of 4 pixels of a row, converts back and writes 12 bytes
__global__ __launch_bounds__(256) void mpeg_output_kernel(const MpegArgs a) {
  const int f = blockIdx.z, clip = mpeg_clip_of(a, f), fi = f - clip * a.t;
  const int H = a.H, W = a.W, Hp = a.Hp, Wp = a.Wp, Wc = Wp >> 1;
  const int py = blockIdx.y * 4 + threadIdx.y, px = 4 * (blockIdx.x * 64 + threadIdx.x);
  if (py >= H || px >= W) return;
  const int64_t pitch = 3 * (int64_t)W;
  const uint8_t *src = a.src + clip * a.src_clip + fi * a.src_frame;
  uint8_t *dst = a.dst + clip * a.dst_clip + fi * a.dst_frame;
  uint32_t v[4];
  if (mpeg_q(a, clip) == 0) {  // the clip passes through unchanged
    int r[4], g[4], b[4];
    jpeg_load4(src + py * pitch, px, W, a.src_vec, r, g, b);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (uint32_t)(r[i] | g[i] << 8 | b[i] << 16);
    jpeg_store4(dst + py * pitch, px, W, a.dst_vec, v);
    return;
  }
  const uint8_t *yp = a.ws + ((int64_t)a.b * a.t + f) * mpeg_plane_bytes(a), *cbp = yp + (int64_t)Hp * Wp, *crp = cbp + (int64_t)(Hp >> 1) * Wc;
  const uint32_t yw = *reinterpret_cast<const uint32_t *>(yp + (int64_t)py * Wp + px);
  const int yv[4] = {(int)(yw & 255), (int)((yw >> 8) & 255), (int)((yw >> 16) & 255), (int)(yw >> 24)};
  const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;  // the real chroma plane
  const int cy = py >> 1, cx = px >> 1;
  const int64_t rc = (int64_t)cy * Wc;
  if (cw <= 2) {  // the decoder replicates chroma planes no wider than 2 samples (W <= 4: cx = 0)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int xi = min(cx + (i >> 1), cw - 1);
      v[i] = jpeg_rgb(yv[i], cbp[rc + xi], crp[rc + xi]);
    }
  } else {
    const int64_t rn = (int64_t)((py & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0)) * Wc;
    int sb[4], sr[4];  // 3 c[cy][x] + c[neighbour row][x] at x = cx - 1 .. cx + 2, clamped to the plane
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int xi = min(max(cx - 1 + k, 0), cw - 1);
      sb[k] = 3 * cbp[rc + xi] + cbp[rn + xi], sr[k] = 3 * crp[rc + xi] + crp[rn + xi];
    }
    v[0] = jpeg_rgb(yv[0], (3 * sb[1] + sb[0] + 8) >> 4, (3 * sr[1] + sr[0] + 8) >> 4);
    v[1] = jpeg_rgb(yv[1], (3 * sb[1] + sb[2] + 7) >> 4, (3 * sr[1] + sr[2] + 7) >> 4);
    v[2] = jpeg_rgb(yv[2], (3 * sb[2] + sb[1] + 8) >> 4, (3 * sr[2] + sr[1] + 8) >> 4);
    v[3] = jpeg_rgb(yv[3], (3 * sb[2] + sb[3] + 7) >> 4, (3 * sr[2] + sr[3] + 7) >> 4);
  }
  jpeg_store4(dst + py * pitch, px, W, a.dst_vec, v);
}

static inline int mpeg_pad16(int v) { return (v + 15) & ~15; }

}  // namespace edvr

extern "C" size_t edvr_mpeg_roundtrip_workspace(int b, int t, int H, int W) {
  if (b < 1 || t < 1 || H < 1 || W < 1 || (int64_t)b * t > 65535 || H > 16384 || W > 16384) return 0;
  return (size_t)2 * b * t * ((size_t)edvr::mpeg_pad16(H) * edvr::mpeg_pad16(W) * 3 / 2);
}

extern "C" int edvr_mpeg_roundtrip_u8(const uint8_t *src, uint8_t *dst, const int32_t *qscale, int qscale_all, int b, int t, int H, int W,
                                      int64_t src_clip_stride, int64_t src_frame_stride, int64_t dst_clip_stride, int64_t dst_frame_stride, int gop,
                                      int search, void *ws, size_t ws_bytes, edvr_stream_t stream) {
  using namespace edvr;
  EDVR_REQUIRE(src && dst && b > 0 && t > 0 && b <= 65535 && (int64_t)b * t <= 65535 && H > 0 && W > 0, "mpeg_roundtrip: bad arguments");
  EDVR_REQUIRE(qscale || (qscale_all >= 0 && qscale_all <= 31), "mpeg_roundtrip: qscale %d is outside 0 ... 31", qscale_all);
  EDVR_REQUIRE(gop >= 0, "mpeg_roundtrip: gop %d is negative", gop);
  EDVR_REQUIRE(search >= 0 && search <= 15, "mpeg_roundtrip: search %d is outside 0 ... 15", search);
  EDVR_REQUIRE(H <= 16384 && W <= 16384, "mpeg_roundtrip: a %d x %d frame is too large", H, W);
  const int64_t frame = 3 * (int64_t)H * W;
  if (src_frame_stride == 0) src_frame_stride = frame;
  if (dst_frame_stride == 0) dst_frame_stride = frame;
  if (src_clip_stride == 0) src_clip_stride = t * src_frame_stride;
  if (dst_clip_stride == 0) dst_clip_stride = t * dst_frame_stride;
  EDVR_REQUIRE(t == 1 || (src_frame_stride >= frame && dst_frame_stride >= frame), "mpeg_roundtrip: a frame stride is shorter than a frame of %lld bytes",
               (long long)frame);
  EDVR_REQUIRE(b == 1 || (src_clip_stride >= (t - 1) * src_frame_stride + frame && dst_clip_stride >= (t - 1) * dst_frame_stride + frame),
               "mpeg_roundtrip: a clip stride is shorter than a clip (t - 1 frame strides and a frame of %lld bytes)", (long long)frame);
  const size_t need = edvr_mpeg_roundtrip_workspace(b, t, H, W);
  EDVR_REQUIRE(ws && ws_bytes >= need && reinterpret_cast<uintptr_t>(ws) % 4 == 0, "mpeg_roundtrip: workspace of %zu bytes (4-byte aligned) needed, %zu given",
               need, ws_bytes);
  MpegArgs a;
  a.src = src, a.dst = dst, a.ws = static_cast<uint8_t *>(ws), a.qscale = qscale, a.qscale_all = qscale_all;
  a.b = b, a.t = t, a.H = H, a.W = W, a.Hp = mpeg_pad16(H), a.Wp = mpeg_pad16(W), a.frame = 0, a.R = search;
  a.rcp_t = t == 1 ? 0u : (uint32_t)(0x100000000ull / (uint32_t)t) + 1u;
  a.src_clip = src_clip_stride, a.src_frame = src_frame_stride, a.dst_clip = dst_clip_stride, a.dst_frame = dst_frame_stride;
  a.src_vec = W % 4 == 0 && jpeg_aligned4(src, src_frame_stride, t) && jpeg_aligned4(src, src_clip_stride, b);
  a.dst_vec = W % 4 == 0 && jpeg_aligned4(dst, dst_frame_stride, t) && jpeg_aligned4(dst, dst_clip_stride, b);
  hipStream_t s = as_stream(stream);
  const unsigned frames = (unsigned)(b * t);
  hipLaunchKernelGGL(mpeg_planes_kernel, dim3((unsigned)cdiv(a.Wp / 4, 64), (unsigned)cdiv(a.Hp / 2, 4), frames), dim3(64, 4), 0, s, a);
  int rc = check_launch("mpeg_planes_kernel");
  if (rc != EDVR_OK) return rc;
  const dim3 grid((unsigned)cdiv(a.Wp, 32), (unsigned)cdiv(a.Hp, 32), (unsigned)b);
  for (int i = 0; i < t; ++i) {
    a.frame = i;
    if (i == 0 || (gop > 0 && i % gop == 0)) hipLaunchKernelGGL((mpeg_frame_kernel<true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((mpeg_frame_kernel<false>), grid, dim3(256), 0, s, a);
    rc = check_launch("mpeg_frame_kernel");
    if (rc != EDVR_OK) return rc;
  }
  hipLaunchKernelGGL(mpeg_output_kernel, dim3((unsigned)cdiv(cdiv(W, 4), 64), (unsigned)cdiv(H, 4), frames), dim3(64, 4), 0, s, a);
  return check_launch("mpeg_output_kernel");
}
