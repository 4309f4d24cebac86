/* edvr_amd.h - C ABI of libedvr_amd.so: the MI355X (gfx950) native EDVR hot path.
 *
 * Drop-in boundary.  These entry points are what the reference's FFI for this
 * path binds; each cites the reference interface it replaces (paths relative to
 * xinntao/EDVR = BasicSR v1.2.0):
 *
 *   edvr_dcnv2_fwd_f32  <- modulated_deform_conv_forward
 *                          basicsr/models/ops/dcn/src/deform_conv_ext.cpp:106-124
 *                          (driver deform_conv_cuda.cpp:490-569, kernel .cu:570-633)
 *   edvr_dcnv2_bwd_f32  <- modulated_deform_conv_backward
 *                          basicsr/models/ops/dcn/src/deform_conv_ext.cpp:126-147
 *                          (driver deform_conv_cuda.cpp:571-685, kernels .cu:635-767)
 *   edvr_conv2d_*       <- the at::conv2d / cuDNN calls under every nn.Conv2d of
 *                          basicsr/models/archs/edvr_arch.py (:37-66,139-155,230-244,322-353)
 *                          with the LeakyReLU/ReLU/residual/PixelShuffle/cat that follow them
 *                          (arch_util.py:92-95, edvr_arch.py:70,157,351,410-411) fused in.
 *   edvr_tsa_temporal_* <- TSAFusion.forward temporal attention, edvr_arch.py:171-184
 *   edvr_pool_*, edvr_upsample2x_*, edvr_tsa_combine_*, edvr_upsample4x_add_*
 *                       <- MaxPool2d/AvgPool2d(3,2,1), nn.Upsample(x2 bilinear) and the
 *                          elementwise tail of TSAFusion / EDVR.forward
 *                          (edvr_arch.py:144-145,158-159,190-213,414-419)
 *
 * Contract (all entry points):
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless stated; NCHW;
 *   - the caller allocates everything (outputs, gradients, workspace), as the
 *     reference's Python does (deform_conv.py:138-140,154-158);
 *   - asynchronous on `stream` (a hipStream_t; NULL = default stream), no host
 *     synchronisation, no allocation, no global state: re-entrant across streams;
 *   - returns 0 or a negative EDVR_ERR_* code; edvr_last_error() gives the
 *     message for the calling thread.  Kernel launch failures are returned, not
 *     printf'd (the reference only prints: deform_conv_cuda_kernel.cu:794-798).
 *   - there is NO CPU implementation behind this ABI.
 */
#ifndef EDVR_AMD_H
#define EDVR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EDVR_OK 0
#define EDVR_ERR_ARG (-1)          /* bad shape / null pointer / mismatched sizes */
#define EDVR_ERR_UNSUPPORTED (-2)  /* parameter combination not implemented */
#define EDVR_ERR_LAUNCH (-3)       /* HIP launch error */
#define EDVR_ERR_WORKSPACE (-4)    /* workspace too small */

typedef void *edvr_stream_t; /* hipStream_t */

const char *edvr_version(void);
const char *edvr_last_error(void);
/* Device-capability probe: 0 if the current HIP device is gfx950, else EDVR_ERR_UNSUPPORTED. */
int edvr_check_device(void);

/* ------------------------------------------------------------------ activations */
#define EDVR_ACT_NONE 0
#define EDVR_ACT_RELU 1
#define EDVR_ACT_LRELU 2 /* negative slope 0.1 (edvr_arch.py:70,157,248,356) */
#define EDVR_ACT_SIGMOID 3

#define EDVR_DCN_HALO_TAPWIN 16 /* halo_hint of edvr_dcnv2_fwd_f32 / edvr_dcnv1_fwd_f32: per-tap shifted windows (below) */
#define EDVR_DCN_SCATTER_AUTO 0
#define EDVR_DCN_SCATTER_DEVICE 1
#define EDVR_DCN_SCATTER_LDS 2
#define EDVR_DCN_SCATTER_STRIP 3
#define EDVR_DCN_SCATTER_LDS_WIDE 4
#define EDVR_CONV_AUTO 0
#define EDVR_CONV_DIRECT 1
#define EDVR_CONV_WINOGRAD 2
#define EDVR_CONV_WINOGRAD_F4 3 /* F(4x4,3x3): needs edvr_conv2d_desc.wpk_f4; falls back like EDVR_CONV_WINOGRAD where it does not apply */
#define EDVR_CONV_WINOGRAD_F4S 4 /* F(4x4,3x3) with split fp32 operands on the f16 matrix pipe: needs wpk_f4s and x_amax; falls back to
                                  * EDVR_CONV_WINOGRAD_F4's chain where it does not apply */

#define EDVR_OUT_NCHW 0
#define EDVR_OUT_PIXEL_SHUFFLE2 1 /* y[n, co/4, 2h+(co%4)/2, 2w+co%2]  (nn.PixelShuffle(2)) */

/* ------------------------------------------------------------------ conv2d (fp32 MFMA implicit GEMM)
 * y = act(conv(cat(x1, x2), W) + bias [+ pre]) + res1 + res2, kernel ks in {1,3}, pad = ks/2,
 * stride in {1,2}, dilation 1, groups 1.  Weights come pre-packed by
 * edvr_conv2d_pack_weight_f32 (layout [ci_pad][ks*ks][co_pad], co fastest; for 3x3 kernels followed by the
 * Winograd-transformed weights G g G^T as [ci_pad][16][co_pad64]).  3x3 / stride-1 layers with >= 48 output channels
 * and w > 16 run as Winograd F(2x2,3x3) on the fp32 MFMA (2.25x fewer multiplies, fp32 throughout; set the
 * environment variable EDVR_CONV_WINOGRAD=0 to force the direct kernel); with `wpk_f4` present, layers with w >= 32 and
 * w % 4 == 0 run as Winograd F(4x4,3x3) (2.25 multiplies per output and channel pair where the direct algorithm needs 9 and
 * F(2x2) 4; EDVR_WINOGRAD_F4=0 switches it off). */
typedef struct edvr_conv2d_desc {
  const float *x1;        /* (n, c1, h, w) */
  const float *x2;        /* optional second input, concatenated after x1 on the channel axis */
  int c1, c2;             /* c2 = 0 when x2 == NULL */
  int64_t x1_img_stride;  /* elements between consecutive images of x1 (>= c1*h*w) */
  int64_t x2_img_stride;
  int x2_div, x2_mul, x2_add; /* image map of x2: i2 = (i / x2_div) * x2_mul + x2_add; x2_div = 0 -> i2 = i */
  int n, h, w;
  const float *wpk;       /* packed weights */
  const float *bias;      /* (co) or NULL */
  int co, ks, stride;
  int act;                /* EDVR_ACT_*; applied to output channels >= act_from only */
  int act_from;
  const float *res1;      /* optional residuals, same shape as the NCHW output (n, co, ho, wo) */
  const float *res2;
  int64_t res1_img_stride, res2_img_stride;
  float *y;
  int64_t y_img_stride;   /* elements between images of y */
  int out_mode;           /* EDVR_OUT_* */
  int algo;               /* EDVR_CONV_AUTO | EDVR_CONV_DIRECT | EDVR_CONV_WINOGRAD (F(2x2); falls back to direct where not applicable) |
                           * EDVR_CONV_WINOGRAD_F4 (needs wpk_f4; falls back to F(2x2), then direct) */
  const float *gate;      /* optional (n, co, ho, wo): y *= gate > 0 ? 1 : gate_slope, applied after bias / act.  This is the
                           * backward of a ReLU (slope 0) / LeakyReLU (0.1) fused into the data-gradient conv that produces its
                           * input gradient (gate = the activation's forward output).  3x3 kernels, NCHW output, no sigmoid
                           * (EDVR_ERR_UNSUPPORTED otherwise).  The Winograd kernels take it when there are no residuals (their
                           * fused-fast epilogue; edvr_conv2d_gate_supported asks for exactly that), every other 3x3 case - with
                           * residuals, stride 2, small layers - runs in the direct kernel's generic store path. */
  int64_t gate_img_stride;
  float gate_slope;
  float y_scale;          /* y = y_scale * act(conv + bias) [gated] + res1 + res2; 0 means 1.  ResidualBlockNoBN's res_scale
                           * (arch_util.py:95).  3x3 kernels with the NCHW output only (EDVR_ERR_UNSUPPORTED for 1x1 / PixelShuffle); a scaled
                           * conv with <= 4 output channels runs on the MFMA kernel instead of the small-co VALU kernel. */
  const float *wpk_f4;    /* optional: the same weights packed by edvr_conv2d_pack_weight_f4_f32.  Its presence ALLOWS the
                           * F(4x4,3x3) Winograd kernel (csrc/winograd_f4.hip: 2.25 instead of 4 multiplies per output; fp32
                           * rounding error ~1e-6 of the output scale instead of ~2e-7) under EDVR_CONV_AUTO where that kernel is the
                           * fastest; NULL keeps the F(2x2) / direct choice.  edvr_amd's inference AND training paths (forward and
                           * data-gradient convs; the weight gradient stays in the F(2x2) domain) pass it by default. */
  float *abs_sum;         /* optional (n): abs_sum[i] += sum |y[i, c, :, :]| over the output channels c < abs_sum_channels, added with
                           * atomics in the epilogue (the caller zeroes the array; summation order is not deterministic).  This is the
                           * statistic behind DCNv2Pack's "Offset abs mean is ..., larger than 50" check (arch_util.py:248-253) taken
                           * where conv_offset's output is still in registers instead of re-reading it (edvr_abs_sum_f32).  Only the
                           * F(4x4) kernel has this epilogue, in its NCHW store only (EDVR_OUT_PIXEL_SHUFFLE2 has none): ask
                           * edvr_conv2d_abs_sum_supported; EDVR_ERR_UNSUPPORTED otherwise.  The sum is taken over conv + bias (+ the
                           * activation of channels >= act_from), BEFORE gate, y_scale and the residuals are applied. */
  int abs_sum_channels;
  const void *wpk_f4s;    /* optional: the weights packed by edvr_conv2d_pack_weight_f4s_f32 (csrc/winograd_f4s.hip).  Together with
                           * `x_amax` it ALLOWS the split-operand F(4x4,3x3) kernel: every fp32 operand travels as two f16 numbers
                           * (hi + lo, 22 significant bits, after a power-of-two scaling), all four cross products are accumulated in
                           * fp32 by v_mfma_f32_32x32x16_f16 - the fp32 kernel's arithmetic to within its own rounding level at 1/4 of
                           * its matrix-pipe time.  EDVR_WINOGRAD_F4S=0 switches it off under EDVR_CONV_AUTO. */
  const float *x_amax;    /* device pointer to ONE float >= max |x1|, |x2| (any upper bound: edvr_amax_f32, or a statistic the
                           * producer of x already has).  Read by the split-operand kernel only, to place the transformed input in
                           * the f16 range; a bound that is too SMALL overflows to infinities, one that is 2^k too large costs
                           * accuracy only for elements below 2^-18 of it.  Two consequences a caller should know: operands carry 22
                           * significant bits (fp32: 24), and ONE bound covers the whole launch - the low bits of an image's output
                           * depend on which other images share the launch (within the kernel's 3e-5 tolerance; per-image calls with
                           * per-image bounds remove the coupling). */
  float *y_amax;          /* optional, split-operand kernel only (EDVR_ERR_UNSUPPORTED elsewhere: ask edvr_conv2d_y_amax_supported): y_amax[0] =
                           * max(y_amax[0], max |y|) over everything the launch stores (residuals / gate applied), with one atomic per
                           * wave at the end - the `x_amax` of the next conv of a chain for free.  The caller zeroes it (or folds bounds).
                           * The maximum is kept as a BIT PATTERN (non-negative floats order as integers, every NaN above +inf): a
                           * non-finite output is sticky in the slot - an overflow sentinel the host can read (edvr_amd/ops.py split_guard_*). */
  const float *pre;       /* optional PRE-ACTIVATION addend (pre_n, co, h, w), plane-contiguous: y = act(conv + bias + pre[map(i)]) on every
                           * output channel, then y_scale / y_amax / abs_sum as without it (both statistics are taken from the final value,
                           * so a NaN or an infinity in `pre` reaches y, the y_amax slot and the host's guard as one in res1 does).  A
                           * convolution is linear in its input channels: conv(cat(a, b), W) = conv(a, W[:, :ca]) + conv(b, W[:, ca:]), so
                           * the half of a two-input conv whose x2 is shared by several images (x2_div / x2_mul / x2_add) can be convolved
                           * ONCE per shared image, without bias or activation, and enter here (PCDAlignment's offset convs: the reference
                           * frame's features are shared by the t frames of a clip, edvr_arch.py:64-86).  Only the two F(4x4) Winograd kernels
                           * implement it (csrc/winograd_f4s.hip, csrc/winograd_f4.hip: it rides in the registers and the prefetch slot of the
                           * residual / gate, which it therefore excludes), NCHW output only, 16-byte aligned: ask edvr_conv2d_pre_supported;
                           * EDVR_ERR_UNSUPPORTED otherwise.  NULL: every launch is what it was without this operand, bit for bit. */
  int64_t pre_img_stride; /* elements between consecutive images of pre (>= co*h*w) */
  int pre_div, pre_mul, pre_add; /* image map of pre, as x2's: ip = (i / pre_div) * pre_mul + pre_add; pre_div = 0 -> ip = i */
  int pre_n;              /* images in pre: the map of the last image, n - 1, must stay below it (EDVR_ERR_ARG) */
  const void *wpk_ds;     /* optional: the weights packed by edvr_conv2d_pack_weight_ds_f32 (csrc/conv2d_s.hip).  Together with `x_amax` it
                           * ALLOWS the split-operand form of the DIRECT kernel for a launch that no other kernel takes - 3x3 / stride 2,
                           * 3x3 / stride 1 where the Winograd kernels do not apply (few input channels), 1x1 below the streaming kernel's
                           * 320 channels: NCHW output, no gate / pre / abs_sum, y_scale 0 or 1, algo != EDVR_CONV_DIRECT, c1 % 4 == 0 when
                           * x2 is set.  Everything else runs as if it were NULL.  A field of its own (not wpk_f4s): a caller may hand both,
                           * the launch takes the one its kernel reads.  Same bound contract as wpk_f4s: `x_amax` >= max |x1|, |x2| (too
                           * small: infinities, which `y_amax` keeps as a sticky non-finite pattern); `y_amax` is supported
                           * (edvr_conv2d_y_amax_supported) and covers every stored element, residuals included. */
} edvr_conv2d_desc;

size_t edvr_conv2d_packed_weight_elems(int co, int ci, int ks);
/* w: (co, ci, ks, ks) -> wpk.  transpose_flip != 0 packs the data-gradient kernel instead:
 * w'(ci, co, ks, ks) with w'[c][o][i][j] = w[o][c][ks-1-i][ks-1-j] (then `co`/`ci` refer to w'). */
int edvr_conv2d_pack_weight_f32(const float *w, float *wpk, int co, int ci, int ks, int transpose_flip,
                                edvr_stream_t stream);
/* F(4x4,3x3) weights of a 3x3 conv: U = G g G^T in MFMA operand order, edvr_conv2d_packed_weight_f4_elems(co, ci) floats.
 * Replaces: the algorithm / filter-transform choice cuDNN makes for the reference's 3x3 nn.Conv2d layers under
 * torch.backends.cudnn.benchmark = True (basicsr/train.py:132; edvr_arch.py:24-71,190-244,322-352, arch_util.py:86-95).
 * transpose_flip as in edvr_conv2d_pack_weight_f32 (data-gradient kernel). */
size_t edvr_conv2d_packed_weight_f4_elems(int co, int ci);
int edvr_conv2d_pack_weight_f4_f32(const float *w, float *wpk_f4, int co, int ci, int transpose_flip, edvr_stream_t stream);
/* The same U for the split-operand kernel (EDVR_CONV_WINOGRAD_F4S): a 64-byte header (s_U = the power of two that puts max |w| in
 * [2^14, 2^15), and 1 / s_U, taken from the weights by a one-workgroup pre-pass on the same stream) followed by one dword
 * (f16 hi | f16 lo << 16) of U * s_U per element in that kernel's operand order.  edvr_conv2d_packed_weight_f4s_elems(co, ci) dwords,
 * 16-byte aligned.  Replaces the same cuDNN choice as edvr_conv2d_pack_weight_f4_f32. */
size_t edvr_conv2d_packed_weight_f4s_elems(int co, int ci);
int edvr_conv2d_pack_weight_f4s_f32(const float *w, void *wpk_f4s, int co, int ci, int transpose_flip, edvr_stream_t stream);
/* The split-operand packing of a 1x1 conv's weights (csrc/conv1x1_s.hip): the same 64-byte header followed by [channel quad][co padded
 * to 128][4 channels] dwords (f16 hi | f16 lo << 16) of w * s_W.  Passed as edvr_conv2d_desc.wpk_f4s of a ks == 1 launch (with x_amax) it
 * allows the split form of the streaming 1x1 kernel (>= 320 input channels, c1 and c2 multiples of 8; EDVR_CONV1X1_SPLIT=0 switches
 * it off): the fp32 kernel's result to within fp32 rounding.  Replaces: the cuDNN call under TSAFusion.feat_fusion's nn.Conv2d
 * (edvr_arch.py:190-193,229).  edvr_conv2d_packed_weight_1x1s_elems(co, ci) dwords, 16-byte aligned. */
size_t edvr_conv2d_packed_weight_1x1s_elems(int co, int ci);
int edvr_conv2d_pack_weight_1x1s_f32(const float *w, void *wpk_1x1s, int co, int ci, edvr_stream_t stream);
/* The split-operand packing for the direct kernel (csrc/conv2d_s.hip; ks = 1 or 3, forward orientation): the same 64-byte header
 * (s_W = the power of two that puts max |w| in [2^14, 2^15), and 1 / s_W) followed by [channel quad][tap][co padded to 32][4 channels]
 * dwords (f16 hi | f16 lo << 16) of w * s_W, the channels zero-filled up to a multiple of 8 (ks = 3) or 32 (ks = 1).  Passed as
 * edvr_conv2d_desc.wpk_ds.  Replaces: the cuDNN algorithm choice under the stride-2 nn.Conv2d of the pyramid (edvr_arch.py:37-66), conv_first
 * (:322) and the 1x1 convs of TSAFusion (:190-244).  edvr_conv2d_packed_weight_ds_elems(co, ci, ks) dwords, 16-byte aligned. */
size_t edvr_conv2d_packed_weight_ds_elems(int co, int ci, int ks);
int edvr_conv2d_pack_weight_ds_f32(const float *w, void *wpk_ds, int co, int ci, int ks, edvr_stream_t stream);
/* amax[0] = max(amax[0], max |x|) over n images of per_img contiguous floats, img_stride elements apart (the caller zeroes amax
 * before the first call; several tensors may be folded into one bound).  Feeds edvr_conv2d_desc.x_amax. */
int edvr_amax_f32(const float *x, float *amax, int n, int64_t per_img, int64_t img_stride, edvr_stream_t stream);
/* Many weights in ONE launch (the training path repacks every conv weight after each optimizer step: ~480 tiny launches per
 * iteration otherwise).  `jobs`: DEVICE array of n_jobs records of edvr_pack_job_bytes() = 64 bytes { const float *w; float *wpk;
 * float *wpk_f4; int32 co, ci, ks, transpose_flip; int32 first_block, n_blocks; void *wpk_f4s; 8 bytes padding }: wpk / wpk_f4 /
 * wpk_f4s as the three functions above fill them (any may be NULL; the 16 header dwords of a wpk_f4s buffer must be zero before
 * its FIRST use here), transpose_flip as above; job j owns the workgroups [first_block, first_block +
 * n_blocks) of the launch (ascending, contiguous from 0; any n_blocks >= 1 - 256 elements per workgroup and pass), total_blocks =
 * their sum.  Results are bit-identical to the per-tensor functions.  split_parity: -1 when no job has a wpk_f4s; else a counter the
 * caller increments per call (its low bit selects which header slot collects max |w| this time: one extra launch, no memset -
 * each call zeroes the other slot for the next one, so a buffer that was NOT part of the call directly before needs its header
 * dwords 2 and 3 zeroed by the caller). */
size_t edvr_pack_job_bytes(void);
int edvr_conv2d_pack_weights_multi(const void *jobs, int n_jobs, int total_blocks, int split_parity, edvr_stream_t stream);
int edvr_conv2d_f32(const edvr_conv2d_desc *d, edvr_stream_t stream);
/* The kernel edvr_conv2d_f32 would run `d` on, in order of precedence (the first whose own rules accept `d` takes the launch): the one
 * selection the launch and every query below derive from.  Nothing is dereferenced; -1 for a NULL descriptor. */
#define EDVR_CONV_KERNEL_SMALL 0        /* conv3x3_smallco_kernel: 3x3 / stride 1, co <= 4, EDVR_CONV_AUTO, no gate / y_scale */
#define EDVR_CONV_KERNEL_F4S 1          /* conv3x3_winograd_f4s_kernel: F(4x4) on split operands (wpk_f4s + x_amax) */
#define EDVR_CONV_KERNEL_F4 2           /* conv3x3_winograd_f4_kernel (wpk_f4) */
#define EDVR_CONV_KERNEL_F2 3           /* conv3x3_winograd_kernel: F(2x2) */
#define EDVR_CONV_KERNEL_1X1_SPLIT 4    /* conv1x1_split_kernel: streaming 1x1 on split operands (wpk_f4s + x_amax) */
#define EDVR_CONV_KERNEL_1X1_STREAM 5   /* conv1x1_stream_kernel */
#define EDVR_CONV_KERNEL_DIRECT_SPLIT 6 /* conv2d_split_kernel: the direct kernel on split operands (wpk_ds + x_amax) */
#define EDVR_CONV_KERNEL_DIRECT 7       /* conv2d_mfma_kernel: takes everything else */
int edvr_conv2d_kernel(const edvr_conv2d_desc *d);
/* 1 if `d` with a `gate` (and no residuals) would run in a Winograd kernel's fused epilogue (that kernel applies under d->algo,
 * the sizes and the EDVR_CONV_WINOGRAD environment switch), else 0 (edvr_conv2d_f32 still accepts the gate on the direct
 * kernel - correct, slower).  Callers that fuse an activation backward into a data-gradient conv ask first and keep the
 * two-launch form otherwise.  Pointers of `d` need not be set. */
int edvr_conv2d_gate_supported(const edvr_conv2d_desc *d);
/* 1 if edvr_conv2d_f32 would run `d` on a split-operand kernel (F(4x4), streaming 1x1 or direct), whose epilogue takes `y_amax`, else 0. */
int edvr_conv2d_y_amax_supported(const edvr_conv2d_desc *d);
/* 1 if edvr_conv2d_f32 would run `d` on a kernel whose epilogue takes `abs_sum` (the F(4x4) Winograd kernel), else 0. */
int edvr_conv2d_abs_sum_supported(const edvr_conv2d_desc *d);
/* 1 if edvr_conv2d_f32 would run `d` WITH a `pre` operand on a kernel whose epilogue takes it (an F(4x4) Winograd kernel, NCHW output, no
 * gate, no residuals), else 0.  Of the pointers of `d` only those that select the kernel need to be set (wpk_f4 / wpk_f4s, x_amax). */
int edvr_conv2d_pre_supported(const edvr_conv2d_desc *d);
/* The split-operand F(4x4) kernel (csrc/winograd_f4s.hip) runs the output pass of a work item (64 channels x 32 tiles) that lies wholly
 * inside the tensor on lean instances: plain NCHW store, act none / relu / lrelu with one slope for the block, at most one addend
 * (res1 or pre), no gate / res2 / abs_sum.  Same bits as the generic instances.  edvr_conv2d_f4s_set_lean(0) forces the generic ones
 * (as EDVR_F4S_LEAN=0 does from the start) and returns the previous setting; edvr_conv2d_f4s_lean_items: how many items of the launch
 * edvr_conv2d_f32 would make for `d` take a lean instance - 0 when that launch is not the split-operand kernel's.  Host only. */
int edvr_conv2d_f4s_set_lean(int on);
int edvr_conv2d_f4s_lean_items(const edvr_conv2d_desc *d);
/* Name of the kernel template instantiation edvr_conv2d_f32 would launch for `d` (as rocprofv3 prints it),
 * written to buf; returns 0 or EDVR_ERR_*.  Measurement aid only. */
int edvr_conv2d_kernel_name(const edvr_conv2d_desc *d, char *buf, size_t buf_len);
/* Flops the fp32 matrix cores EXECUTE for that launch: for the two Winograd kernels the number of v_mfma_f32_32x32x2_f32 issued
 * x 4096, tile and channel padding included (what rocprofv3's SQ_INSTS_VALU_MFMA_MOPS_F32 counts); for every other kernel the
 * algorithmic 2 * n * ho * wo * co * ci * ks^2.  Measurement aid only (bench.py's roofline fraction). */
int edvr_conv2d_executed_flops(const edvr_conv2d_desc *d, double *flops);

/* stride / pad / dil arguments of the DCN entry points below: a plain value n means (h, w) = (n, n); EDVR_HW(h, w) passes a
 * rectangular pair in one int (h <= 65535 in the low half, w + 1 in the high half).  The reference's DCNv1 Python takes pairs
 * (deform_conv.py:33-36,56-58 -> kW, kH, dW, dH, padW, padH, dilationW, dilationH of deform_conv_ext.cpp:51-104); its DCNv2 Python
 * only ever passes equal values (deform_conv.py:141-146).  Rectangular geometries run on the generic column-buffer kernels. */
#define EDVR_HW(h, w) ((int)(h) | (((int)(w) + 1) << 16))

/* ------------------------------------------------------------------ DCNv2 (modulated deformable conv)
 * x (B,C,H,W); offset (B, dg*2*kh*kw, Ho, Wo) channel = g*2K + 2k + {0:dy,1:dx};
 * mask (B, dg*kh*kw, Ho, Wo); weight (Co, C/groups, kh, kw); bias (Co) or NULL; y (B,Co,Ho,Wo).
 * offset_bstride / mask_bstride: elements between consecutive images of offset / mask
 * (0 = contiguous), so channel-sliced views of one conv_offset output can be passed without a copy.
 * Validity rule, every entry point below (forward, backward, DCNv1, every dtype, every kernel class and scatter strategy): a tap whose
 * sampling position (h, w) = regular position + offset lies outside (-1, H) x (-1, W) - offsets of any size, beyond the range of int,
 * +-inf and NaN included; NaN fails the comparisons, as in deform_conv_cuda_kernel.cu:618 - adds nothing to y, dX or dW and has
 * dOffset = dMask = 0 exactly, whatever its (finite) mask.  A diverging conv_offset yields zeros there, never NaN
 * (tests/test_gpu_dcn_poison.py).  x, mask, weight and dy are the caller's to keep finite: 0 x NaN is NaN here as in the reference.
 * act: EDVR_ACT_* applied to y in the GEMM epilogue (EDVR_ACT_NONE = the reference op; PCDAlignment
 * follows two of its four DCNs with LeakyReLU, edvr_arch.py:103-104,116).
 * halo_hint: performance hint only: every class computes the same operator, but their summation orders (and the tap-window class's
 * explicit fma chains) differ, so results agree to fp32 rounding (<= 2e-5 of the output scale, tests/test_gpu_dcn.py), not bit for bit.  The
 * Python layer picks the class from statistics of earlier calls that arrive asynchronously; EDVR_DCN_HINT_WAIT=1 makes that choice (and so
 * the bits) reproducible at the price of one host synchronisation per forward.  The EDVR signature (3x3, stride 1, pad 1,
 * dil 1, groups 1, (C/dg) % 8 == 0) runs a fused kernel that stages an input halo of R pixels around each tile in LDS
 * and falls back to global gathers for taps that leave it: 0 or 3 -> R = 3 (|offset| mostly < 3), 7 -> R = 7,
 * -1 -> skip the fused kernel (generic column-buffer path; always used for other signatures).
 * EDVR_DCN_HALO_TAPWIN (16) -> csrc/dcn_tapwin.hip: the walk is (group, tap, channel pair) and the staged window of every
 * (group, tap) is centred on that tap's displacement over the tile, so the cost does not depend on the offset MAGNITUDE as long as
 * the field is spatially smooth (+-2 px inside an 8 x 32 pixel tile) - what a trained conv_offset produces, and what the
 * reference's gather costs at any offset (.cu:570-633).  Needs W % 4 == 0, W >= 32, 8 or 16 channels per deformable group,
 * dg <= 8 and a 16-byte aligned x; otherwise the R = 7 kernel runs. */
size_t edvr_dcnv2_fwd_ws_bytes(int B, int C, int H, int W, int Co, int kh, int kw, int stride, int pad, int dil,
                               int groups, int dg);
int edvr_dcnv2_fwd_f32(const float *x, const float *offset, const float *mask, const float *weight,
                       const float *bias, float *y, int B, int C, int H, int W, int Co, int kh, int kw, int stride,
                       int pad, int dil, int groups, int dg, int64_t offset_bstride, int64_t mask_bstride, int act,
                       int halo_hint, void *ws, size_t ws_bytes, edvr_stream_t stream);

/* edvr_dcnv2_fwd_f32 with split fp32 operands on the f16 matrix pipe where the tap-window kernel applies (halo_hint EDVR_DCN_HALO_TAPWIN and
 * its constraints; csrc/dcn_tapwin_s.hip: weights and sampled columns as f16 (hi, lo) pairs, all four cross products, fp32 accumulation -
 * the fp32 kernel's result to within fp32 rounding at a quarter of its matrix-pipe time); identical to edvr_dcnv2_fwd_f32 everywhere
 * else.  xm_amax: device pointer to ONE float >= max |x| * max(1, max |mask|) (an upper bound; DCNv2Pack's masks are sigmoid outputs, so a
 * bound of |x| does).  edvr_dcnv2_fwd_split_applies: 1 if that kernel would run.  EDVR_DCN_SPLIT=0 switches it off.  Replaces the same
 * reference code as edvr_dcnv2_fwd_f32 (deform_conv_cuda.cpp:490-569, deform_conv_cuda_kernel.cu:570-633). */
int edvr_dcnv2_fwd_split_f32(const float *x, const float *offset, const float *mask, const float *weight, const float *bias,
                             float *y, int B, int C, int H, int W, int Co, int kh, int kw, int stride, int pad, int dil, int groups,
                             int dg, int64_t offset_bstride, int64_t mask_bstride, int act, int halo_hint, void *ws, size_t ws_bytes,
                             const float *xm_amax, edvr_stream_t stream);
int edvr_dcnv2_fwd_split_applies(const float *x, int B, int C, int H, int W, int Co, int kh, int kw, int stride, int pad, int dil, int groups,
                                 int dg, int halo_hint);
/* The weights of that kernel packed ONCE (they do not change between the calls of an inference run): edvr_dcnv2_split_pack_weight_f32
 * fills a caller-owned, 16-byte aligned buffer of edvr_dcnv2_split_packed_weight_elems(Co, C) dwords (scale pre-pass + packing, the two
 * launches edvr_dcnv2_fwd_split_f32 issues at every call) and edvr_dcnv2_fwd_split_packed_f32 runs the forward from it - valid only
 * where edvr_dcnv2_fwd_split_applies says 1 (anything else is an error); no workspace.  Same packed bytes, same y. */
size_t edvr_dcnv2_split_packed_weight_elems(int Co, int C);
int edvr_dcnv2_split_pack_weight_f32(const float *weight, void *wpk, int Co, int C, edvr_stream_t stream);
int edvr_dcnv2_fwd_split_packed_f32(const float *x, const float *offset, const float *mask, const void *wpk, const float *bias,
                                    float *y, int B, int C, int H, int W, int Co, int kh, int kw, int stride, int pad, int dil, int groups,
                                    int dg, int64_t offset_bstride, int64_t mask_bstride, int act, int halo_hint, const float *xm_amax,
                                    edvr_stream_t stream);
/* Name of the kernel edvr_dcnv2_fwd_f32 would launch for these arguments (as rocprofv3 prints it): dcn_tapwin_fwd_kernel,
 * dcn_fused_fwd_kernel or dcn_im2col_kernel (+ the conv kernel of its GEMM).  Measurement aid only. */
int edvr_dcnv2_fwd_kernel_name(const float *x, int B, int C, int H, int W, int Co, int kh, int kw, int stride, int pad, int dil,
                               int groups, int dg, int halo_hint, char *buf, size_t buf_len);

size_t edvr_dcnv2_bwd_ws_bytes(int B, int C, int H, int W, int Co, int kh, int kw, int stride, int pad, int dil,
                               int groups, int dg);
/* Gradients are OVERWRITTEN (no pre-zeroing needed).  dbias may be NULL.  dx accumulates by fp32
 * atomics (as the reference's col2im does, .cu:688), so its summation order is not deterministic. */
int edvr_dcnv2_bwd_f32(const float *x, const float *offset, const float *mask, const float *weight, const float *dy,
                       float *dx, float *doffset, float *dmask, float *dweight, float *dbias, int B, int C, int H,
                       int W, int Co, int kh, int kw, int stride, int pad, int dil, int groups, int dg,
                       int64_t offset_bstride, int64_t mask_bstride, int64_t doffset_bstride, int64_t dmask_bstride,
                       int scatter_hint, void *ws, size_t ws_bytes, edvr_stream_t stream);
/* The same with magnitude bounds: xm_amax / dy_amax = device pointers to ONE float >= max |x| * max(1, max |mask|) and >= max |dy|
 * (upper BOUNDS, as edvr_conv2d_desc.x_amax).  dW = sum dY col^T (deform_conv_cuda.cpp:664-672) then runs with both operands as f16
 * (hi, lo) pairs on the f16 matrix pipe (csrc/gemm_nt_s.hip): the fp32 result to within fp32 rounding.  Everything else is
 * edvr_dcnv2_bwd_f32.  edvr_dcnv2_bwd_split_applies: 1 unless EDVR_GEMM_SPLIT=0. */
int edvr_dcnv2_bwd_split_f32(const float *x, const float *offset, const float *mask, const float *weight, const float *dy,
                             float *dx, float *doffset, float *dmask, float *dweight, float *dbias, int B, int C, int H,
                             int W, int Co, int kh, int kw, int stride, int pad, int dil, int groups, int dg,
                             int64_t offset_bstride, int64_t mask_bstride, int64_t doffset_bstride, int64_t dmask_bstride,
                             int scatter_hint, void *ws, size_t ws_bytes, const float *xm_amax, const float *dy_amax,
                             edvr_stream_t stream);
int edvr_dcnv2_bwd_split_applies(void);
/* Name of the kernel that produces dx for these arguments (host only; the launch decides by the same function):
 * dcn_bwd_fused_kernel, dcn_bwd_dx_strip_kernel (followed by dcn_bwd_coord_kernel<false> for doffset / dmask),
 * dcn_bwd_coord_tile_kernel<3>, dcn_bwd_coord_tile_kernel<6> or dcn_bwd_coord_kernel (device atomics). */
int edvr_dcnv2_bwd_kernel_name(int B, int C, int H, int W, int Co, int kh, int kw, int stride, int pad, int dil, int groups, int dg,
                               int scatter_hint, char *buf, size_t buf_len);
/* scatter_hint (performance only, like halo_hint of the forward; results are the same up to the summation order of dx):
 * how the four corner contributions per (pixel, tap, channel) are accumulated into dx.
 *   EDVR_DCN_SCATTER_DEVICE (1): fp32 device atomics straight to dx, as the reference's col2im (.cu:688).  Fastest when the
 *       offset field is smooth (neighbouring pixels hit neighbouring addresses: 6 ms on the EDVR-L training layer), collapses
 *       when it is not (89 ms with white-noise offsets of 1 px).
 *   EDVR_DCN_SCATTER_LDS (2): per-tile LDS window flushed with one device atomic per touched element: 7 ms /
 *       14 ms on the same two cases (round 6: the window's float additions are compare-and-swap loops - the hardware's ds_add_f32 runs
 *       at 0.4 lane-operations per cycle and CU on gfx950 -: 12.0 -> 8.8 ms per call on a trained-like field).  3x3, stride 1, pad 1,
 *       dil 1, <= 16 channels per deformable group; else DEVICE is used.  The window reaches 3 px beyond the tile's 3x3 footprint;
 *       EDVR_DCN_SCATTER_LDS_WIDE (4): 6 px, for fields whose taps sit ~4 px out and more (a corner outside the window is a device atomic).
 *   EDVR_DCN_SCATTER_STRIP (3): no scatter at all for sub-pixel offsets - one wave owns whole channel planes, folds the 9 taps of a
 *       pixel into a 5x5 register patch, the patch onto its owner lanes with DPP wave shifts and the rows into a register ring;
 *       one uncontended atomic per dx element.  Taps with |offset| >= 1 fall back to device atomics one by one, so this is the
 *       choice for fresh / lightly trained offset convs.  3x3, stride 1, pad 1, dil 1 (any size; one wave per 64-column strip); else DEVICE.
 *       With 16 channels per deformable group, Co <= 128 and W >= 32 this hint selects the kernel that needs no dcol buffer at
 *       all (csrc/dcn_bwd_fused.hip: W^T dY slices consumed in the registers the matrix core leaves them in; dx through
 *       wave-private LDS rows for sub-pixel taps, device atomics for the others): 6.4 vs 8.6 ms on the EDVR-L training layer.
 *   EDVR_DCN_SCATTER_AUTO (0): LDS where applicable.
 * doffset_bstride / dmask_bstride (0 = contiguous): image strides of the two gradient outputs, so both can be
 * written straight into channel slices of one (B, 3*dg*K, Ho, Wo) buffer = the gradient of conv_offset's output. */

/* The same operator in float64 / float16: the other legs of the reference's AT_DISPATCH_FLOATING_TYPES_AND_HALF
 * (deform_conv_cuda_kernel.cu:781,811,843).  All tensors of one call have the type `dtype` names; EDVR_DTYPE_F32 forwards to the
 * entry points above (no activation, default hints).  float64 computes in float64 throughout (torch.autograd.gradcheck users);
 * float16 keeps tensors in float16 and every intermediate in float32.  Plain VALU kernels (csrc/dcn_any.hip): any geometry, not
 * the measured path.  Gradients are overwritten; dbias may be NULL.  One workspace size serves both directions. */
#define EDVR_DTYPE_F32 0
#define EDVR_DTYPE_F64 1
#define EDVR_DTYPE_F16 2
size_t edvr_dcnv2_any_ws_bytes(int dtype, int B, int C, int H, int W, int Co, int kh, int kw, int stride, int pad, int dil, int groups,
                               int dg);
int edvr_dcnv2_fwd_any(int dtype, const void *x, const void *offset, const void *mask, const void *weight, const void *bias, void *y, int B,
                       int C, int H, int W, int Co, int kh, int kw, int stride, int pad, int dil, int groups, int dg,
                       int64_t offset_bstride, int64_t mask_bstride, void *ws, size_t ws_bytes, edvr_stream_t stream);
int edvr_dcnv2_bwd_any(int dtype, const void *x, const void *offset, const void *mask, const void *weight, const void *dy, void *dx,
                       void *doffset, void *dmask, void *dweight, void *dbias, int B, int C, int H, int W, int Co, int kh, int kw, int stride,
                       int pad, int dil, int groups, int dg, int64_t offset_bstride, int64_t mask_bstride, int64_t doffset_bstride,
                       int64_t dmask_bstride, void *ws, size_t ws_bytes, edvr_stream_t stream);

/* DCNv1 (DeformConv / DeformConvPack: no mask, no bias) <- deform_conv_forward, deform_conv_backward_input,
 * deform_conv_backward_parameters, basicsr/models/ops/dcn/src/deform_conv_ext.cpp:51-104 (drivers deform_conv_cuda.cpp:152-488,
 * kernels .cu:190-465).  Same offset layout and gather as DCNv2; gradients are overwritten; dx by fp32 atomics.
 * The reference's im2col_step only sizes its column buffer and has no counterpart. */
size_t edvr_dcnv1_fwd_ws_bytes(int B, int C, int H, int W, int Co, int kh, int kw, int stride, int pad, int dil,
                               int groups, int dg);
int edvr_dcnv1_fwd_f32(const float *x, const float *offset, const float *weight, float *y, int B, int C, int H, int W,
                       int Co, int kh, int kw, int stride, int pad, int dil, int groups, int dg, int64_t offset_bstride,
                       int halo_hint, void *ws, size_t ws_bytes, edvr_stream_t stream);
size_t edvr_dcnv1_bwd_ws_bytes(int B, int C, int H, int W, int Co, int kh, int kw, int stride, int pad, int dil,
                               int groups, int dg);
int edvr_dcnv1_bwd_f32(const float *x, const float *offset, const float *weight, const float *dy, float *dx,
                       float *doffset, float *dweight, int B, int C, int H, int W, int Co, int kh, int kw, int stride,
                       int pad, int dil, int groups, int dg, int64_t offset_bstride, int64_t doffset_bstride,
                       int scatter_hint, void *ws, size_t ws_bytes, edvr_stream_t stream);

/* ------------------------------------------------------------------ TSA / PCD glue kernels (HBM-bound) */
/* Temporal attention (edvr_arch.py:171-184): prob[b,t,p] = sigmoid(sum_c emb[b,t,c,p]*emb_ref[b,c,p]);
 * out[b,t,c,p] = aligned[b,t,c,p] * prob[b,t,p].  prob_out (b,t,hw) may be NULL. */
int edvr_tsa_temporal_f32(const float *emb, const float *emb_ref, const float *aligned, float *out, float *prob_out,
                          int b, int t, int c, int hw, edvr_stream_t stream);
/* The same pass with two outputs: out as above (bit for bit), and out_rev[b,t-1-ti,c,p] = out[b,ti,c,p] - the modulated features of
 * every clip in reversed frame order (temporal-reversal self-ensemble, edvr_amd/video.py).  out, out_rev and aligned are distinct,
 * non-overlapping buffers (anything else is an error); t = 1 is legal (out_rev equals out in value). */
int edvr_tsa_temporal_pair_f32(const float *emb, const float *emb_ref, const float *aligned, float *out, float *out_rev,
                               int b, int t, int c, int hw, edvr_stream_t stream);
/* The head of TSA fusion in one pass over `aligned` (csrc/tsa_front_s.hip): temporal attention and the two 1x1 convs that read its
 * product - feat = act_feat(conv1x1(mod, W_feat) + b_feat), attn likewise, mod[b, j*c + k, p] = aligned[b,j,k,p] * prob[b,j,p] as
 * edvr_tsa_temporal_f32 defines it - without storing mod.  Bit for bit what edvr_tsa_temporal_f32 followed by two edvr_conv2d_f32 calls
 * on conv1x1_split_kernel give.  emb / aligned (b, t, c, h, w) dense, emb_ref (b, c, h, w) with dense images emb_ref_img_stride floats
 * apart; x_amax: device pointer to ONE float >= max |aligned| (a bound of mod as well: the sigmoid is <= 1); wq_*: the buffers of
 * edvr_conv2d_pack_weight_1x1s_f32(w, ., co, t * c), 16-byte aligned, each head with its own scale; act_*: EDVR_ACT_*; feat / attn
 * (b, co, h, w) dense; *_amax (may be NULL): max |y| slots with the semantics of edvr_conv2d_desc.y_amax (raw bit patterns, NaN sticky).
 * edvr_tsa_front_supported: the kernel's own limits (t <= 16, c % 8 == 0, co <= 128, a frame pair below 2 GB).
 * edvr_tsa_front_applies: THE eligibility rule of the fused path - no gradients, both convs 1x1 with bias and the same co, supported
 * shape, aligned buffers, and each conv one that edvr_conv2d_f32 would run on conv1x1_split_kernel (only then are the three launches
 * reproduced bit for bit); EDVR_TSA_FRONT=0 switches it off.  Replaces edvr_arch.py:171-193 (the ATen glue and two cuDNN calls). */
int edvr_tsa_front_supported(int b, int t, int c, int h, int w, int co);
int edvr_tsa_front_applies(int needs_grad, int b, int t, int c, int h, int w, int co_feat, int co_attn, int ks_feat, int ks_attn, int has_bias_feat,
                           int has_bias_attn, const void *wq_feat, const void *wq_attn, const float *x_amax);
int edvr_tsa_front_f32(const float *emb, const float *emb_ref, int64_t emb_ref_img_stride, const float *aligned, const float *x_amax,
                       const void *wq_feat, const float *bias_feat, int act_feat, float *feat, float *feat_amax, const void *wq_attn,
                       const float *bias_attn, int act_attn, float *attn, float *attn_amax, int b, int t, int c, int h, int w, int co,
                       edvr_stream_t stream);
/* MaxPool2d(3,2,1) and AvgPool2d(3,2,1, count_include_pad) in one pass; y (n, 2c, ho, wo) = cat(max, avg). */
int edvr_pool_maxavg_3x3s2_f32(const float *x, float *y, int n, int c, int h, int w, edvr_stream_t stream);
/* nn.Upsample(scale_factor=2, bilinear, align_corners=False); y = scale * up(x). */
int edvr_upsample2x_f32(const float *x, float *y, int nc, int h, int w, float scale, edvr_stream_t stream);
/* y = feat * sigmoid(attn) * 2 + attn_add  (edvr_arch.py:210-213). */
int edvr_tsa_combine_f32(const float *feat, const float *attn, const float *attn_add, float *y, int64_t numel,
                         edvr_stream_t stream);
/* y += bilinear x4 (align_corners=False) of base (n, c, h, w); y is (n, c, 4h, 4w)  (edvr_arch.py:417-419). */
int edvr_upsample4x_add_f32(const float *base, float *y, int nc, int h, int w, edvr_stream_t stream);
/* y = a + b */
int edvr_add_f32(const float *a, const float *b, float *y, int64_t numel, edvr_stream_t stream);
/* dz = dy * act'(.) expressed through the activation OUTPUT y (relu: y>0; lrelu: y>0 ? 1 : 0.1;
 * sigmoid: y(1-y)); channels < act_from of an (n, c, hw) tensor pass through unchanged. */
int edvr_act_bwd_f32(const float *dy, const float *y, const float *res1, const float *res2, float *dz, int n, int c,
                     int64_t hw, int act, int act_from, edvr_stream_t stream);
/* res1/res2 (nullable): the fused conv computed y = act(z) + res1 + res2; they are subtracted to recover act(z). */
/* out[i] = sum |x[i, :per_img]| for each of n images (image stride img_stride) - feeds the
 * "offset abs mean > 50" warning of arch_util.py:248-253 without a per-call host sync. */
int edvr_abs_sum_f32(const float *x, float *out, int n, int64_t per_img, int64_t img_stride, edvr_stream_t stream);
/* The same sums in out[0 .. n) plus, in out[n .. 2n), sum |x[i, c, r, col] - x[i, c, r, col + 1]| over the three neighbour pairs inside
 * every aligned group of four columns of the w-wide rows (3 of every 4 horizontal pairs; per_img % w == 0) - the ROUGHNESS of an
 * offset field: together with the sums it tells which DCN kernel suits the layer (a smooth field of any magnitude runs on the per-tap
 * windows, EDVR_DCN_HALO_TAPWIN).  (The F(4x4) conv epilogue only takes the plain sums, edvr_conv2d_desc.abs_sum: one more
 * accumulator in its staging waves spills - 128 registers - and costs the kernel 4 % on EVERY layer, measured.)
 * Rows that are not whole 16-byte groups (w % 4 != 0 or unaligned views): out[n .. 2n) = -1 (unknown). */
int edvr_abs_stats_f32(const float *x, float *out, int n, int64_t per_img, int w, int64_t img_stride, edvr_stream_t stream);

/* ------------------------------------------------------------------ training: gradients of the fused launches
 * (what autograd runs under SRModel.optimize_parameters, basicsr/models/sr_model.py:88-112) */
/* dW (co, c1+c2, ks, ks) (+)= sum_{n,pixel} dz[n,co,pixel] * cat(x1,x2)[n,ci,pixel*stride+tap-pad]; fp32 MFMA implicit GEMM,
 * deterministic split-K through `ws`.  x2 image map as in edvr_conv2d_desc. */
size_t edvr_conv2d_wgrad_ws_bytes(int n, int ci, int h, int w, int co, int ks, int stride);
int edvr_conv2d_wgrad_f32(const float *x1, const float *x2, const float *dz, float *dw, int c1, int c2, int n, int h, int w,
                          int co, int ks, int stride, int64_t x1_img_stride, int64_t x2_img_stride, int x2_div, int x2_mul,
                          int x2_add, int64_t dz_img_stride, int accumulate, float *dbias, void *ws, size_t ws_bytes,
                          edvr_stream_t stream);
/* The same with split fp32 operands on the f16 matrix pipe where the Winograd-domain kernel applies (both GEMM operands as f16 (hi, lo)
 * pairs, all four cross products, fp32 accumulation - the fp32 kernel's result to within its own rounding level): the Winograd-domain
 * form csrc/winograd_wgrad_s.hip; identical to edvr_conv2d_wgrad_f32 everywhere else.  Opt-in alternative (EDVR_WGRAD_DIRECT_SPLIT=1,
 * rows of 16-byte aligned tensors with w % 4 == 0; edvr_conv2d_wgrad_split_is_direct() says whether it would run): the DIRECT pixel-axis
 * GEMM csrc/wgrad_direct_s.hip - nothing is transformed, a value is split once and the nine taps are nine reads of the same LDS rows;
 * same accuracy, 10-15 % slower on MI355X (2.25x the matrix work meets the power-limited matrix clock, see that file).  x_amax / dz_amax: device pointers to
 * ONE float each, upper bounds of max |x1|, |x2| and of max |dz| (edvr_amax_f32 or a producer's statistic; too small = infinities).
 * edvr_conv2d_wgrad_split_applies: 1 if that kernel would run for this layer (callers skip computing the bounds otherwise).
 * EDVR_WGRAD_SPLIT=0 switches it off. */
int edvr_conv2d_wgrad_split_f32(const float *x1, const float *x2, const float *dz, float *dw, int c1, int c2, int n, int h, int w,
                                int co, int ks, int stride, int64_t x1_img_stride, int64_t x2_img_stride, int x2_div, int x2_mul,
                                int x2_add, int64_t dz_img_stride, int accumulate, float *dbias, void *ws, size_t ws_bytes,
                                const float *x_amax, const float *dz_amax, edvr_stream_t stream);
int edvr_conv2d_wgrad_split_applies(int n, int c1, int c2, int h, int w, int co, int ks, int stride);
int edvr_conv2d_wgrad_split_is_direct(int h, int w);
/* Name of the kernel edvr_conv2d_wgrad_f32 would launch for this layer (as rocprofv3 prints it).  Measurement aid only. */
int edvr_conv2d_wgrad_kernel_name(int n, int c1, int c2, int h, int w, int co, int ks, int stride, char *buf, size_t buf_len);
/* dbias (nullable): also db[co] = sum_{n,pixel} dz (the bias gradient).  The Winograd-domain kernel holds every dz value in
 * registers already and adds it to its two launches; the direct kernel runs edvr_channel_sum_f32 afterwards. */

/* Algorithm request for edvr_conv2d_wgrad_f32 (process-wide; tests and benchmarks use it to run both kernels on the same
 * layer): EDVR_CONV_AUTO (default: Winograd-domain kernel where eligible and profitable), EDVR_CONV_DIRECT, or
 * EDVR_CONV_WINOGRAD (wherever structurally possible: 3x3, stride 1, even h and w, c1 % 64 == 0 when x2 is given).
 * Returns the previous setting.  No reference counterpart (cuDNN picks its backward-filter algorithm internally). */
int edvr_conv2d_wgrad_algo(int algo);
/* out[c] = sum_{n,p} x[n,c,p]  (bias gradient); img_stride 0 = contiguous; ws: >= 64*c floats of scratch for the
 * deterministic two-stage reduction (NULL = single-stage, slower) */
int edvr_channel_sum_f32(const float *x, float *out, int n, int c, int64_t hw, int64_t img_stride, void *ws, size_t ws_bytes,
                         edvr_stream_t stream);
/* inverse of PixelShuffle(2): x (n, c, 2h, 2w) -> y (n, 4c, h, w) */
int edvr_pixel_unshuffle2_f32(const float *x, float *y, int n, int c, int h, int w, edvr_stream_t stream);
/* the same on dy * act'(y): dz (n, 4c, h, w) = unshuffle(dy (n, c, 2h, 2w) gated by the activation output y of the same shape) - the
 * gradient of PixelShuffle(act(conv(.))) w.r.t. the conv output in one pass (edvr_arch.py:403-404); y may be NULL with EDVR_ACT_NONE */
int edvr_pixel_unshuffle2_act_bwd_f32(const float *dy, const float *y, float *dz, int n, int c, int h, int w, int act, edvr_stream_t stream);
/* z (nc, H, W): z[2oy,2ox] = dz[oy,ox] (dz is (nc, ho, wo)), 0 elsewhere - the stride-2 data gradient is the
 * stride-1 transposed-kernel conv of z */
int edvr_zero_stuff2_f32(const float *dz, float *z, int nc, int H, int W, int ho, int wo, edvr_stream_t stream);
/* dst[b, center, :] += sum_t src[b, t, :]   (src, dst: (b, t, chw)) */
int edvr_frame_reduce_add_f32(const float *src, float *dst, int b, int t, int center, int64_t chw, edvr_stream_t stream);
int edvr_upsample2x_bwd_f32(const float *dy, float *dx, int nc, int h, int w, float scale, edvr_stream_t stream);
int edvr_pool_maxavg_3x3s2_bwd_f32(const float *x, const float *dy, float *dx, int n, int c, int h, int w, edvr_stream_t stream);
/* ws: b*t*hw floats of scratch (two fully parallel passes); NULL = the one-pass kernel, one thread per (clip, pixel) */
int edvr_tsa_temporal_bwd_f32(const float *emb, const float *emb_ref, const float *aligned, const float *dout, float *d_emb,
                              float *d_emb_ref, float *d_aligned, int b, int t, int c, int hw, float *ws, edvr_stream_t stream);
int edvr_tsa_combine_bwd_f32(const float *feat, const float *attn, const float *dy, float *dfeat, float *dattn, int64_t numel,
                             edvr_stream_t stream);
/* CharbonnierLoss, reduction 'sum' (basicsr/models/losses/losses.py:23-25): *loss = sum sqrt((p-t)^2 + eps) and, if dpred != NULL,
 * dpred = grad_scale * (p-t)/sqrt((p-t)^2+eps) in the same pass. */
int edvr_charbonnier_f32(const float *pred, const float *target, float *loss, float *dpred, int64_t numel, float eps,
                         float grad_scale, edvr_stream_t stream);

/* Validation PSNR on the device <- tensor2img (basicsr/utils/img_util.py:36-98) + calculate_psnr (basicsr/metrics/psnr_ssim.py:7-51),
 * which the reference runs per frame on the host after a D2H copy (video_base_model.py:60-98).  a, b: (n, c, h, w) fp32 in RGB
 * channel order, c = 3 or 1.  partial[img * blocks + k] receives the k-th partial sum of squared differences of the two
 * clamp[0,1]-x255-round uint8 images inside the crop (exact integers in double; sum them per image, divide by the element
 * count, PSNR = 20 log10(255 / sqrt(mse))).  y_channel != 0: differences of the Y channel as to_y_channel computes it
 * (metric_util.py:34-47; float32, not rounded), one value per pixel. */
int edvr_psnr_sse_f32(const float *a, const float *b, double *partial, int n, int c, int h, int w, int64_t a_img_stride,
                      int64_t b_img_stride, int crop_border, int y_channel, int blocks, edvr_stream_t stream);

/* Validation SSIM on the device <- tensor2img + calculate_ssim / _ssim (basicsr/metrics/psnr_ssim.py:54-141): per channel, 11x11
 * Gaussian window (sigma 1.5) over the clamp-round-uint8 images in float64, valid region only, mean of the SSIM map.  a, b as
 * for edvr_psnr_sse_f32.  partial[(img * channels + ch) * tiles + k], tiles = edvr_ssim_partials(h, w, crop_border), channels =
 * 1 when y_channel (and c == 3) else c, receives the k-th partial SUM of the SSIM map: add them, divide by
 * (h - 2 crop - 10) * (w - 2 crop - 10), average over channels.  Images without room for one window -> EDVR_ERR_ARG. */
size_t edvr_ssim_partials(int h, int w, int crop_border);
int edvr_ssim_f32(const float *a, const float *b, double *partial, int n, int c, int h, int w, int64_t a_img_stride,
                  int64_t b_img_stride, int crop_border, int y_channel, edvr_stream_t stream);

/* NIQE on the device, the per-pixel part <- tensor2img + calculate_niqe / niqe (basicsr/metrics/niqe.py:10-205, convert_to='y').  The
 * image loses crop_border on every side, then keeps its top-left 96 nbh x 96 nbw pixels; blocks = nbh * nbw = edvr_niqe_blocks(h, w,
 * crop_border) (0: no block fits -> EDVR_ERR_ARG).  Per scale (0: full size, 1: the 2x2 float32 mean) and 96 / 48-pixel block the MSCN
 * map z = (x - mu) / (sigma + 1) is computed in float32 as NumPy computes it (7x7 Gaussian, sigma 7/6, 49 products accumulated in
 * double and rounded once, mode='nearest' at the edge of the KEPT rectangle), and for each of the five maps z, z roll(z,[0,1]),
 * z roll(z,[1,0]), z roll(z,[1,1]), z roll(z,[1,-1]) (float32 products, the roll wraps inside the block) five doubles leave:
 *   out[((img * 2 + scale) * blocks + block) * 25 + map * 5 + k],  k: 0 sum v^2 over v < 0, 1 #(v < 0), 2 sum v^2 over v > 0, 3 #(v > 0),
 *   4 sum |v|;  block = bw * nbh + bh (column-major, the reference's order);  v^2 is the float32 square, the sums run in double in a
 *   fixed order (no atomics: a frame's numbers do not depend on its place in the batch).
 * _f32: x (n, c, h, w) fp32 RGB in [0, 1] (clamped, x255, rounded: tensor2img), c = 3 -> Y of to_y_channel, c = 1 -> the byte itself;
 * _u8: x (n, h, w, 3) RGB bytes.  img_stride in elements, 0 = dense.  One launch: grid (blocks, 2, n). */
size_t edvr_niqe_blocks(int h, int w, int crop_border);
int edvr_niqe_moments_f32(const float *x, double *out, int n, int c, int h, int w, int64_t img_stride, int crop_border, edvr_stream_t stream);
int edvr_niqe_moments_u8(const uint8_t *x, double *out, int n, int h, int w, int64_t img_stride, int crop_border, edvr_stream_t stream);

/* Input pipeline, device side <- imfrombytes(float32=True) (basicsr/utils/img_util.py:101-123: uint8 -> float32 / 255.), augment
 * (basicsr/data/transforms.py:84-151: hflip, then vflip, then transpose, the same state for every image of a clip), img2tensor
 * (img_util.py:9-33: BGR->RGB, HWC->CHW), default collate + CUDAPrefetcher's H2D copy (prefetch_dataloader.py:84-126).
 * src: DEVICE uint8 (n_clips, frames_per_clip, h, w, 3) - decoded and cropped on the host, 1 byte per sample over PCIe;
 * dst: DEVICE float32 (n_clips, frames_per_clip, 3, h', w'), (h', w') = (w, h) under EDVR_AUG_ROT90;
 * clip_flags: HOST array of n_clips bytes (OR of EDVR_AUG_*), or NULL for none (validation: read_img_seq, data_util.py:11-33);
 * it travels in the kernel-argument block, no device allocation or copy.  ROT90 with h != w -> EDVR_ERR_ARG.
 * swap_rb != 0: channel order of src is reversed on the way (src BGR as cv2 decodes -> RGB). */
#define EDVR_AUG_HFLIP 1
#define EDVR_AUG_VFLIP 2
#define EDVR_AUG_ROT90 4
int edvr_frames_u8_to_f32(const uint8_t *src, float *dst, int n_clips, int frames_per_clip, int h, int w,
                          const uint8_t *clip_flags, int swap_rb, edvr_stream_t stream);

/* Whole-video restoration (edvr_amd/video.py): every frame's feature pyramid is computed once and kept in a bank; the window of an
 * output frame (generate_frame_indices, basicsr/data/data_util.py:35-88) is a gather of bank images.
 * One launch, for `levels` (1..EDVR_GATHER_MAX_LEVELS) tensors at once: image j of dst[l] (contiguous, per_img[l] floats per image)
 * = image table[j] of src[l] (src_img_stride[l] floats between images: slices and ring positions of a larger bank work), j < n_out.
 * src / dst / src_img_stride / per_img: HOST arrays of `levels` entries; table: DEVICE int32 array of n_out indices into the n_src
 * images of the sources - stream-ordered, no host synchronisation.  An index outside [0, n_src) is never followed: that destination
 * image is filled with NaN.  16-byte accesses where pointers, stride and image size allow, scalar ones otherwise. */
#define EDVR_GATHER_MAX_LEVELS 3
int edvr_gather_images_f32(const float *const *src, float *const *dst, const int64_t *src_img_stride, const int64_t *per_img, int levels,
                           const int *table, int n_out, int n_src, edvr_stream_t stream);
/* The network's last step with the output in the form it is stored or encoded: out (n, 4h, 4w, 3) uint8, interleaved, =
 * tensor2img (basicsr/utils/img_util.py:36-98: clamp to [0, 1], x 255, round half to even) of y + bilinear x4 of base, y (n, 3, 4h, 4w),
 * base (n, 3, h, w), both contiguous - bit for bit the bytes of the float result of the y += form above. */
int edvr_upsample4x_add_u8(const float *y, const float *base, uint8_t *out, int n, int h, int w, edvr_stream_t stream);
/* out (n, h, w, 3) uint8 = tensor2img of x (n, 3, h, w), x_img_stride floats between images (>= 3 * h * w). */
int edvr_f32_to_u8_hwc(const float *x, uint8_t *out, int n, int h, int w, int64_t x_img_stride, edvr_stream_t stream);

/* Frames of any size (edvr_amd/video.py: pad_mode / tile).  One launch replaces torch.nn.functional.pad(x, (0, Wp - W, 0, Hp - H), mode)
 * of float frames (the reference has no such step: edvr_arch.py:358-366 asserts the size multiple), the slice of a tile out of the padded
 * frames and, for uint8 frames, the byte -> float conversion ahead of both (img_util.py:101-123): dst (n, 3, th, tw) dense float32 =
 * the rectangle at (y0, x0) of the frames extended at the bottom and right, rows >= H / columns >= W by the 'reflect' (2 (n - 1) - j; a
 * rectangle reaching further is EDVR_ERR_ARG) or 'replicate' (n - 1) index rule.  _u8: src (n, H, W, 3) dense bytes, dst = byte / 255
 * exactly as edvr_frames_u8_to_f32 rounds it; _f32: src (n, 3, H, W), dense images src_img_stride floats apart.  16-byte stores where
 * tw % 4 == 0 and dst is aligned, aligned wide loads for groups inside the frame, a scalar path otherwise. */
#define EDVR_PAD_REFLECT 0
#define EDVR_PAD_REPLICATE 1
int edvr_crop_pad_frames_u8(const uint8_t *src, float *dst, int n, int H, int W, int y0, int x0, int th, int tw, int pad_mode,
                            edvr_stream_t stream);
int edvr_crop_pad_frames_f32(const float *src, float *dst, int n, int H, int W, int64_t src_img_stride, int y0, int x0, int th, int tw,
                             int pad_mode, edvr_stream_t stream);
/* The network's last step with a RECTANGLE store: replaces running the whole-tile form and then slicing + copying its result into a
 * full-frame tensor (out[..., oy:oy + kh, ox:ox + kw] = tile_result[..., ky:ky + kh, kx:kx + kw] in ATen).  Pixel (ky + r, kx + q) of what
 * edvr_upsample4x_add_f32 / edvr_upsample4x_add_u8 / edvr_f32_to_u8_hwc would store for y (n, 3, 4h, 4w) + base (n, 3, h, w), both
 * contiguous - or for x (n, 3, h, w), x_img_stride floats between images - goes to (r, q) of dst, r < kh, q < kw, bit for bit.  dst
 * points at the rectangle's first element in the full-frame output; strides in elements of dst: float (n, 3, ., .) destinations have
 * row / plane / image strides, byte (n, ., ., 3) destinations row / image strides.  Wide loads and stores where kx, kw, the pointers
 * and the strides allow, scalar ones otherwise. */
int edvr_upsample4x_add_rect_f32(const float *y, const float *base, float *dst, int n, int h, int w, int ky, int kx, int kh, int kw,
                                 int64_t dst_row_stride, int64_t dst_plane_stride, int64_t dst_img_stride, edvr_stream_t stream);
int edvr_upsample4x_add_rect_u8(const float *y, const float *base, uint8_t *dst, int n, int h, int w, int ky, int kx, int kh, int kw,
                                int64_t dst_row_stride, int64_t dst_img_stride, edvr_stream_t stream);
int edvr_f32_to_u8_hwc_rect(const float *x, uint8_t *dst, int n, int h, int w, int64_t x_img_stride, int ky, int kx, int kh, int kw,
                            int64_t dst_row_stride, int64_t dst_img_stride, edvr_stream_t stream);
int edvr_copy_rect_f32(const float *x, float *dst, int n, int h, int w, int64_t x_img_stride, int ky, int kx, int kh, int kw,
                       int64_t dst_row_stride, int64_t dst_plane_stride, int64_t dst_img_stride, edvr_stream_t stream);

/* Self-ensemble (flip / D4 test-time augmentation; edvr_amd/video.py: self_ensemble).  elem = 4 t + 2 v + h names a symmetry of the
 * square on the last two axes: g(x) = x transposed if t, then rows reversed if v, then columns reversed if h; its inverse applies the
 * same steps in the opposite order.
 * edvr_crop_pad_frames_d4_*: the (th, tw) rectangle edvr_crop_pad_frames_* delivers (the padding rule applied in SOURCE coordinates), as
 * the dense tile g(rectangle): dst (n, 3, th, tw), or (n, 3, tw, th) when t.
 * edvr_*_rect_d4_*: the rectangle tails above storing g^-1 of the tile's result and accumulating over the elements of an ensemble.  y /
 * base / x (and h, w) are in the tile's own, TRANSFORMED orientation and the value of a pixel is the very expression of the plain tail
 * there; (ky, kx, kh, kw) is the kept rectangle of g^-1(result), i.e. in the frame's orientation.  acc: float32 accumulator rectangle
 * (row / plane / image strides in floats); mode: EDVR_D4_FIRST -> acc = value (acc is not read); 0 -> acc = acc + value; EDVR_D4_LAST ->
 * (acc + value) * scale, stored into acc (float tails) or as tensor2img bytes into dst (byte tails: acc is read only, dst is touched by
 * this mode alone); EDVR_D4_FIRST | EDVR_D4_LAST (an ensemble of one) -> value * scale.  Round-to-nearest adds and one multiply, in that
 * order; one writer per pixel and launch, no atomics.  Transposing elements go through a padded 32 x 32 LDS tile, so that reads and
 * stores both run along rows. */
#define EDVR_D4_FIRST 1
#define EDVR_D4_LAST 2
int edvr_crop_pad_frames_d4_u8(const uint8_t *src, float *dst, int n, int H, int W, int y0, int x0, int th, int tw, int pad_mode, int elem,
                               edvr_stream_t stream);
int edvr_crop_pad_frames_d4_f32(const float *src, float *dst, int n, int H, int W, int64_t src_img_stride, int y0, int x0, int th, int tw,
                                int pad_mode, int elem, edvr_stream_t stream);
int edvr_upsample4x_add_rect_d4_f32(const float *y, const float *base, float *acc, int n, int h, int w, int ky, int kx, int kh, int kw,
                                    int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride, int elem, int mode, float scale,
                                    edvr_stream_t stream);
int edvr_upsample4x_add_rect_d4_u8(const float *y, const float *base, float *acc, uint8_t *dst, int n, int h, int w, int ky, int kx, int kh,
                                   int kw, int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride, int64_t dst_row_stride,
                                   int64_t dst_img_stride, int elem, int mode, float scale, edvr_stream_t stream);
int edvr_f32_to_u8_hwc_rect_d4(const float *x, float *acc, uint8_t *dst, int n, int h, int w, int64_t x_img_stride, int ky, int kx, int kh,
                               int kw, int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride, int64_t dst_row_stride,
                               int64_t dst_img_stride, int elem, int mode, float scale, edvr_stream_t stream);
int edvr_copy_rect_d4_f32(const float *x, float *acc, int n, int h, int w, int64_t x_img_stride, int ky, int kx, int kh, int kw,
                          int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride, int elem, int mode, float scale,
                          edvr_stream_t stream);

/* Tile blending (edvr_amd/video.py: tile_blend) - csrc/ensemble.hip.  The four edvr_*_rect_d4_* tails above with a WEIGHT: neighbouring
 * tiles are cross-faded over a band of B output pixels around each cut instead of being cut there.  (ky, kx, kh, kw) is the tile's
 * EXTENDED rectangle (its kept rectangle plus half a band into each neighbour's side); band_y_lo / band_y_hi / band_x_lo / band_x_hi,
 * each 0 or B, say how many of its first / last rows / columns are a band shared with the lower- / higher-index neighbour
 * (band_y_lo + band_y_hi <= kh, band_x_lo + band_x_hi <= kw).  For the j-th pixel (j = 0 ... B - 1, frame's orientation) of a band,
 * r(j) = float(2 j + 1) / float(2 B), the correctly rounded float32 quotient: the higher-index tile (whose LOW band it is) has weight
 * r(j), the lower-index tile (whose HIGH band it is) 1.0f - r(j); outside the bands the weight of an axis is 1.0f; w = w_y * w_x.  All
 * round-to-nearest float32 operations.  With value the float the _d4 tail (element 0: the plain tail) computes for the pixel:
 *   p = w * value, rounded on its own (never fused into the add);
 *   first contributor of the pixel: s = p; every later one: s = acc + p;  last contributor: s * scale is what is stored
 * where "first" = the launch has EDVR_D4_FIRST and the pixel lies in none of the rectangle's low bands, "last" = the launch has
 * EDVR_D4_LAST and the pixel lies in none of its high bands - per pixel, not per launch, so nothing has to be zeroed.  The byte tails
 * store tensor2img bytes into dst for the pixels this launch is last for and the float into acc for all others.  Launches in work-list
 * order (tiles row-major, element innermost) on one stream; one writer per pixel and launch, no atomics.  Without an ensemble: elem 0,
 * mode EDVR_D4_FIRST | EDVR_D4_LAST, scale 1 (a multiply by 1.0f is exact). */
int edvr_upsample4x_add_rect_blend_f32(const float *y, const float *base, float *acc, int n, int h, int w, int ky, int kx, int kh, int kw,
                                       int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride, int elem, int mode, float scale,
                                       int band_y_lo, int band_y_hi, int band_x_lo, int band_x_hi, edvr_stream_t stream);
int edvr_upsample4x_add_rect_blend_u8(const float *y, const float *base, float *acc, uint8_t *dst, int n, int h, int w, int ky, int kx, int kh,
                                      int kw, int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride, int64_t dst_row_stride,
                                      int64_t dst_img_stride, int elem, int mode, float scale, int band_y_lo, int band_y_hi, int band_x_lo,
                                      int band_x_hi, edvr_stream_t stream);
int edvr_f32_to_u8_hwc_rect_blend(const float *x, float *acc, uint8_t *dst, int n, int h, int w, int64_t x_img_stride, int ky, int kx, int kh,
                                  int kw, int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride, int64_t dst_row_stride,
                                  int64_t dst_img_stride, int elem, int mode, float scale, int band_y_lo, int band_y_hi, int band_x_lo,
                                  int band_x_hi, edvr_stream_t stream);
int edvr_copy_rect_blend_f32(const float *x, float *acc, int n, int h, int w, int64_t x_img_stride, int ky, int kx, int kh, int kw,
                             int64_t acc_row_stride, int64_t acc_plane_stride, int64_t acc_img_stride, int elem, int mode, float scale,
                             int band_y_lo, int band_y_hi, int band_x_lo, int band_x_hi, edvr_stream_t stream);

/* MATLAB-style bicubic imresize on the device <- imresize / calculate_weights_indices (basicsr/utils/matlab_functions.py:88-170 and
 * 17-84; the Python statement of scripts/matlab_scripts/generate_bicubic_img.m, i.e. of "BI x4"): one launch resamples n frames by one
 * factor on both axes, rows first, then columns, accumulating in fp32.  Per axis, for the 1-based output x: u = x / scale + 0.5 (1 - 1 /
 * scale), support 4 (4 / scale and kernel scale * cubic(scale * d) when scale < 1 and antialiasing != 0), first tap floor(u - support / 2),
 * ceil(support) + 2 taps of the Keys cubic (a = -0.5), normalised to sum 1; a tap outside the frame reads the symmetric extension
 * (... 1 0 | 0 1 ...).  The weights are computed inside the kernel (per workgroup, in LDS): no table tensors, no allocation, no wait.
 * (ho, wo) = (ceil(H * scale), ceil(W * scale)) are computed by the caller.  1/8 <= scale <= 8; a frame shorter on an axis than the
 * symmetric extension reaches there is EDVR_ERR_ARG, as is n > 65535.
 * _u8: src (n, H, W, 3) dense bytes, each divided by 255 exactly as edvr_frames_u8_to_f32 rounds it; _f32: src (n, 3, H, W), dense images
 * src_img_stride floats apart.  out_kind EDVR_RESIZE_OUT_F32: dst (n, 3, ho, wo) dense float32, NOT clamped (an enlargement overshoots
 * [0, 1], as the reference's does); EDVR_RESIZE_OUT_U8: dst (n, ho, wo, 3) dense bytes = tensor2img (clamp, x 255, round half to even) of
 * that float - bit for bit, and the _u8 source gives bit for bit what the _f32 source holding byte / 255 gives.  16-byte loads where the
 * source rows start on 16-byte boundaries (3 W % 16 == 0 bytes / W % 4 == 0 floats, aligned pointer and stride), 16-byte float and dword
 * byte stores where wo % 4 == 0 and dst is aligned; narrower accesses otherwise. */
#define EDVR_RESIZE_OUT_F32 0
#define EDVR_RESIZE_OUT_U8 1
int edvr_imresize_bicubic_u8(const uint8_t *src, void *dst, int n, int H, int W, int ho, int wo, double scale, int antialiasing,
                             int out_kind, edvr_stream_t stream);
int edvr_imresize_bicubic_f32(const float *src, void *dst, int n, int H, int W, int64_t src_img_stride, int ho, int wo, double scale,
                              int antialiasing, int out_kind, edvr_stream_t stream);

/* Separable resampling of float32 planes to a stated size (csrc/resample.hip; definition: DESIGN 4.21, R1 - R7 - the project's own, no
 * reference): one launch resamples n images of c planes from (H, W) to (Ho, Wo), each axis with its own ratio in [1/8, 8], columns first,
 * then rows.  The taps come from the caller as DEVICE tables (edvr_amd/resample.py: axis_table): fy int32 (Ho) / fx int32 (Wo) - the
 * first tap of every output row / column - and wy float32 (Ho, Ty) / wx float32 (Wo, Tx), its weights, 1 <= T <= 49.  A pass is
 *   out[j] = float32(sum_t double(w[j][t]) * double(in[clamp(first[j] + t, 0, I - 1)])),
 * added in float64 in tap order from 0: the edge sample repeats, nothing else is clamped (Lanczos overshoots), and a result does not
 * depend on the image's place in the batch.  The clamp is the kernel's: whatever the tables hold, no read leaves src.
 * src (n, c, H, W): dense planes, images src_img_stride floats apart, any base alignment; dst (n, c, Ho, Wo) likewise with
 * dst_img_stride (a slice of a longer tensor works on either side).  16-byte loads where the source rows start on 16-byte boundaries
 * (W % 4 == 0, aligned pointer and stride), 16-byte stores where the output rows do; scalar accesses otherwise - the same bits.
 * EDVR_ERR_ARG, nothing launched: a null pointer, n outside 1 ... 65535, c < 1, a T outside 1 ... 49, an axis ratio outside [1/8, 8], an
 * image stride smaller than an image.  No allocation, no wait.
 * edvr_resample_tile: the output tile (toh x tow) a workgroup of that call owns - tow is 64, toh falls from 32 as H / Ho grows toward 8,
 * so that the source rows a tile's vertical taps reach fit 64 KB of LDS with the tables; pure host arithmetic. */
int edvr_resample_tile(int H, int W, int Ho, int Wo, int Ty, int Tx, int *toh, int *tow);
int edvr_resample_f32(const float *src, float *dst, int n, int c, int H, int W, int64_t src_img_stride, int Ho, int Wo,
                      int64_t dst_img_stride, const int32_t *fy, const float *wy, int Ty, const int32_t *fx, const float *wx, int Tx,
                      edvr_stream_t stream);

/* "BD" downsampling on the device <- duf_downsample / generate_gaussian_kernel (basicsr/data/data_util.py:281-331; the LQ frames of
 * VideoTestDUFDataset, video_test_dataset.py:231-290): DUF's 13 x 13 Gaussian blur, sigma = 0.4 * scale, sampled at every scale-th
 * input sample, as ONE launch.  For scale s in {2, 3, 4}:
 *   out[i, j] = sum_{a, b = 0..12} g[a] g[b] x[R(i s - 6 + a, H), R(j s - 6 + b, W)],  R(p, n) = -p (p < 0), 2 (n - 1) - p (p >= n), p:
 * the reflection that does not repeat the edge sample (F.pad 'reflect'); taps are centred on input sample i * s.  g is the 1-D kernel of
 * scipy.ndimage.gaussian_filter at sigma: exp(-d^2 / 2 sigma^2) / sum for |d| <= int(4 sigma + 0.5) (3, 5, 6), 0 beyond - its outer
 * product is the reference's 2-D filter exactly.  The 13 weights are computed on the host in float64 and passed as kernel arguments;
 * rows first, then columns, fp32 accumulation: no allocation, no wait.  (ho, wo) = (ceil(H / s), ceil(W / s)), computed by the caller
 * (the reference pads by 6 + 2 s and crops two outputs per side: the same samples).  EDVR_ERR_ARG for a scale outside {2, 3, 4}, for
 * min(H, W) < 7 (one reflection must cover the reach of 6; the reference needs min(H, W) > 6 + 2 s), for other (ho, wo), n > 65535.
 * _u8: src (n, H, W, 3) dense bytes, each divided by 255 exactly as edvr_frames_u8_to_f32 rounds it; _f32: src (n, 3, H, W), dense images
 * src_img_stride floats apart.  out_u8 == 0: dst (n, 3, ho, wo) dense float32, not clamped; != 0: dst (n, ho, wo, 3) dense bytes =
 * tensor2img (clamp, x 255, round half to even) of that float - bit for bit, and the _u8 source gives bit for bit what the _f32 source
 * holding byte / 255 gives.  16-byte loads where the source rows start on 16-byte boundaries (3 W % 16 == 0 bytes / W % 4 == 0 floats,
 * aligned pointer and stride), 16-byte float and dword byte stores where wo % 4 == 0 and dst is aligned; narrower accesses otherwise. */
int edvr_bd_downsample_u8(const uint8_t *src, void *dst, int n, int H, int W, int ho, int wo, int scale, int out_u8, edvr_stream_t stream);
int edvr_bd_downsample_f32(const float *src, void *dst, int n, int H, int W, int64_t src_img_stride, int ho, int wo, int scale, int out_u8,
                           edvr_stream_t stream);

/* The two degradations above for TRAINING crops: per image a p x p crop of the x`scale` LQ frame, made from a WINDOW of the GT frame -
 * the GT samples the crop's taps read with non-zero weight once the frame's boundary rule has folded out-of-frame taps back in
 * (edvr_amd/data.py: lq_window).  src: n dense windows of wh rows of `pitch` bytes (pitch % 16 == 0, pitch >= 3 ww, src 16-byte
 * aligned: every row takes the 16-byte load path), ww interleaved RGB pixels per row; wh = ww = the fixed extent lq_window gives for
 * (p, scale, degradation).  table: DEVICE array of n records of EDVR_LQ_WINDOW_RECORD_INTS int32: { y0, x0: the window's origin in its
 * frame; H, W: the (mod-cropped) GT frame; top, left: the crop's origin in the LQ frame; 2 unused }.  dst (n, p, p, 3) bytes: exactly
 * the bytes edvr_imresize_bicubic_u8 (scale 1 / `scale`, antialiasing, EDVR_RESIZE_OUT_U8) / edvr_bd_downsample_u8 (out_u8) give at
 * [top, top + p) x [left, left + p) of the whole frame - by construction: weights are a function of the absolute output index, the
 * boundary rule is applied in frame coordinates and then mapped into the window, and the passes are the full-frame kernels' own code.
 * A tap of weight zero outside the window is clamped into it; whatever the table holds, no read leaves src and no write leaves dst.
 * EDVR_ERR_ARG, nothing launched: scale outside {2, 3, 4}; wh or ww other than that extent; a pitch or src off 16 bytes; and, when
 * table_host (a host copy of the table, or NULL) is given, any record whose frame, crop or window the geometry refuses.  No
 * allocation, no wait. */
#define EDVR_LQ_WINDOW_RECORD_INTS 8
int edvr_imresize_bicubic_u8_windows(const uint8_t *src, const int32_t *table, const int32_t *table_host, uint8_t *dst, int n, int p, int wh,
                                     int ww, int pitch, int scale, edvr_stream_t stream);
int edvr_bd_downsample_u8_windows(const uint8_t *src, const int32_t *table, const int32_t *table_host, uint8_t *dst, int n, int p, int wh, int ww,
                                  int pitch, int scale, edvr_stream_t stream);

/* Planar Y'CbCr of any Y4M format <-> RGB (csrc/yuv.hip, one kernel family; definition: DESIGN 4.11, depths and subsamplings: 4.14).
 * A format is a chroma subsampling (sub_x, sub_y) - (1, 1) 4:2:0, (1, 0) 4:2:2, (0, 0) 4:4:4 - and a bit depth 8 ... 16.  A frame of
 * (H, W) is the dense planes Y (H, W), Cb, Cr (Hc, Wc) = ((H + sub_y) >> sub_y, (W + sub_x) >> sub_x) - the payload of a YUV4MPEG2
 * frame; a sample is one byte at depth 8, otherwise one little-endian 16-bit word (bits above the depth are NOT masked by the decode).
 * A batch is n frames yuv_stride >= framesize BYTES apart at ANY base address and stride (a Y4M read buffer: framesize + 6 apart, 6 past
 * its start); with 16-bit samples the base address and yuv_stride are even.  Odd H and W are legal.
 * coef: 12 HOST floats read before the call returns - a 3 x 3 matrix row-major, then the offsets (yoff, coff, coff): for the decode the
 * INVERSE of the forward matrix M, for the encode M itself (RGB in 0 ... 255 -> Y, Cb, Cr), computed in float64 and scaled for the depth
 * by the caller (ops.yuv_coeffs(matrix, range, depth)) and rounded.  All arithmetic float32, every product and sum rounded on its own
 * in the order of DESIGN 4.11 (no contraction).
 * yuv_to_rgb: chroma upsampled along the subsampled axes by replication (bilinear == 0) or by the centre-sited 1/4 - 3/4 filter, vertical
 * then horizontal, indices clamped to the plane; v = Mi (Y - yoff, Cb - coff, Cr - coff); _f32: rgb (n, 3, H, W), dense images
 * rgb_img_stride floats apart, clamp(v, 0, 255) / 255.0f; _u8: rgb (n, H, W, 3) dense bytes, clamp and round half to even.
 * rgb_to_yuv: _f32 reads x = clamp(f, 0, 1) * 255.0f (NaN -> 0), _u8 the byte; p = M x + off; a chroma sample is the mean of p over its
 * 2 x 2 block (4:2:0), over its pair of columns (4:2:2: (p[2l] + p[2l + 1]) * 0.5f) or p itself (4:4:4), row and column indices clamped
 * to the frame (an odd edge replicates); every sample is clamped to [0, 2^depth - 1] and rounded half to even.  Bytes between the frames
 * of the output batch are not written.
 * The yuv420 four are the same functions at (sub_x, sub_y, depth) = (1, 1, 8) - an I420 frame: H W luma bytes, then Hc Wc bytes of Cb,
 * then of Cr, Hc = ceil(H / 2), Wc = ceil(W / 2); uint8 RGB exists for this format alone.
 * 16-byte accesses on a side whose base and strides are 16-byte aligned where W % 16 == 0, scalar ones otherwise; same values either way.
 * EDVR_ERR_ARG: null pointers, n, H or W < 1, depth outside 8 ... 16, a subsampling other than the three, yuv_stride < framesize or
 * rgb_img_stride < 3 H W with n > 1, an odd base or stride with 16-bit samples, H W > 2^29.  No allocation, no wait. */
int edvr_yuv420_to_rgb_f32(const uint8_t *yuv, float *rgb, int n, int H, int W, int64_t yuv_stride, int64_t rgb_img_stride, const float *coef,
                           int bilinear, edvr_stream_t stream);
int edvr_yuv420_to_rgb_u8(const uint8_t *yuv, uint8_t *rgb, int n, int H, int W, int64_t yuv_stride, const float *coef, int bilinear,
                          edvr_stream_t stream);
int edvr_rgb_to_yuv420_f32(const float *rgb, uint8_t *yuv, int n, int H, int W, int64_t rgb_img_stride, int64_t yuv_stride, const float *coef,
                           edvr_stream_t stream);
int edvr_rgb_to_yuv420_u8(const uint8_t *rgb, uint8_t *yuv, int n, int H, int W, int64_t yuv_stride, const float *coef, edvr_stream_t stream);
int edvr_yuv_to_rgb_f32(const uint8_t *yuv, float *rgb, int n, int H, int W, int sub_x, int sub_y, int depth, int64_t yuv_stride,
                        int64_t rgb_img_stride, const float *coef, int bilinear, edvr_stream_t stream);
int edvr_rgb_to_yuv_f32(const float *rgb, uint8_t *yuv, int n, int H, int W, int sub_x, int sub_y, int depth, int64_t rgb_img_stride,
                        int64_t yuv_stride, const float *coef, edvr_stream_t stream);

/* The same conversions with a chroma siting per axis (definition: DESIGN 4.15): siting_x / siting_y = 0 centre (chroma sample k lies
 * between luma samples 2k and 2k + 1: JPEG / MPEG-1, and what the functions above compute - each of them is its _sited form at (0, 0)) or
 * 1 co-sited (sample k lies ON luma sample 2k).  (1, 0) is 'left' - H.264 / HEVC / AV1 4:2:0 by default, every 4:2:2; (1, 1) is 'topleft' -
 * BT.2020 / UHD.  An axis that is not subsampled ignores its value, and so does a decode with bilinear == 0.
 * Decode, co-sited axis: even 2k takes c[k], odd 2k + 1 takes 0.5 c[k] + 0.5 c[k + 1] (vertical, then horizontal, indices clamped).
 * Encode, co-sited axis: [1 2 1] / 4 around luma sample 2k over the values p before quantisation - horizontally (p[2l - 1] + p[2l + 1]) +
 * (p[2l] + p[2l]) (a centred axis: p[2l] + p[2l + 1]), then the same over those sums vertically, then one product with the reciprocal of
 * the weights' sum; indices clamped to the frame.  The horizontal halo column and the row above a row pair are recomputed from RGB.
 * EDVR_ERR_ARG as above, and for a siting other than 0 / 1 or (0, 1) (co-sited rows under centred columns: no standard's siting). */
int edvr_yuv_to_rgb_sited_f32(const uint8_t *yuv, float *rgb, int n, int H, int W, int sub_x, int sub_y, int depth, int64_t yuv_stride,
                              int64_t rgb_img_stride, const float *coef, int bilinear, int siting_x, int siting_y, edvr_stream_t stream);
int edvr_rgb_to_yuv_sited_f32(const float *rgb, uint8_t *yuv, int n, int H, int W, int sub_x, int sub_y, int depth, int64_t rgb_img_stride,
                              int64_t yuv_stride, const float *coef, int siting_x, int siting_y, edvr_stream_t stream);
int edvr_yuv420_to_rgb_sited_u8(const uint8_t *yuv, uint8_t *rgb, int n, int H, int W, int64_t yuv_stride, const float *coef, int bilinear,
                                int siting_x, int siting_y, edvr_stream_t stream);
int edvr_rgb_to_yuv420_sited_u8(const uint8_t *rgb, uint8_t *yuv, int n, int H, int W, int64_t yuv_stride, const float *coef, int siting_x,
                                int siting_y, edvr_stream_t stream);

/* Deinterlacing of interlaced planar Y'CbCr frames (csrc/deint.hip; definition: DESIGN 4.19, D1 - D6).  Replaces nothing in the
 * reference, which restores progressive frames only: it is the `ffmpeg -vf yadif` pass otherwise run in front of the pipe, done on the
 * device, on the samples as decoded, at field rate.  No bit-compatibility with any other deinterlacer is claimed.
 * yuv: n frames of the format (sub_x, sub_y, depth) described above, in_stride BYTES apart at any base address (both even for 16-bit
 * samples); each holds two fields, on its even and odd rows - in every plane alike - of which the top one (even rows) is the earlier in
 * time unless bottom_first.  Field k = 0 ... 2 n - 1 lives in frame k / 2.  out: field_rate != 0: 2 n frames, frame k built from field k
 * (its rows copied, the others predicted along the least-different of five edge directions between the rows above and below and clamped
 * to a band around the mean of the fields before and after, integers throughout); field_rate == 0: n frames, from the even k.  Output
 * frames lie out_stride bytes apart, any base address (even for 16-bit samples); bytes between them are not written.
 * prev / next: ONE dense frame each, the one before / after the batch, or NULL: fields -2, -1 and 2 n, 2 n + 1 are read from them, so a
 * batch cut from a longer video gets what the whole video would give; on a side without one the field index reflects about the batch's
 * end.  Rows reflect about the plane's first and last row, columns clamp.  Odd H and W are legal.  out must not overlap the inputs.
 * One launch, (lanes of 8 samples, output frames); whole-segment accesses of any alignment inside a row, sample by sample at its ends.
 * EDVR_ERR_ARG: null yuv / out, n < 1 or > 32767, W < 1, H < 4 (every plane needs two rows), depth outside 8 ... 16, a subsampling other
 * than the three, a stride shorter than a frame where more than one is read / written, an odd pointer or stride with 16-bit samples,
 * H W > 2^29, bottom_first / field_rate other than 0 / 1.  No allocation, no wait. */
int edvr_deinterlace(const uint8_t *yuv, const uint8_t *prev, const uint8_t *next, uint8_t *out, int n, int H, int W, int sub_x, int sub_y,
                     int depth, int64_t in_stride, int64_t out_stride, int bottom_first, int field_rate, edvr_stream_t stream);

/* Inverse telecine (csrc/telecine.hip; definition: DESIGN 4.20, T1 - T9, integers only).  Replaces nothing in the reference: it is the
 * `ffmpeg -vf fieldmatch,decimate` pass otherwise run in front of the pipe.  No bit-compatibility with those filters or TIVTC is claimed.
 * Frames are as edvr_deinterlace takes them: n frames of the format (sub_x, sub_y, depth), in_stride BYTES apart at any base address
 * (both even for 16-bit samples); bottom_first: the odd rows are the earlier field; q = bottom_first is the row parity of the first field.
 *
 * edvr_field_match: the metrics.  table: int64 (n, 7), row i = S_c, S_p, mic_c, mic_p, A, B, C of frame i, from LUMA alone (R = H rows):
 *   W_c = L_i; W_p = the rows of parity q of L_i and the other rows of L_(i-1) (W_c where frame i - 1 does not exist);
 *   comb k at 1 <= y <= R - 2: d1 = W[y] - W[y-1], d2 = W[y] - W[y+1], k = min(|d1|, |d2|) where both are > 0 or both < 0, else 0;
 *   S = sum of max(k - (nt << (depth - 8)), 0); mic = the largest count of k > (ct << (depth - 8)) in a 16 x 16 block anchored at (0, 0);
 *   A = sum |L_i - L_(i-1)| over the rows of parity q, B over the other rows, C = sum |L_i - L_(i-2)| over the other rows; 0 where the
 *   earlier frame does not exist.  prev / prev2: frame -1 / frame -2, ONE dense frame each, or NULL.
 * Exact 64-bit integers: a row does not depend on the batch it was computed in.  TWO operations on the stream: a clear of the table
 * (hipMemsetAsync) and ONE kernel launch, grid (strips of 16 rows, workgroups per strip, n); a workgroup ends with one 64-bit integer
 * atomic add per non-zero sum and one integer atomic max per non-zero mic.
 * EDVR_ERR_ARG: null yuv / table, n < 1 or > 32767, W < 1, H < 4, depth outside 8 ... 16, a subsampling other than the three, a stride
 * shorter than a frame with n > 1, an odd pointer or stride with 16-bit samples, H W > 2^29, bottom_first other than 0 / 1, nt or ct
 * outside 0 ... 255.  No allocation, no wait.
 *
 * edvr_field_weave: T9's weave, ONE launch for n_out output frames, all three planes.  table: int32 (n_out, 2) ON THE DEVICE, row j =
 * (input frame index s in [0, n), match: 0 = c, 1 = p).  Output frame j takes its rows of parity q from frame s and its other rows from
 * frame s (c) or frame s - 1 (p; frame -1 is `prev`, one dense frame or NULL).  A row whose source does not exist (s outside [0, n), p at
 * s = 0 without prev) is not written.  Output frames lie out_stride bytes apart at any base address; bytes between them are not written.
 * out must not overlap the inputs.  A lane moves 16 bytes of a row, whole where they lie inside it, byte by byte at its end.
 * EDVR_ERR_ARG: null yuv / out / table, n or n_out < 1 or > 32767, and the size / format / stride conditions above. */
int edvr_field_match(const uint8_t *yuv, const uint8_t *prev, const uint8_t *prev2, int64_t *table, int n, int H, int W, int sub_x, int sub_y,
                     int depth, int64_t in_stride, int bottom_first, int nt, int ct, edvr_stream_t stream);
int edvr_field_weave(const uint8_t *yuv, const uint8_t *prev, uint8_t *out, const int32_t *table, int n, int n_out, int H, int W, int sub_x,
                     int sub_y, int depth, int64_t in_stride, int64_t out_stride, int bottom_first, edvr_stream_t stream);

/* Letterbox / pillarbox bars (csrc/bars.hip; definition: DESIGN 4.22, B1 - B7, integers only).  Replaces nothing in the reference: it is the
 * `ffmpeg -vf cropdetect,crop` pass otherwise run in front of the pipe.  No bit-compatibility with cropdetect is claimed.  Frames are as
 * edvr_field_match takes them: n frames of the format (sub_x, sub_y, depth), in_stride BYTES apart at any base address (both even for
 * 16-bit samples).
 *
 * edvr_bar_profile: B1.  table: int64 (n, H + W), row i = the H row sums P_i[y] = sum over x of L_i[y, x] and then the W column sums
 * Q_i[x] = sum over y of L_i[y, x] of frame i's LUMA plane L_i, samples as integers.  ONE kernel launch for all n frames behind a
 * hipMemsetAsync of the table; every luma sample is read once and reduced along both axes in that pass; 64-bit integer atomics carry the
 * totals, so a row does not depend on the batch it was computed in.  EDVR_ERR_ARG: null yuv / table, n < 1 or > 32767, H or W < 1, a
 * depth outside 8 ... 16, a subsampling other than (1, 1), (1, 0), (0, 0), in_stride shorter than a frame with n > 1, an odd pointer or
 * stride with 16-bit samples, H W > 2^29.  No allocation, no wait.
 *
 * edvr_yuv_crop: B7, ONE launch for all n frames, all three planes: output frame i is the luma rect (y0, x0, h, w) of input frame i and the
 * chroma rects (y0 >> sub_y, x0 >> sub_x, h >> sub_y, w >> sub_x), in the layout of an h x w frame of the format; output frames lie
 * out_stride bytes apart at any base address, bytes between them are not written.  out must not overlap the input.  A lane moves 16 bytes
 * of an output row, whole where they lie inside it, byte by byte at its end; source rows start at any byte offset.  EDVR_ERR_ARG: null
 * yuv / out, a rect that is empty, leaves the frame or is off the chroma steps (y0, h multiples of 1 << sub_y; x0, w of 1 << sub_x), an
 * out_stride shorter than an h x w frame with n > 1, and the size / format / stride conditions above. */
int edvr_bar_profile(const uint8_t *yuv, int64_t *table, int n, int H, int W, int sub_x, int sub_y, int depth, int64_t in_stride,
                     edvr_stream_t stream);
int edvr_yuv_crop(const uint8_t *yuv, uint8_t *out, int n, int H, int W, int sub_x, int sub_y, int depth, int64_t in_stride, int64_t out_stride,
                  int y0, int x0, int h, int w, edvr_stream_t stream);

/* Frame-to-frame change for scene-cut detection (csrc/shots.hip; definition: DESIGN 4.13).  The bytes R, G, B of a pixel are the input's
 * own (_u8: x (n, H, W, 3)) or its tensor2img bytes (_f32: x (n, 3, H, W); clamp to [0, 1], x 255, round half to even, NaN -> 0); in
 * integers Y8 = ((66 R + 129 G + 25 B + 128) >> 8) + 16, and
 *   sad[j] = sum over the H W pixels of |Y8 of frame j - Y8 of frame j - 1| for j >= 1;  sad[0] the same against the frame `prev` (one
 *   dense frame of x's type, e.g. the last one of the batch before), or 0 where prev == NULL.
 * Exact 64-bit integers (at most 219 H W): a pair's number does not depend on the batch it was computed in.  Each frame is dense; the
 * frames of the batch lie img_stride ELEMENTS (bytes / floats) apart at any base address, 0 = dense.  16-byte loads where x, prev and
 * the stride in bytes are multiples of 16 (_f32: and H W of 4), single bytes / floats otherwise; same values either way.  ONE kernel
 * launch, grid (blocks per frame, pairs), behind a clear of sad[0 ... n) on the same stream; one 64-bit integer atomic add per block.
 * EDVR_ERR_ARG: x or sad NULL, n, H or W < 1, H W > 2^31 - 1, 0 < img_stride < 3 H W with n > 1.  No allocation, no wait. */
int edvr_frame_sad_rgb_u8(const uint8_t *x, const uint8_t *prev, uint64_t *sad, int n, int H, int W, int64_t img_stride, edvr_stream_t stream);
int edvr_frame_sad_rgb_f32(const float *x, const float *prev, uint64_t *sad, int n, int H, int W, int64_t img_stride, edvr_stream_t stream);

/* Baseline JPEG round trip (csrc/jpeg.hip; definition: DESIGN 4.16): dst = what a baseline JPEG encoder at `quality` followed by a decoder
 * returns for src - libjpeg's integer pipeline (colour conversion, edge padding to the MCU, 2 x 2 chroma mean with alternating bias, 13-bit
 * Loeffler DCT, Annex K tables scaled by the quality, inverse DCT, triangle-filter chroma upsampling), byte for byte; entropy coding is
 * lossless and is not performed.  src, dst: n dense (H, W, 3) RGB byte images src_image_stride / dst_image_stride BYTES apart at any base
 * address (0 = dense; a slice of a longer batch works); the two must not overlap (a workgroup reads pixels of its neighbours' tiles).
 * quality: a DEVICE table of n int32, each clamped to 0 ... 100 by the kernel, or NULL: quality_all, 0 ... 100, for every image.  A
 * quality of 0 copies that image through unchanged.  subsampling: EDVR_JPEG_420 (16 x 16 MCUs) or EDVR_JPEG_444 (8 x 8).
 * ONE kernel launch, grid (64 x 64 pixel tiles, n); dword accesses on a side whose base and stride are multiples of 4 where W % 4 == 0,
 * bytes otherwise; same values either way.  EDVR_ERR_ARG: null src / dst, n outside 1 ... 65535, H or W < 1, H W > 2^29, a subsampling
 * other than the two, quality_all outside 0 ... 100 with a NULL table, an image stride shorter than 3 H W with n > 1.  No allocation, no
 * wait, capturable in a graph. */
#define EDVR_JPEG_444 444
#define EDVR_JPEG_420 420
int edvr_jpeg_roundtrip_u8(const uint8_t *src, uint8_t *dst, const int32_t *quality, int quality_all, int n, int H, int W,
                           int64_t src_image_stride, int64_t dst_image_stride, int subsampling, edvr_stream_t stream);

/* MPEG-style round trip (csrc/mpeg.hip; definition: DESIGN 4.18, M1 - M7): dst = what an I / P video encoder at `qscale` followed by a
 * decoder returns for b clips of t frames in display order - the planes, 13-bit DCT and colour steps of the JPEG round trip above for
 * 4:2:0; frame i is intra (MPEG-2 default intra matrix scaled by qscale) if i == 0 or gop > 0 and i % gop == 0, else predicted from the
 * reconstruction of frame i - 1: per 16 x 16 macroblock a full search over [-search, search]^2 (SAD + qscale (|dy| + |dx|), ties to the
 * first candidate in raster order, reads clamped to the padded plane), a half-sample chroma vector, a flat dead-zone quantiser on the
 * residual.  Entropy coding is not performed and no stream compatibility is claimed.  src, dst: dense (H, W, 3) RGB byte frames,
 * *_frame_stride BYTES apart within a clip and *_clip_stride between clips - at least a frame and at least a clip, (t - 1) frame strides
 * and a frame, so that no two frames share a byte - at any base address (0 = dense); src and dst must not overlap.
 * qscale: a DEVICE table of b int32, each clamped to 0 ... 31 by the kernels, or NULL: qscale_all, 0 ... 31, for every clip; 0 copies that
 * clip through unchanged.  ws: edvr_mpeg_roundtrip_workspace(b, t, H, W) bytes, 4-byte aligned (source and reconstructed planes of every
 * frame: 2 b t 1.5 Hp Wp, Hp = 16 ceil(H / 16), Wp likewise); 0 for sizes the entry point rejects.  t + 2 kernel launches.
 * EDVR_ERR_ARG: null src / dst, b, t, H or W < 1, b t > 65535, H or W > 16384, gop < 0, search outside 0 ... 15, qscale_all outside
 * 0 ... 31 with a NULL table, a frame stride shorter than 3 H W or a clip stride shorter than a clip, a workspace too small or misaligned.  No allocation, no wait. */
size_t edvr_mpeg_roundtrip_workspace(int b, int t, int H, int W);
int edvr_mpeg_roundtrip_u8(const uint8_t *src, uint8_t *dst, const int32_t *qscale, int qscale_all, int b, int t, int H, int W,
                           int64_t src_clip_stride, int64_t src_frame_stride, int64_t dst_clip_stride, int64_t dst_frame_stride, int gop,
                           int search, void *ws, size_t ws_bytes, edvr_stream_t stream);

/* Blur and noise degradations (csrc/degrade.hip; definition: DESIGN 4.17): the steps of the first-order degradation model that come before
 * compression, in ONE launch.  src, dst: n dense (H, W, 3) RGB byte images src_image_stride / dst_image_stride BYTES apart at any base
 * address (0 = dense; a slice of a longer batch works); the two must not overlap (a workgroup reads pixels of its neighbours' tiles).
 * table: DEVICE array of n records of EDVR_DEGRADE_RECORD_INTS int32 { ksize, weight_offset, read_bits, shot_bits, flags, key_lo, key_hi,
 * ctr_t }.  Blur: ksize 0 (none) or odd 3 ... EDVR_DEGRADE_MAX_KSIZE, the image's ksize x ksize Q20 weights (each 0 ... 2^20, summing to
 * 2^20) at weights[weight_offset ...]; acc = sum of weight x sample over the frame extended by the reflection that does not repeat the
 * edge sample (H, W > ksize / 2), exact in 32-bit integers; acc = src << 20 at ksize 0.  Noise: read_bits / shot_bits are the float32 bit
 * patterns of the read noise's sigma (levels) and the shot noise's variance per level; both +0.0: dst = (acc + 2^19) >> 20.  Otherwise v =
 * float(acc) 2^-20, s = sqrt(shot v + read^2), dst = clamp(floor(v + s z + 0.5), 0, 255) with z standard normal: one Philox4x32-10 call per
 * pixel, counter (x, y, ctr_t, 0), key (key_lo, key_hi), words r0 ... r3 -> Box-Muller pairs (r0, r1) -> z_R = rho cos phi, z_G = rho sin phi
 * and (r2, r3) -> z_B = rho cos phi, rho = sqrt(-2 ln(((r >> 8) + 0.5) 2^-24)), phi = 2 pi (r' >> 8) 2^-24, float32; flags &
 * EDVR_DEGRADE_GRAY: all three channels take z_R.  (x, y) are the coordinates in the image handed in.  weights may be NULL where no
 * record blurs; the kernel treats any other ksize as 0 and clamps a weight to 0 ... 2^20, but trusts weight_offset: the caller checks its
 * records (edvr_amd/ops.py does, on the host copy).  Grid (EDVR_DEGRADE_TILE^2 pixel tiles, n); dword accesses on a side whose base and
 * stride are multiples of 4 where W % 4 == 0, bytes otherwise; same values either way.  EDVR_ERR_ARG: null src / dst / table, n outside
 * 1 ... 65535, H or W < 1, H W > 2^29, an image stride shorter than 3 H W with n > 1.  No allocation, no wait, capturable in a graph. */
#define EDVR_DEGRADE_TILE 64
#define EDVR_DEGRADE_MAX_KSIZE 21
#define EDVR_DEGRADE_RECORD_INTS 8
#define EDVR_DEGRADE_GRAY 1
int edvr_degrade_u8(const uint8_t *src, uint8_t *dst, const int32_t *table, const int32_t *weights, int n, int H, int W,
                    int64_t src_image_stride, int64_t dst_image_stride, edvr_stream_t stream);
/* The generator of edvr_degrade_u8 on its own: dst (H, W, 4) uint32, 16-byte aligned = the four words of Philox4x32-10 at
 * counter (x, y, ctr_t, 0) and key (key_lo, key_hi) - multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85, as
 * Random123 defines it.  EDVR_ERR_ARG: null or misaligned dst, H or W < 1, H W > 2^29. */
int edvr_philox_words_u32(uint32_t *dst, uint32_t key_lo, uint32_t key_hi, uint32_t ctr_t, int H, int W, edvr_stream_t stream);

/* Multi-tensor Adam step <- torch.optim.Adam.step() as the reference builds it (basicsr/models/edvr_model.py:21-53, parameter
 * groups with dcn_lr_mul; stepped in sr_model.py:112).  `chunk_table` is a DEVICE array of n_chunks records of
 * edvr_adam_chunk_bytes() = 64 bytes: { float *p; const float *g; float *m; float *v; int32 n (<= 65536 elements of one tensor);
 * float lr; float weight_decay; float 1/(1-beta1^t); float 1/sqrt(1-beta2^t); 12 bytes padding }.  One launch updates every
 * tensor of every group; arithmetic of torch.optim.Adam (amsgrad = False, maximize = False). */
size_t edvr_adam_chunk_bytes(void);
int edvr_adam_multi_f32(const void *chunk_table, int n_chunks, float beta1, float beta2, float eps, edvr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EDVR_AMD_H */
