"""ctypes binding of libedvr_amd.so (include/edvr_amd.h).

The library is the product: there is no Python/CPU fallback.  If it cannot be
loaded, every op raises - loudly - instead of silently running something else.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('EDVR_AMD_LIB') or os.path.join(_HERE, 'lib', 'libedvr_amd.so')  # env: A/B kernel variants

c_float_p = ctypes.c_void_p
i32, i64, f32, sz, u32 = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t, ctypes.c_uint32
vp = ctypes.c_void_p


class ConvDesc(ctypes.Structure):
    """Mirror of `edvr_conv2d_desc` (include/edvr_amd.h)."""
    _fields_ = [
        ('x1', vp), ('x2', vp), ('c1', i32), ('c2', i32), ('x1_img_stride', i64), ('x2_img_stride', i64),
        ('x2_div', i32), ('x2_mul', i32), ('x2_add', i32), ('n', i32), ('h', i32), ('w', i32), ('wpk', vp),
        ('bias', vp), ('co', i32), ('ks', i32), ('stride', i32), ('act', i32), ('act_from', i32), ('res1', vp),
        ('res2', vp), ('res1_img_stride', i64), ('res2_img_stride', i64), ('y', vp), ('y_img_stride', i64),
        ('out_mode', i32), ('algo', i32), ('gate', vp), ('gate_img_stride', i64), ('gate_slope', f32), ('y_scale', f32),
        ('wpk_f4', vp), ('abs_sum', vp), ('abs_sum_channels', i32), ('wpk_f4s', vp), ('x_amax', vp), ('y_amax', vp),
        ('pre', vp), ('pre_img_stride', i64), ('pre_div', i32), ('pre_mul', i32), ('pre_add', i32), ('pre_n', i32), ('wpk_ds', vp),
    ]


# name -> (restype, argtypes); every symbol include/edvr_amd.h declares
PROTOTYPES = {
    'edvr_version': (ctypes.c_char_p, []),
    'edvr_last_error': (ctypes.c_char_p, []),
    'edvr_check_device': (i32, []),
    'edvr_conv2d_packed_weight_elems': (sz, [i32, i32, i32]),
    'edvr_conv2d_pack_weight_f32': (i32, [vp, vp, i32, i32, i32, i32, vp]),
    'edvr_conv2d_packed_weight_f4_elems': (sz, [i32, i32]),
    'edvr_conv2d_pack_weight_f4_f32': (i32, [vp, vp, i32, i32, i32, vp]),
    'edvr_conv2d_packed_weight_f4s_elems': (sz, [i32, i32]),
    'edvr_conv2d_pack_weight_f4s_f32': (i32, [vp, vp, i32, i32, i32, vp]),
    'edvr_conv2d_packed_weight_1x1s_elems': (sz, [i32, i32]),
    'edvr_conv2d_pack_weight_1x1s_f32': (i32, [vp, vp, i32, i32, vp]),
    'edvr_conv2d_packed_weight_ds_elems': (sz, [i32, i32, i32]),
    'edvr_conv2d_pack_weight_ds_f32': (i32, [vp, vp, i32, i32, i32, vp]),
    'edvr_amax_f32': (i32, [vp, vp, i32, i64, i64, vp]),
    'edvr_pack_job_bytes': (sz, []),
    'edvr_conv2d_pack_weights_multi': (i32, [vp, i32, i32, i32, vp]),
    'edvr_conv2d_f32': (i32, [ctypes.POINTER(ConvDesc), vp]),
    'edvr_conv2d_kernel': (i32, [ctypes.POINTER(ConvDesc)]),
    'edvr_conv2d_gate_supported': (i32, [ctypes.POINTER(ConvDesc)]),
    'edvr_conv2d_abs_sum_supported': (i32, [ctypes.POINTER(ConvDesc)]),
    'edvr_conv2d_y_amax_supported': (i32, [ctypes.POINTER(ConvDesc)]),
    'edvr_conv2d_pre_supported': (i32, [ctypes.POINTER(ConvDesc)]),
    'edvr_conv2d_f4s_set_lean': (i32, [i32]),
    'edvr_conv2d_f4s_lean_items': (i32, [ctypes.POINTER(ConvDesc)]),
    'edvr_conv2d_kernel_name': (i32, [ctypes.POINTER(ConvDesc), ctypes.c_char_p, sz]),
    'edvr_conv2d_executed_flops': (i32, [ctypes.POINTER(ConvDesc), ctypes.POINTER(ctypes.c_double)]),
    'edvr_dcnv2_fwd_ws_bytes': (sz, [i32] * 12),
    'edvr_dcnv2_fwd_f32': (i32, [vp] * 6 + [i32] * 12 + [i64, i64, i32, i32, vp, sz, vp]),
    'edvr_dcnv2_fwd_split_f32': (i32, [vp] * 6 + [i32] * 12 + [i64, i64, i32, i32, vp, sz, vp, vp]),
    'edvr_dcnv2_fwd_split_applies': (i32, [vp] + [i32] * 13),
    'edvr_dcnv2_split_packed_weight_elems': (sz, [i32, i32]),
    'edvr_dcnv2_split_pack_weight_f32': (i32, [vp, vp, i32, i32, vp]),
    'edvr_dcnv2_fwd_split_packed_f32': (i32, [vp] * 6 + [i32] * 12 + [i64, i64, i32, i32, vp, vp]),
    'edvr_dcnv2_fwd_kernel_name': (i32, [vp] + [i32] * 13 + [ctypes.c_char_p, sz]),
    'edvr_dcnv2_bwd_ws_bytes': (sz, [i32] * 12),
    'edvr_dcnv2_any_ws_bytes': (sz, [i32] * 13),
    'edvr_dcnv2_fwd_any': (i32, [i32] + [vp] * 6 + [i32] * 12 + [i64, i64, vp, sz, vp]),
    'edvr_dcnv2_bwd_any': (i32, [i32] + [vp] * 10 + [i32] * 12 + [i64, i64, i64, i64, vp, sz, vp]),
    'edvr_psnr_sse_f32': (i32, [vp, vp, vp, i32, i32, i32, i32, i64, i64, i32, i32, i32, vp]),
    'edvr_ssim_partials': (sz, [i32, i32, i32]),
    'edvr_ssim_f32': (i32, [vp, vp, vp, i32, i32, i32, i32, i64, i64, i32, i32, vp]),
    'edvr_niqe_blocks': (sz, [i32, i32, i32]),
    'edvr_niqe_moments_f32': (i32, [vp, vp, i32, i32, i32, i32, i64, i32, vp]),
    'edvr_niqe_moments_u8': (i32, [vp, vp, i32, i32, i32, i64, i32, vp]),
    'edvr_frames_u8_to_f32': (i32, [vp, vp, i32, i32, i32, i32, vp, i32, vp]),
    'edvr_gather_images_f32': (i32, [vp, vp, vp, vp, i32, vp, i32, i32, vp]),
    'edvr_upsample4x_add_u8': (i32, [vp, vp, vp, i32, i32, i32, vp]),
    'edvr_f32_to_u8_hwc': (i32, [vp, vp, i32, i32, i32, i64, vp]),
    'edvr_crop_pad_frames_u8': (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    'edvr_crop_pad_frames_f32': (i32, [vp, vp, i32, i32, i32, i64, i32, i32, i32, i32, i32, vp]),
    'edvr_upsample4x_add_rect_f32': (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i64, i64, i64, vp]),
    'edvr_upsample4x_add_rect_u8': (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i64, i64, vp]),
    'edvr_f32_to_u8_hwc_rect': (i32, [vp, vp, i32, i32, i32, i64, i32, i32, i32, i32, i64, i64, vp]),
    'edvr_copy_rect_f32': (i32, [vp, vp, i32, i32, i32, i64, i32, i32, i32, i32, i64, i64, i64, vp]),
    'edvr_crop_pad_frames_d4_u8': (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    'edvr_crop_pad_frames_d4_f32': (i32, [vp, vp, i32, i32, i32, i64, i32, i32, i32, i32, i32, i32, vp]),
    'edvr_upsample4x_add_rect_d4_f32': (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i64, i64, i64, i32, i32, f32, vp]),
    'edvr_upsample4x_add_rect_d4_u8': (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i64, i64, i64, i64, i64, i32, i32, f32, vp]),
    'edvr_f32_to_u8_hwc_rect_d4': (i32, [vp, vp, vp, i32, i32, i32, i64, i32, i32, i32, i32, i64, i64, i64, i64, i64, i32, i32, f32, vp]),
    'edvr_copy_rect_d4_f32': (i32, [vp, vp, i32, i32, i32, i64, i32, i32, i32, i32, i64, i64, i64, i32, i32, f32, vp]),
    'edvr_upsample4x_add_rect_blend_f32': (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i64, i64, i64, i32, i32, f32, i32, i32, i32, i32, vp]),
    'edvr_upsample4x_add_rect_blend_u8': (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i64, i64, i64, i64, i64, i32, i32, f32, i32, i32, i32, i32, vp]),
    'edvr_f32_to_u8_hwc_rect_blend': (i32, [vp, vp, vp, i32, i32, i32, i64, i32, i32, i32, i32, i64, i64, i64, i64, i64, i32, i32, f32, i32, i32, i32, i32, vp]),
    'edvr_copy_rect_blend_f32': (i32, [vp, vp, i32, i32, i32, i64, i32, i32, i32, i32, i64, i64, i64, i32, i32, f32, i32, i32, i32, i32, vp]),
    'edvr_imresize_bicubic_u8': (i32, [vp, vp, i32, i32, i32, i32, i32, ctypes.c_double, i32, i32, vp]),
    'edvr_imresize_bicubic_f32': (i32, [vp, vp, i32, i32, i32, i64, i32, i32, ctypes.c_double, i32, i32, vp]),
    'edvr_resample_tile': (i32, [i32, i32, i32, i32, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]),
    'edvr_resample_f32': (i32, [vp, vp, i32, i32, i32, i32, i64, i32, i32, i64, vp, vp, i32, vp, vp, i32, vp]),
    'edvr_bd_downsample_u8': (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    'edvr_bd_downsample_f32': (i32, [vp, vp, i32, i32, i32, i64, i32, i32, i32, i32, vp]),
    'edvr_imresize_bicubic_u8_windows': (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    'edvr_bd_downsample_u8_windows': (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    'edvr_yuv420_to_rgb_f32': (i32, [vp, vp, i32, i32, i32, i64, i64, vp, i32, vp]),
    'edvr_yuv420_to_rgb_u8': (i32, [vp, vp, i32, i32, i32, i64, vp, i32, vp]),
    'edvr_rgb_to_yuv420_f32': (i32, [vp, vp, i32, i32, i32, i64, i64, vp, vp]),
    'edvr_rgb_to_yuv420_u8': (i32, [vp, vp, i32, i32, i32, i64, vp, vp]),
    'edvr_yuv_to_rgb_f32': (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i64, i64, vp, i32, vp]),
    'edvr_rgb_to_yuv_f32': (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i64, i64, vp, vp]),
    'edvr_yuv_to_rgb_sited_f32': (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i64, i64, vp, i32, i32, i32, vp]),
    'edvr_rgb_to_yuv_sited_f32': (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i64, i64, vp, i32, i32, vp]),
    'edvr_yuv420_to_rgb_sited_u8': (i32, [vp, vp, i32, i32, i32, i64, vp, i32, i32, i32, vp]),
    'edvr_rgb_to_yuv420_sited_u8': (i32, [vp, vp, i32, i32, i32, i64, vp, i32, i32, vp]),
    'edvr_deinterlace': (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i64, i64, i32, i32, vp]),
    'edvr_field_match': (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i64, i32, i32, i32, vp]),
    'edvr_field_weave': (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i64, i64, i32, vp]),
    'edvr_bar_profile': (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i64, vp]),
    'edvr_yuv_crop': (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i64, i64, i32, i32, i32, i32, vp]),
    'edvr_frame_sad_rgb_u8': (i32, [vp, vp, vp, i32, i32, i32, i64, vp]),
    'edvr_frame_sad_rgb_f32': (i32, [vp, vp, vp, i32, i32, i32, i64, vp]),
    'edvr_jpeg_roundtrip_u8': (i32, [vp, vp, vp, i32, i32, i32, i32, i64, i64, i32, vp]),
    'edvr_mpeg_roundtrip_workspace': (sz, [i32, i32, i32, i32]),
    'edvr_mpeg_roundtrip_u8': (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i64, i64, i64, i64, i32, i32, vp, sz, vp]),
    'edvr_degrade_u8': (i32, [vp, vp, vp, vp, i32, i32, i32, i64, i64, vp]),
    'edvr_philox_words_u32': (i32, [vp, u32, u32, u32, i32, i32, vp]),
    'edvr_adam_chunk_bytes': (sz, []),
    'edvr_adam_multi_f32': (i32, [vp, i32, ctypes.c_float, ctypes.c_float, ctypes.c_float, vp]),
    'edvr_dcnv1_fwd_ws_bytes': (sz, [i32] * 12),
    'edvr_dcnv1_fwd_f32': (i32, [vp] * 4 + [i32] * 12 + [i64, i32, vp, sz, vp]),
    'edvr_dcnv1_bwd_ws_bytes': (sz, [i32] * 12),
    'edvr_dcnv1_bwd_f32': (i32, [vp] * 7 + [i32] * 12 + [i64, i64, i32, vp, sz, vp]),
    'edvr_dcnv2_bwd_f32': (i32, [vp] * 10 + [i32] * 12 + [i64, i64, i64, i64, i32, vp, sz, vp]),
    'edvr_dcnv2_bwd_split_f32': (i32, [vp] * 10 + [i32] * 12 + [i64, i64, i64, i64, i32, vp, sz, vp, vp, vp]),
    'edvr_dcnv2_bwd_split_applies': (i32, []),
    'edvr_dcnv2_bwd_kernel_name': (i32, [i32] * 13 + [ctypes.c_char_p, sz]),
    'edvr_tsa_temporal_f32': (i32, [vp] * 5 + [i32] * 4 + [vp]),
    'edvr_tsa_temporal_pair_f32': (i32, [vp] * 5 + [i32] * 4 + [vp]),
    'edvr_tsa_front_supported': (i32, [i32] * 6),
    'edvr_tsa_front_applies': (i32, [i32] * 12 + [vp, vp, vp]),
    'edvr_tsa_front_f32': (i32, [vp, vp, i64, vp, vp] + [vp, vp, i32, vp, vp] * 2 + [i32] * 6 + [vp]),
    'edvr_pool_maxavg_3x3s2_f32': (i32, [vp, vp, i32, i32, i32, i32, vp]),
    'edvr_upsample2x_f32': (i32, [vp, vp, i32, i32, i32, f32, vp]),
    'edvr_tsa_combine_f32': (i32, [vp, vp, vp, vp, i64, vp]),
    'edvr_upsample4x_add_f32': (i32, [vp, vp, i32, i32, i32, vp]),
    'edvr_add_f32': (i32, [vp, vp, vp, i64, vp]),
    'edvr_act_bwd_f32': (i32, [vp, vp, vp, vp, vp, i32, i32, i64, i32, i32, vp]),
    'edvr_conv2d_wgrad_ws_bytes': (sz, [i32] * 7),
    'edvr_conv2d_wgrad_algo': (i32, [i32]),
    'edvr_conv2d_wgrad_kernel_name': (i32, [i32] * 8 + [ctypes.c_char_p, sz]),
    'edvr_conv2d_wgrad_f32': (i32, [vp] * 4 + [i32] * 8 + [i64, i64, i32, i32, i32, i64, i32, vp, vp, sz, vp]),
    'edvr_conv2d_wgrad_split_f32': (i32, [vp] * 4 + [i32] * 8 + [i64, i64, i32, i32, i32, i64, i32, vp, vp, sz, vp, vp, vp]),
    'edvr_conv2d_wgrad_split_applies': (i32, [i32] * 8),
    'edvr_conv2d_wgrad_split_is_direct': (i32, [i32] * 2),
    'edvr_channel_sum_f32': (i32, [vp, vp, i32, i32, i64, i64, vp, sz, vp]),
    'edvr_pixel_unshuffle2_f32': (i32, [vp, vp, i32, i32, i32, i32, vp]),
    'edvr_pixel_unshuffle2_act_bwd_f32': (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    'edvr_zero_stuff2_f32': (i32, [vp, vp, i32, i32, i32, i32, i32, vp]),
    'edvr_frame_reduce_add_f32': (i32, [vp, vp, i32, i32, i32, i64, vp]),
    'edvr_upsample2x_bwd_f32': (i32, [vp, vp, i32, i32, i32, f32, vp]),
    'edvr_pool_maxavg_3x3s2_bwd_f32': (i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
    'edvr_tsa_temporal_bwd_f32': (i32, [vp] * 7 + [i32] * 4 + [vp, vp]),
    'edvr_tsa_combine_bwd_f32': (i32, [vp] * 5 + [i64, vp]),
    'edvr_charbonnier_f32': (i32, [vp, vp, vp, vp, i64, f32, f32, vp]),
    'edvr_abs_sum_f32': (i32, [vp, vp, i32, i64, i64, vp]),
    'edvr_abs_stats_f32': (i32, [vp, vp, i32, i64, i32, i64, vp]),
}

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_SIGMOID = 0, 1, 2, 3
OUT_NCHW, OUT_PIXEL_SHUFFLE2 = 0, 1
CONV_AUTO, CONV_DIRECT, CONV_WINOGRAD, CONV_WINOGRAD_F4, CONV_WINOGRAD_F4S = 0, 1, 2, 3, 4
(CONV_KERNEL_SMALL, CONV_KERNEL_F4S, CONV_KERNEL_F4, CONV_KERNEL_F2, CONV_KERNEL_1X1_SPLIT, CONV_KERNEL_1X1_STREAM,
 CONV_KERNEL_DIRECT_SPLIT, CONV_KERNEL_DIRECT) = range(8)  # EDVR_CONV_KERNEL_*: what edvr_conv2d_kernel returns
DTYPE_F32, DTYPE_F64, DTYPE_F16 = 0, 1, 2  # EDVR_DTYPE_*
DCN_HALO_TAPWIN = 16  # EDVR_DCN_HALO_TAPWIN
JPEG_SUBSAMPLINGS = {'420': 420, '444': 444}  # EDVR_JPEG_*
DEGRADE_TILE, DEGRADE_MAX_KSIZE, DEGRADE_RECORD_INTS, DEGRADE_GRAY = 64, 21, 8, 1  # EDVR_DEGRADE_*

_lib = None


class ExtensionMissing(RuntimeError):
    pass


def lib():
    """Return the loaded library; raise ExtensionMissing if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ExtensionMissing(
                f'{LIB_PATH} not found: the HIP extension is not built (run `python -m edvr_amd.build`). '
                'edvr_amd has no CPU/PyTorch fallback.')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(handle, name)  # AttributeError if the ABI is incomplete
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().edvr_last_error().decode()
        raise RuntimeError(f'{what} failed (code {rc}): {msg}')
