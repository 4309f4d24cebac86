"""edvr_amd - the EDVR hot path (DCNv2 / PCD alignment / TSA fusion / conv trunks) as
hand-written HIP for AMD MI355X (gfx950), behind the module API of xinntao/EDVR.

    from edvr_amd import EDVR, PCDAlignment, TSAFusion, PredeblurModule
    from edvr_amd import DCNv2Pack, ModulatedDeformConv, ModulatedDeformConvPack, modulated_deform_conv
    from edvr_amd import VideoRestorer, window_table   # whole videos: every frame's features extracted once (edvr_amd/video.py)
    from edvr_amd import imresize                      # MATLAB bicubic on the device: x4 LQ frames from GT, the bicubic baseline
    from edvr_amd import duf_downsample                # DUF's Gaussian "BD" downsampling on the device (x2 / x3 / x4)

The kernels live in edvr_amd/lib/libedvr_amd.so (C ABI: include/edvr_amd.h; build with
`python -m edvr_amd.build`).  There is no CPU or stock-PyTorch fallback: CPU tensors raise
NotImplementedError exactly like the reference op, and a missing library raises ExtensionMissing.
"""
from ._lib import ExtensionMissing  # noqa: F401
from .arch_util import DCNv2Pack, ResidualBlockNoBN, default_init_weights, make_layer  # noqa: F401
from .data import bd_shape, duf_downsample, imresize, imresize_shape  # noqa: F401
from .dcn import (DeformConv, DeformConvFunction, DeformConvPack, ModulatedDeformConv,  # noqa: F401
                  ModulatedDeformConvFunction, ModulatedDeformConvPack, deform_conv, modulated_deform_conv)
from .edvr_arch import EDVR, PCDAlignment, PredeblurModule, TSAFusion  # noqa: F401
from .video import VideoRestorer, WindowSchedule, ensemble_elements, tile_bands, tile_grid, window_table  # noqa: F401
from .shots import ShotDetector, cut_scores, select_cuts  # noqa: F401

__version__ = '0.1.0'
