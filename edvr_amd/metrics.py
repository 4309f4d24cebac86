"""Validation metrics on the device.

Mirrors xinntao/EDVR (BasicSR v1.2.0): tensor2img (basicsr/utils/img_util.py:36-98) followed by calculate_psnr
(basicsr/metrics/psnr_ssim.py:7-51), which VideoBaseModel.dist_validation (video_base_model.py:60-98) runs per frame in NumPy
after copying the frame to the host.  Here the clamp-round-uint8 conversion and the squared differences happen in one HIP
kernel (csrc/metrics.hip) and only one double per image leaves the GPU.  calculate_ssim (psnr_ssim.py:54-141) likewise: the
11x11 Gaussian moments and the SSIM map are computed in float64 on the device, a few partial sums per image leave it.

validate_clip() is the batched form of that loop for one clip: every frame's window of `num_frame` neighbours is built with
generate_frame_indices (basicsr/data/data_util.py:35-88, the padding modes of the REDS4 / Vid4 test sets), windows run through
the network `batch` at a time, and each output frame is scored on the device.
"""
import math

import torch

from . import _lib, ops


def sum_squared_error_uint8(pred, gt, crop_border=0, test_y_channel=False):
    """Per-image sum of squared differences of tensor2img(pred) and tensor2img(gt) inside the crop, and the element count.
    pred, gt: (n, c, h, w) fp32 CUDA tensors in RGB channel order (c = 3 or 1), values nominally in [0, 1] (clamped)."""
    ops.require_gpu(pred, gt)
    if pred.shape != gt.shape:
        raise AssertionError(f'Image shapes are differnet: {tuple(pred.shape)}, {tuple(gt.shape)}.')  # psnr_ssim.py:30-31
    if pred.dim() == 3:
        pred, gt = pred[None], gt[None]
    pred, gt = pred.contiguous(), gt.contiguous()
    n, c, h, w = pred.shape
    blocks = max(1, min(256, (h * w + 4095) // 4096))
    partial = torch.empty(n, blocks, dtype=torch.float64, device=pred.device)
    y = 1 if (test_y_channel and c == 3) else 0
    _lib.check(_lib.lib().edvr_psnr_sse_f32(pred.data_ptr(), gt.data_ptr(), partial.data_ptr(), n, c, h, w, c * h * w, c * h * w,
                                            int(crop_border), y, blocks, torch.cuda.current_stream(pred.device).cuda_stream), 'edvr_psnr_sse_f32')
    count = (h - 2 * crop_border) * (w - 2 * crop_border) * (1 if y else c)
    return partial.sum(1), count


def calculate_psnr(pred, gt, crop_border=0, test_y_channel=False):
    """calculate_psnr(tensor2img(pred), tensor2img(gt), crop_border, test_y_channel=...) of the reference for every image of
    the batch, as a list of floats (inf where the images are identical)."""
    sse, count = sum_squared_error_uint8(pred, gt, crop_border, test_y_channel)
    out = []
    for s in sse.cpu().tolist():
        mse = s / count
        out.append(float('inf') if mse == 0 else 20.0 * math.log10(255.0 / math.sqrt(mse)))
    return out


def calculate_ssim(pred, gt, crop_border=0, test_y_channel=False):
    """calculate_ssim(tensor2img(pred), tensor2img(gt), crop_border, test_y_channel=...) of the reference (psnr_ssim.py:90-141)
    for every image of the batch, as a list of floats.  pred, gt: (n, c, h, w) or (c, h, w) fp32 CUDA tensors, RGB, c = 3 or 1."""
    ops.require_gpu(pred, gt)
    if pred.shape != gt.shape:
        raise AssertionError(f'Image shapes are differnet: {tuple(pred.shape)}, {tuple(gt.shape)}.')  # psnr_ssim.py:118-119
    if pred.dim() == 3:
        pred, gt = pred[None], gt[None]
    pred, gt = pred.contiguous(), gt.contiguous()
    n, c, h, w = pred.shape
    L = _lib.lib()
    tiles = L.edvr_ssim_partials(h, w, int(crop_border))
    if tiles == 0:
        raise ValueError(f'calculate_ssim: {h}x{w} with crop_border {crop_border} leaves no 11x11 window')
    y = 1 if (test_y_channel and c == 3) else 0
    chans = 1 if y else c
    partial = torch.empty(n, chans, tiles, dtype=torch.float64, device=pred.device)
    _lib.check(L.edvr_ssim_f32(pred.data_ptr(), gt.data_ptr(), partial.data_ptr(), n, c, h, w, c * h * w, c * h * w, int(crop_border), y,
                               torch.cuda.current_stream(pred.device).cuda_stream), 'edvr_ssim_f32')
    count = (h - 2 * crop_border - 10) * (w - 2 * crop_border - 10)
    return (partial.sum(2) / count).mean(1).cpu().tolist()


# ------------------------------------------------------------------------------------------------ NIQE
NIQE_BLOCK = 96  # block_size_h / block_size_w of the reference (the official recommended value), no overlap
_NIQE_TABLE = None


def niqe_window():
    """The 7 x 7 Gaussian of NIQE (sigma 7 / 6, normalised to sum 1) in float64: the `gaussian_window` of the reference's parameter
    file to 1.4e-17, and what csrc/niqe.hip builds on the host for its argument block."""
    import numpy as np
    d = np.arange(7, dtype=np.float64) - 3.0
    g = np.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


def load_niqe_params(path):
    """The pristine multivariate Gaussian model NIQE compares against: the `niqe_pris_params.npz` that ships with BasicSR
    (basicsr/metrics/), user-supplied like a checkpoint.  Returns (mu_pris_param (1, 36), cov_pris_param (36, 36)) in float64."""
    import numpy as np
    with np.load(path) as f:
        mu, cov = np.asarray(f['mu_pris_param'], np.float64), np.asarray(f['cov_pris_param'], np.float64)
    if mu.reshape(-1).shape != (36,) or cov.shape != (36, 36):
        raise ValueError(f'{path}: mu_pris_param {mu.shape} / cov_pris_param {cov.shape} are not a 36-feature model')
    return mu.reshape(1, 36), cov


def _niqe_table():
    """gam = arange(0.2, 10.001, 0.001) and r_gam = Gamma(2/g)^2 / (Gamma(1/g) Gamma(3/g)) (niqe.py:21-24), built once."""
    global _NIQE_TABLE
    if _NIQE_TABLE is None:
        import numpy as np
        gam = np.arange(0.2, 10.001, 0.001)
        rec = np.reciprocal(gam)
        G = np.vectorize(math.gamma, otypes=[np.float64])
        r_gam = np.square(G(rec * 2)) / (G(rec) * G(rec * 3))
        _NIQE_TABLE = (gam, r_gam, bool(np.all(np.diff(r_gam) > 0)))
    return _NIQE_TABLE


def _niqe_argmin(x):
    """np.argmin((r_gam - x) ** 2) for every element of x: the table is increasing, so the minimum is next to the insertion point
    (the first of equal minima, as argmin returns); an all-NaN row gives 0, as argmin does."""
    import numpy as np
    gam, r_gam, increasing = _niqe_table()
    flat = np.asarray(x, np.float64).reshape(-1)
    if not increasing:
        pos = np.array([int(np.argmin((r_gam - v) ** 2)) for v in flat], dtype=np.int64)
        return pos.reshape(np.shape(x))
    nan = np.isnan(flat)
    i = np.searchsorted(r_gam, np.where(nan, 0.0, flat))
    cand = np.clip(i[:, None] + np.arange(-2, 2)[None, :], 0, len(r_gam) - 1)  # ascending: argmin picks the first minimum
    pos = np.take_along_axis(cand, np.argmin((r_gam[cand] - np.where(nan, 0.0, flat)[:, None]) ** 2, axis=1)[:, None], 1)[:, 0]
    return np.where(nan, 0, pos).reshape(np.shape(x))


def niqe_features(moments):
    """estimate_aggd_param + compute_feature (niqe.py:10-64) from the 25 moments of every block: (..., 2, blocks, 5, 5) -> (..., blocks, 36)
    float64, scale 1's 18 features then scale 2's.  NaN where the reference gets NaN (a map without negative or without positive
    values: the mean of an empty selection)."""
    import numpy as np
    m = np.asarray(moments.detach().cpu().numpy() if torch.is_tensor(moments) else moments, dtype=np.float64)
    if m.ndim < 4 or m.shape[-4] != 2 or m.shape[-2:] != (5, 5):
        raise ValueError(f'moments are (..., 2, blocks, 5, 5), got {m.shape}')
    gam = _niqe_table()[0]
    G = np.vectorize(math.gamma, otypes=[np.float64])
    count = np.array([NIQE_BLOCK ** 2, (NIQE_BLOCK // 2) ** 2], np.float64).reshape(2, 1, 1)  # pixels per block at each scale
    with np.errstate(all='ignore'):
        left_std, right_std = np.sqrt(m[..., 0] / m[..., 1]), np.sqrt(m[..., 2] / m[..., 3])
        gammahat = left_std / right_std
        rhat = (m[..., 4] / count) ** 2 / ((m[..., 0] + m[..., 2]) / count)
        rhatnorm = (rhat * (gammahat ** 3 + 1) * (gammahat + 1)) / ((gammahat ** 2 + 1) ** 2)
        alpha = gam[_niqe_argmin(rhatnorm)]
        scale = np.sqrt(G(1 / alpha) / G(3 / alpha))
        beta_l, beta_r = left_std * scale, right_std * scale
        mean = (beta_r - beta_l) * (G(2 / alpha) / G(1 / alpha))  # Eq. 8
    feat = [alpha[..., 0], (beta_l[..., 0] + beta_r[..., 0]) / 2]
    for k in range(1, 5):
        feat += [alpha[..., k], mean[..., k], beta_l[..., k], beta_r[..., k]]
    f = np.stack(feat, -1)  # (..., 2, blocks, 18)
    return np.concatenate([f[..., 0, :, :], f[..., 1, :, :]], -1)


def niqe_from_moments(moments, nbh, nbw, params):
    """The host finish of NIQE (niqe.py:140-155) in NumPy float64: moments (n, 2, nbh nbw, 5, 5) as niqe_moments returns them (a device or
    host tensor, or an array) -> [NIQE per frame].  params: (mu_pris_param, cov_pris_param) of load_niqe_params.  NaN where the
    reference's arithmetic gives NaN - in particular with fewer than two NaN-free blocks, where np.cov has nothing to estimate."""
    import numpy as np
    feats = niqe_features(moments)
    if feats.ndim != 3 or feats.shape[1] != int(nbh) * int(nbw):
        raise ValueError(f'moments of {feats.shape[1:2]} blocks for a {nbh} x {nbw} grid')
    mu_pris, cov_pris = np.asarray(params[0], np.float64).reshape(1, 36), np.asarray(params[1], np.float64)
    out = []
    for distparam in feats:
        with np.errstate(all='ignore'):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                mu = np.nanmean(distparam, axis=0)
                rows = distparam[~np.isnan(distparam).any(axis=1)]
                cov = np.cov(rows, rowvar=False) if rows.shape[0] else np.full((36, 36), np.nan)
            mat = (cov_pris + cov) / 2
            if not np.isfinite(mat).all() or not np.isfinite(mu).all():
                out.append(float('nan'))
                continue
            d = mu_pris - mu
            out.append(float(np.sqrt(np.matmul(np.matmul(d, np.linalg.pinv(mat)), d.T))[0, 0]))
    return out


def _niqe_input(img):
    if not torch.is_tensor(img):
        raise TypeError('NIQE reads a torch tensor')
    ops.require_gpu(img, dtypes=(torch.float32, torch.uint8))
    if img.dtype == torch.uint8:
        if img.dim() == 3:
            img = img[None]
        if img.dim() != 4 or img.shape[3] != 3:
            raise ValueError(f'uint8 frames are (n, h, w, 3) RGB, got {tuple(img.shape)}')
        return img.contiguous(), 3, img.shape[1], img.shape[2]
    if img.dim() == 3:
        img = img[None]
    if img.dim() != 4 or img.shape[1] not in (1, 3):
        raise ValueError(f'float32 frames are (n, 3 | 1, h, w) RGB, got {tuple(img.shape)}')
    return img.contiguous(), img.shape[1], img.shape[2], img.shape[3]


def niqe_grid(h, w, crop_border=0):
    """(nbh, nbw): the 96 x 96 blocks of an (h, w) frame after crop_border left every side; ValueError when none fits."""
    c = int(crop_border)
    nbh, nbw = (h - 2 * c) // NIQE_BLOCK, (w - 2 * c) // NIQE_BLOCK
    if c < 0 or nbh < 1 or nbw < 1:
        raise ValueError(f'calculate_niqe: {h}x{w} with crop_border {crop_border} leaves no {NIQE_BLOCK}x{NIQE_BLOCK} block')
    return nbh, nbw


def niqe_moments(img, crop_border=0):
    """The device part of NIQE (csrc/niqe.hip), one launch for all frames, both scales and all blocks: (n, 2, blocks, 5, 5) float64 on the
    device - per frame, scale (full size, 2x2 mean) and 96 / 48-pixel block (column-major), per map (z and its four roll products) the
    sum of squares and the count of the negative values, the same of the positive ones, and the sum of absolute values.
    img: float32 (n, 3 | 1, h, w) or (3 | 1, h, w), RGB in [0, 1] (tensor2img's clamp and rounding apply; 3 channels -> Y of to_y_channel), or
    uint8 (n, h, w, 3) RGB bytes as VideoRestorer(out_dtype=torch.uint8) returns them."""
    x, c, h, w = _niqe_input(img)
    nbh, nbw = niqe_grid(h, w, crop_border)
    L = _lib.lib()
    n, blocks = x.shape[0], nbh * nbw
    assert L.edvr_niqe_blocks(h, w, int(crop_border)) == blocks
    out = torch.empty(n, 2, blocks, 5, 5, dtype=torch.float64, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    if x.dtype == torch.uint8:
        _lib.check(L.edvr_niqe_moments_u8(x.data_ptr(), out.data_ptr(), n, h, w, 3 * h * w, int(crop_border), stream), 'edvr_niqe_moments_u8')
    else:
        _lib.check(L.edvr_niqe_moments_f32(x.data_ptr(), out.data_ptr(), n, c, h, w, c * h * w, int(crop_border), stream), 'edvr_niqe_moments_f32')
    return out


def calculate_niqe(img, crop_border=0, params=None, convert_to='y'):
    """calculate_niqe(tensor2img(img), crop_border, convert_to='y') of the reference (basicsr/metrics/niqe.py:158-205) for every frame of
    the batch, as a list of floats (lower is better; NaN where the reference's arithmetic gives NaN).  img: as niqe_moments takes it (a
    1-channel image is scored as its bytes, the reference's 'HW' order).  params: load_niqe_params(...)'s result or the path of the .npz -
    the pristine model is user-supplied, the package ships no copy.  ValueError when no 96 x 96 block fits; the per-pixel work runs in one
    HIP kernel and 50 doubles per block leave the device."""
    if convert_to != 'y':
        if convert_to == 'gray':
            raise NotImplementedError("calculate_niqe: convert_to='gray' needs OpenCV's luma; only 'y' is implemented")
        raise ValueError(f"convert_to is 'y' (or 'gray'), got {convert_to!r}")
    if params is None:
        raise ValueError('calculate_niqe needs params: load_niqe_params(path) or the path of niqe_pris_params.npz')
    if isinstance(params, (str, bytes)) or hasattr(params, '__fspath__'):
        params = load_niqe_params(params)
    x, c, h, w = _niqe_input(img)
    nbh, nbw = niqe_grid(h, w, crop_border)
    return niqe_from_moments(niqe_moments(x, crop_border), nbh, nbw, params)


def generate_frame_indices(crt_idx, max_frame_num, num_frames, padding='reflection'):
    """basicsr/data/data_util.py:35-88: indices of the `num_frames` frames around `crt_idx` in a sequence of `max_frame_num`
    frames, out-of-range positions padded by 'replicate' | 'reflection' | 'reflection_circle' | 'circle'."""
    assert num_frames % 2 == 1, 'num_frames should be an odd number.'
    assert padding in ('replicate', 'reflection', 'reflection_circle', 'circle'), f'Wrong padding mode: {padding}.'
    max_frame_num = max_frame_num - 1  # start from 0
    num_pad = num_frames // 2
    indices = []
    for i in range(crt_idx - num_pad, crt_idx + num_pad + 1):
        if i < 0:
            pad_idx = {'replicate': 0, 'reflection': -i, 'reflection_circle': crt_idx + num_pad - i, 'circle': num_frames + i}[padding]
        elif i > max_frame_num:
            pad_idx = {'replicate': max_frame_num, 'reflection': max_frame_num * 2 - i,
                       'reflection_circle': (crt_idx - num_pad) - (i - max_frame_num), 'circle': i - num_frames}[padding]
        else:
            pad_idx = i
        indices.append(pad_idx)
    return indices


@torch.no_grad()
def validate_clip(net, lq, gt=None, num_frame=5, padding='reflection_circle', batch=4, crop_border=0, test_y_channel=False):
    """Restore every frame of one clip and (if `gt` is given) score it: what VideoBaseModel.dist_validation
    (video_base_model.py:44-98) does frame by frame with a host round trip per frame.
    lq: (t, c, h, w) low-quality frames on the GPU, gt: (t, c, H, W).  Returns (outputs (t, c, H, W), [PSNR per frame] or None)."""
    t = lq.shape[0]
    outs, scores = [], []
    for s0 in range(0, t, batch):
        idx = [generate_frame_indices(i, t, num_frame, padding) for i in range(s0, min(s0 + batch, t))]
        windows = lq[torch.tensor(idx, device=lq.device)]  # (b, num_frame, c, h, w)
        out = net(windows)
        outs.append(out)
        if gt is not None:
            scores += calculate_psnr(out, gt[s0:s0 + out.shape[0]], crop_border, test_y_channel)
    return torch.cat(outs, 0), (scores if gt is not None else None)


@torch.no_grad()
def validate_video(net, lq, gt=None, num_frame=5, padding='reflection_circle', chunk=8, crop_border=0, test_y_channel=False, pad_mode=None,
                   tile=None, tile_overlap=None, self_ensemble=None, tile_blend=None, time_reverse=False, cuts=None,
                   cut_threshold=None):
    """validate_clip with every frame's features extracted once (edvr_amd/video.py: VideoRestorer) instead of once per window it
    appears in; `chunk` output frames per alignment / fusion / reconstruction pass.  Same arguments otherwise, same return value:
    (outputs (t, c, H, W), [PSNR per frame] or None).  pad_mode / tile / tile_overlap: VideoRestorer's, for frames of any size - the
    outputs and `gt` are (s H, s W) for LQ frames of (H, W), whatever they were padded to.  self_ensemble: VideoRestorer's ('flip4', 'd4' or
    element ids): the outputs and their PSNRs are those of the averaged result, at n times the cost.  tile_blend: VideoRestorer's (input
    pixels): the outputs and their PSNRs are those of the tiles cross-faded around their cuts.  time_reverse: VideoRestorer's - every
    element also runs on the video in reversed frame order (the alignment is shared); composes with self_ensemble.  cuts:
    VideoRestorer's (None | 'auto' | frame indices; cut_threshold with 'auto') - every shot is restored as a video of its own."""
    from .video import VideoRestorer
    outs, scores, s0 = [], [], 0
    vr = VideoRestorer(net, num_frame=num_frame, padding=padding, chunk=chunk, pad_mode=pad_mode, tile=tile, tile_overlap=tile_overlap,
                       self_ensemble=self_ensemble, **({} if tile_blend is None else dict(tile_blend=tile_blend)),
                       **(dict(time_reverse=True) if time_reverse else {}), **({} if cuts is None else dict(cuts=cuts)),
                       **({} if cut_threshold is None else dict(cut_threshold=cut_threshold)))
    for out in vr.restore_chunks(lq.split(chunk), length=lq.shape[0]):
        outs.append(out)
        if gt is not None:
            scores += calculate_psnr(out, gt[s0:s0 + out.shape[0]], crop_border, test_y_channel)
        s0 += out.shape[0]
    return torch.cat(outs, 0), (scores if gt is not None else None)
