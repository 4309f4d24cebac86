"""The LQ copy of a folder of sharp frames, made on the device: MATLAB's antialiased bicubic imresize ("BI x4") - the replacement for
the reference's scripts/matlab_scripts/generate_bicubic_img.m - or, with --degradation bd, DUF's Gaussian blur and subsampling ("BD",
the reference's duf_downsample; scales 2, 3, 4).

    python scripts/make_lq.py datasets/REDS4/GT datasets/REDS4/sharp_bicubic --scale 4
    python scripts/make_lq.py datasets/Vid4/GT datasets/Vid4/BDx4 --scale 4 --degradation bd
    python scripts/make_lq.py datasets/REDS/train_blur datasets/REDS/train_blur_comp --scale 1 --jpeg-quality 40

GT_ROOT/<clip>/<frame>.png -> LQ_ROOT/<clip>/<frame>.png.  Frames are decoded and encoded on host threads through PIL (as
edvr_amd/data.py decodes), mod-cropped to a multiple of the scale (as the MATLAB script does), resized by 1 / scale in one launch per
batch of equal-sized frames (edvr_amd.ops.imresize or ops.bd_downsample, uint8 in, uint8 out: the rounding tensor2img applies) and
written as 8-bit PNG.

`--jpeg-quality Q [--jpeg-subsampling 420|444]` sends the resized bytes through a baseline JPEG round trip on the device before they are
stored (edvr_amd.ops.jpeg_roundtrip, DESIGN 4.16: the bytes PIL's JPEG writer and reader return): compression artifacts in the LQ tree,
still stored as PNG.  `--scale 1` skips the resize - imresize at scale 1 is the identity on bytes (tests/test_gpu_jpeg.py checks it), so
nothing changes without the option - and with it compresses a tree at its own size (deblurcomp-style data).

`--blur-sigma SX [SY THETA] [--blur-size K]`, `--noise-sigma S`, `--noise-shot A`, `--noise-gray`, `--degrade-seed N` blur the resized
bytes with a Gaussian kernel and add read / shot noise on the device (edvr_amd.ops.degrade) before the JPEG round trip:
blur, noise, compression, the first-order degradation model.  Frame i of a clip takes the noise field of index i of the key N, so a
tree is reproducible whatever --batch is; `--scale 1` degrades a tree at its own size.

`--mpeg-qscale Q [--mpeg-gop N] [--mpeg-search R]` codes each clip's frames, in order, with the MPEG-style I / P round trip on the device
(edvr_amd.ops.mpeg_roundtrip, DESIGN 4.18: an intra frame every N frames, motion-compensated prediction between them) after blur and
noise and before the JPEG round trip.  A clip is handled in pieces that start on an intra frame - the largest multiple of N within
--batch, or N itself - so the tree is what the whole clip in one call gives, whatever --batch is; `--mpeg-gop 0` (the first frame alone
is intra) takes each clip in one piece.  The frames of a clip must then have one size.
"""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

EXTENSIONS = ('.png', '.jpg', '.jpeg', '.bmp')


def walk(gt_root):
    """[(clip, [frame file names])] of a <clip>/<frame> tree, both sorted; dot files and other file types are skipped."""
    clips = []
    for clip in sorted(e.name for e in os.scandir(gt_root) if e.is_dir() and not e.name.startswith('.')):
        frames = sorted(e.name for e in os.scandir(os.path.join(gt_root, clip))
                        if e.is_file() and not e.name.startswith('.') and e.name.lower().endswith(EXTENSIONS))
        if frames:
            clips.append((clip, frames))
    return clips


def resize_u8(frames_u8, scale, antialiasing, device):
    """(n, H, W, 3) uint8 host array -> (n, H / scale, W / scale, 3) uint8 host array, resized on the device."""
    from edvr_amd import ops
    return ops.imresize(torch.from_numpy(frames_u8).to(device), 1 / scale, antialiasing, out_dtype=torch.uint8).cpu().numpy()


def bd_u8(frames_u8, scale, device):
    """(n, H, W, 3) uint8 host array -> (n, H / scale, W / scale, 3) uint8 host array, DUF-downsampled on the device."""
    from edvr_amd import ops
    return ops.bd_downsample(torch.from_numpy(frames_u8).to(device), scale, out_dtype=torch.uint8).cpu().numpy()


def jpeg_u8(frames_u8, quality, subsampling, device):
    """(n, H, W, 3) uint8 host array -> the same after a JPEG round trip on the device."""
    from edvr_amd import ops
    return ops.jpeg_roundtrip(torch.from_numpy(frames_u8).to(device), quality, subsampling).cpu().numpy()


def mpeg_u8(frames_u8, qscale, gop, search, device):
    """(t, H, W, 3) uint8 host array, one clip in order -> the same after the MPEG-style round trip on the device."""
    from edvr_amd import ops
    return ops.mpeg_roundtrip(torch.from_numpy(frames_u8).to(device), qscale, gop, search).cpu().numpy()


def gop_pieces(n, batch, gop):
    """[(first, past the last)] frames of the pieces a clip of n frames is handled in: `batch` frames each without the MPEG round trip
    (gop None); with it every piece starts on an intra frame - the largest multiple of gop within batch, or gop itself - and gop 0 is
    the whole clip."""
    step = batch if gop is None else n if gop == 0 else max(gop, batch // gop * gop)
    return [(s0, min(s0 + step, n)) for s0 in range(0, n, max(step, 1))]


def degrade_u8(frames_u8, kernel, noise, seed, frame_index, device):
    """(n, H, W, 3) uint8 host array -> the same blurred and noisy, on the device."""
    from edvr_amd import ops
    return ops.degrade(torch.from_numpy(frames_u8).to(device), kernel, noise, seed, frame_index).cpu().numpy()


def load(path, scale):
    from edvr_amd.data import decode_image
    with open(path, 'rb') as f:
        img = decode_image(f.read())
    return np.ascontiguousarray(img[:img.shape[0] - img.shape[0] % scale, :img.shape[1] - img.shape[1] % scale])


def save(path, rgb_u8):
    from PIL import Image
    Image.fromarray(rgb_u8).save(os.path.splitext(path)[0] + '.png', format='PNG')


def make_lq(gt_root, lq_root, scale=4, antialiasing=True, batch=16, num_threads=8, device='cuda', log=print, degradation='bi',
            jpeg_quality=None, jpeg_subsampling='420', degrade=None, degrade_seed=0, mpeg_qscale=None, mpeg_gop=12, mpeg_search=7):
    """Returns the number of frames written.  jpeg_quality 1 .. 100: the stored bytes have been through a JPEG round trip.  degrade: the
    dict data.lq_from_gt takes - blur and noise before that, frame i of a clip at frame index i of the key degrade_seed.  mpeg_qscale
    1 .. 31: between the two, each clip goes through the MPEG-style round trip, in pieces cut at multiples of mpeg_gop (gop_pieces)."""
    from edvr_amd.data import bd_shape, degrade_spec, imresize_shape
    kernel, noise = degrade_spec(degrade) if degrade is not None else (None, None)
    if degradation not in ('bi', 'bd'):
        raise ValueError(f"degradation must be 'bi' or 'bd', got {degradation!r}")
    if jpeg_quality is not None:
        from edvr_amd import ops
        jpeg_quality = ops.jpeg_quality(jpeg_quality, 'jpeg_quality')
        if jpeg_subsampling not in ops.JPEG_SUBSAMPLINGS:
            raise ValueError(f'jpeg_subsampling must be one of {ops.JPEG_SUBSAMPLINGS}, got {jpeg_subsampling!r}')
    if mpeg_qscale is not None:
        from edvr_amd import ops
        mpeg_qscale, mpeg_gop, mpeg_search = ops.mpeg_qscale(mpeg_qscale, 'mpeg_qscale'), ops.mpeg_gop(mpeg_gop, 'mpeg_gop'), ops.mpeg_search(mpeg_search, 'mpeg_search')
    if degradation == 'bd':
        bd_shape(7, 7, scale)  # a scale DUF's kernel does not have: ValueError before any file is read
    clips = walk(gt_root)
    if not clips:
        raise FileNotFoundError(f'no <clip>/<frame> images under {gt_root}')
    written = 0
    with ThreadPoolExecutor(num_threads) as pool:
        for clip, frames in clips:
            os.makedirs(os.path.join(lq_root, clip), exist_ok=True)
            for s0, s1 in gop_pieces(len(frames), batch, mpeg_gop if mpeg_qscale is not None else None):
                names = frames[s0:s1]
                imgs = list(pool.map(lambda n: load(os.path.join(gt_root, clip, n), scale), names))
                if mpeg_qscale is not None and len({im.shape for im in imgs}) > 1:
                    raise ValueError(f'{clip}: the MPEG round trip predicts a frame from the one before: the frames of a clip must have one size')
                for shape in sorted({im.shape for im in imgs}):  # one launch per frame size (a clip normally has one)
                    sel = [i for i, im in enumerate(imgs) if im.shape == shape]
                    if degradation == 'bd':
                        bd_shape(shape[0], shape[1], scale)  # a frame too small for the kernel: ValueError naming it
                        out = bd_u8(np.stack([imgs[i] for i in sel]), scale, device)
                    elif scale == 1:  # the identity on bytes
                        out = np.stack([imgs[i] for i in sel])
                    else:
                        imresize_shape(shape[0], shape[1], 1 / scale, antialiasing)  # likewise
                        out = resize_u8(np.stack([imgs[i] for i in sel]), scale, antialiasing, device)
                    if degrade is not None:
                        out = degrade_u8(out, kernel, noise, degrade_seed, [s0 + i for i in sel], device)
                    if mpeg_qscale is not None:
                        out = mpeg_u8(out, mpeg_qscale, mpeg_gop, mpeg_search, device)
                    if jpeg_quality is not None:
                        out = jpeg_u8(out, jpeg_quality, jpeg_subsampling, device)
                    list(pool.map(lambda io: save(os.path.join(lq_root, clip, names[io[0]]), io[1]), zip(sel, out)))
                written += len(names)
            log(f'{clip}: {len(frames)} frame(s)')
    return written


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('gt_root')
    ap.add_argument('lq_root')
    ap.add_argument('--scale', type=int, default=4)
    ap.add_argument('--degradation', choices=('bi', 'bd'), default='bi',
                    help="bi: MATLAB's antialiased bicubic imresize; bd: DUF's 13 x 13 Gaussian blur and subsampling (scale 2, 3 or 4)")
    ap.add_argument('--no-antialias', action='store_true', help="imresize(..., 'Antialiasing', false) (bi only)")
    ap.add_argument('--jpeg-quality', type=int, default=None, metavar='Q',
                    help='send the LQ bytes through a baseline JPEG round trip at quality Q (1..100) before they are stored')
    ap.add_argument('--jpeg-subsampling', choices=('420', '444'), default='420', help='chroma subsampling of --jpeg-quality')
    ap.add_argument('--mpeg-qscale', type=int, default=None, metavar='Q',
                    help='code each clip with the MPEG-style I / P round trip at quantiser scale Q (1..31) before the JPEG round trip')
    ap.add_argument('--mpeg-gop', type=int, default=12, metavar='N', help='with --mpeg-qscale: an intra frame every N frames (0: the first alone)')
    ap.add_argument('--mpeg-search', type=int, default=7, metavar='R', help='with --mpeg-qscale: the motion search range, 0..15')
    ap.add_argument('--blur-sigma', type=float, nargs='+', default=None, metavar='S',
                    help='Gaussian blur of the LQ bytes: SX, or SX SY THETA (sigmas in pixels, THETA in radians from the x axis)')
    ap.add_argument('--blur-size', type=int, default=None, metavar='K', help='with --blur-sigma: the kernel size, odd, 3..21 (default: 3 sigma each side)')
    ap.add_argument('--noise-sigma', type=float, default=None, metavar='S', help='read noise: standard deviation in levels of 0..255')
    ap.add_argument('--noise-shot', type=float, default=None, metavar='A', help='shot noise: variance per level (Poisson scale p: A = p^2)')
    ap.add_argument('--noise-gray', action='store_true', help='one noise draw for the three channels of a pixel')
    ap.add_argument('--degrade-seed', type=int, default=0, metavar='N', help='the 64-bit key of the noise fields')
    ap.add_argument('--batch', type=int, default=16, help='frames per launch')
    ap.add_argument('--threads', type=int, default=8, help='host threads decoding and encoding')
    args = ap.parse_args(argv)
    if not 1 <= args.scale <= 8:
        ap.error('--scale must be an integer in 1..8')
    if args.degradation == 'bd' and args.scale not in (2, 3, 4):
        ap.error('--degradation bd takes --scale 2, 3 or 4')
    if args.degradation == 'bd' and args.no_antialias:
        ap.error('--no-antialias belongs to --degradation bi')
    if args.jpeg_quality is not None and not 1 <= args.jpeg_quality <= 100:
        ap.error('--jpeg-quality must be an integer in 1..100')
    if args.mpeg_qscale is not None and not 1 <= args.mpeg_qscale <= 31:
        ap.error('--mpeg-qscale must be an integer in 1..31')
    if args.mpeg_gop < 0 or not 0 <= args.mpeg_search <= 15:
        ap.error('--mpeg-gop must not be negative, --mpeg-search must be an integer in 0..15')
    from edvr_amd.data import degrade_options
    try:
        args.degrade = degrade_options(args.blur_sigma, args.blur_size, args.noise_sigma, args.noise_shot, args.noise_gray)
    except ValueError as e:
        ap.error(str(e))
    return args


def main():
    args = parse_args()
    n = make_lq(args.gt_root, args.lq_root, args.scale, not args.no_antialias, args.batch, args.threads, degradation=args.degradation,
                jpeg_quality=args.jpeg_quality, jpeg_subsampling=args.jpeg_subsampling, degrade=args.degrade, degrade_seed=args.degrade_seed,
                mpeg_qscale=args.mpeg_qscale, mpeg_gop=args.mpeg_gop, mpeg_search=args.mpeg_search)
    print(f'{n} frame(s) -> {args.lq_root}')


if __name__ == '__main__':
    main()
