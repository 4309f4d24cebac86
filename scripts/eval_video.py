"""scripts/test_reds.py for the folder datasets (REDS4 / Vid4 layout) with every frame's features extracted ONCE per clip
(metrics.validate_video on edvr_amd/video.py: VideoRestorer) instead of once per window the frame appears in.  Same options, same
sharding of the clips over the ranks, same per-folder and overall averages; `--batch` is the number of output frames per alignment /
fusion / reconstruction pass.  `--pad-mode reflect` admits frames of any size, `--tile TH TW` bounds the memory of large ones,
`--tile-blend N` cross-fades neighbouring tiles over N input pixels around each cut (VideoRestorer's tile_blend).
`--self-ensemble flip4|d4` also restores every clip under the 4 flips / the 8 symmetries of the square and averages (the "+" rows of
the papers; VideoRestorer's self_ensemble, n times the time) and reports the plain and the ensemble PSNR side by side.
`--time-reverse` adds the video in reversed frame order to the ensemble (VideoRestorer's time_reverse: x2 on top, the alignment shared
between the two orders); alone it is an ensemble of the two time orders, with `--self-ensemble d4` the x16 one.

    python scripts/eval_video.py --lq datasets/REDS4/sharp_bicubic --gt datasets/REDS4/GT --weights EDVR_L_x4_SR_REDS_official.pth
    python scripts/eval_video.py --lq-from-gt 4 --bicubic-baseline --gt my_footage --weights EDVR_L_x4_SR_REDS_official.pth

`--lq-from-gt SCALE` needs no LQ folder: the LQ frames are MATLAB's bicubic reduction of the GT frames, made on the device
(edvr_amd.data.imresize, 8-bit like a stored dataset); with `--degradation bd` they are DUF's Gaussian blur and subsampling instead
(edvr_amd.data.duf_downsample, SCALE 2, 3 or 4, float as the reference's VideoTestDUFDataset feeds them).  `--bicubic-baseline` scores the
bicubic enlargement of the LQ frames beside the model under either degradation, as the published BI and BD tables do (the LQ frames
themselves for --hr-in networks); `--jpeg-quality Q [--jpeg-subsampling 420|444]` sends the 8-bit LQ frames through a baseline JPEG round
trip first (edvr_amd.ops.jpeg_roundtrip; with --degradation bd it rounds them to 8 bits), and the baseline then enlarges the compressed
frames; `--blur-sigma SX [SY THETA] [--blur-size K]`, `--noise-sigma S`, `--noise-shot A`, `--noise-gray`, `--degrade-seed N` blur the
8-bit LQ frames and add noise before that (edvr_amd.ops.degrade); `--mpeg-qscale Q [--mpeg-gop N] [--mpeg-search R]` codes
each folder's 8-bit LQ frames, read whole as one clip, with the MPEG-style I / P round trip between the two (edvr_amd.ops.mpeg_roundtrip,
DESIGN 4.18; a folder is one piece, so any --mpeg-gop, 0 included, is what the whole clip gives); `--json FILE` writes what is printed, and the degradation. `--niqe PARAMS.npz` also scores every
output with the no-reference NIQE (metrics.calculate_niqe against BasicSR's niqe_pris_params.npz, lower is better) - the model's, the
second pass's and the baseline's, next to their PSNRs.

The Vimeo90K-Test list is one window per item - nothing to reuse: use scripts/test_reds.py --vimeo-meta for it.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def bicubic_baseline(lq, gt, hr_in=False, crop_border=0, test_y_channel=False, chunk=8):
    """PSNR per frame of the bicubic enlargement of `lq` (t, 3, h, w) to the size of `gt` (t, 3, H, W) - the LQ frames themselves when
    hr_in - scored exactly as the model's output is."""
    from edvr_amd import metrics
    from edvr_amd.data import imresize
    scale = 1 if hr_in else gt.shape[-1] // lq.shape[-1]
    scores = []
    for s0 in range(0, lq.shape[0], chunk):
        part = lq[s0:s0 + chunk]
        scores += metrics.calculate_psnr(part if scale == 1 else imresize(part, scale), gt[s0:s0 + chunk], crop_border, test_y_channel)
    return scores


def niqe_scores(frames, params, crop_border=0, chunk=8):
    """NIQE per frame of (t, 3, H, W) float32 RGB frames on the device, `chunk` frames per launch."""
    from edvr_amd import metrics
    scores = []
    for s0 in range(0, frames.shape[0], chunk):
        scores += metrics.calculate_niqe(frames[s0:s0 + chunk], crop_border, params=params)
    return scores


def bicubic_niqe(lq, gt, params, hr_in=False, crop_border=0, chunk=8):
    """NIQE per frame of what bicubic_baseline scores: the bicubic enlargement of `lq` to the size of `gt` (the LQ frames when hr_in)."""
    from edvr_amd.data import imresize
    scale = 1 if hr_in else gt.shape[-1] // lq.shape[-1]
    scores = []
    for s0 in range(0, lq.shape[0], chunk):
        part = lq[s0:s0 + chunk]
        scores += niqe_scores(part if scale == 1 else imresize(part, scale), params, crop_border, chunk)
    return scores


def evaluate(args, log=print):
    from edvr_amd import EDVR, dist as D, metrics
    from edvr_amd.data import VideoTestClips
    from edvr_amd.optim import load_network
    rank, world = D.get_dist_info() if torch.distributed.is_initialized() else D.init_dist()
    device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', 0)))
    torch.cuda.set_device(device)
    net = EDVR(num_in_ch=3, num_out_ch=3, num_feat=args.num_feat, num_frame=args.num_frame, deformable_groups=8,
               num_extract_block=5, num_reconstruct_block=args.num_reconstruct_block, center_frame_idx=None, hr_in=args.hr_in,
               with_predeblur=args.with_predeblur, with_tsa=not args.no_tsa).to(device).eval()
    if args.weights:
        load_network(net, args.weights, strict=True)
    opt = dict(dataroot_gt=args.gt, dataroot_lq=args.lq, io_backend=dict(type='disk'), num_frame=args.num_frame,
               padding=args.padding, name=args.name, cache_data=True)
    lq_from_gt, baseline = getattr(args, 'lq_from_gt', None), getattr(args, 'bicubic_baseline', False)
    degradation = getattr(args, 'degradation', None) or 'bi'
    if args.lq is None:
        if not lq_from_gt:
            raise ValueError('either an LQ folder or lq_from_gt is needed')
        opt['lq_from_gt'] = dict(scale=lq_from_gt, quantize=True) if degradation == 'bi' else dict(scale=lq_from_gt, degradation=degradation)
        if getattr(args, 'jpeg_quality', None) is not None:
            opt['lq_from_gt'].update(jpeg_quality=args.jpeg_quality, jpeg_subsampling=getattr(args, 'jpeg_subsampling', None) or '420')
        if getattr(args, 'mpeg_qscale', None) is not None:  # each folder coded whole as one clip, between blur / noise and the JPEG round trip
            opt['lq_from_gt'].update(mpeg_qscale=args.mpeg_qscale, mpeg_gop=getattr(args, 'mpeg_gop', 12), mpeg_search=getattr(args, 'mpeg_search', 7))
        if getattr(args, 'degrade', None) is not None:  # blur and noise on the 8-bit LQ frames, before the JPEG round trip
            opt['lq_from_gt'].update(degrade=args.degrade, degrade_seed=getattr(args, 'degrade_seed', 0))
    ds = VideoTestClips(opt, device=device)
    # frames of any size (--pad-mode / --tile / --tile-overlap / --tile-blend): passed on only where given
    any_size = {k: (tuple(v) if k == 'tile' else v) for k in ('pad_mode', 'tile', 'tile_overlap', 'tile_blend')
                for v in [getattr(args, k, None)] if v is not None}
    if getattr(args, 'scene_cuts', None) is not None:  # --scene-cuts [THR]: folders that hold more than one shot
        any_size.update(cuts='auto', cut_threshold=float(args.scene_cuts))
    ensemble, reverse = getattr(args, 'self_ensemble', None), bool(getattr(args, 'time_reverse', False))
    # what the second pass runs, and how it is called in the report
    plus_kw = {**({'self_ensemble': ensemble} if ensemble else {}), **({'time_reverse': True} if reverse else {})}
    label = '+'.join(([ensemble] if ensemble else []) + (['time-reverse'] if reverse else []))
    results, base, plus = {}, {}, {}
    niqe_path = getattr(args, 'niqe', None)
    niqe_params = metrics.load_niqe_params(niqe_path) if niqe_path else None
    niqe, niqe_base, niqe_plus = {}, {}, {}
    for folder in ds.folders[rank::world]:
        lq, gt = ds.clip(folder)
        out, psnr = metrics.validate_video(net, lq, gt, num_frame=args.num_frame, padding=args.padding, chunk=args.batch,
                                         crop_border=args.crop_border, test_y_channel=args.test_y_channel, **any_size)
        results[folder] = (sum(psnr), len(psnr))
        if niqe_params is not None:
            q = niqe_scores(out, niqe_params, args.crop_border, args.batch)
            niqe[folder] = (sum(q), len(q))
        if plus_kw:
            out, p = metrics.validate_video(net, lq, gt, num_frame=args.num_frame, padding=args.padding, chunk=args.batch,
                                          crop_border=args.crop_border, test_y_channel=args.test_y_channel, **plus_kw, **any_size)
            plus[folder] = (sum(p), len(p))
            if niqe_params is not None:
                q = niqe_scores(out, niqe_params, args.crop_border, args.batch)
                niqe_plus[folder] = (sum(q), len(q))
        del out
        if baseline:
            b = bicubic_baseline(lq, gt, args.hr_in, args.crop_border, args.test_y_channel, args.batch)
            base[folder] = (sum(b), len(b))
            if niqe_params is not None:
                q = bicubic_niqe(lq, gt, niqe_params, args.hr_in, args.crop_border, args.batch)
                niqe_base[folder] = (sum(q), len(q))
        ds._cache.pop(folder, None)  # one clip resident at a time

    def merged(parts):
        if world > 1:
            gathered = [None] * world
            torch.distributed.all_gather_object(gathered, parts)
            parts = {}
            for part in gathered:
                for k, (s, n) in part.items():
                    s0, n0 = parts.get(k, (0.0, 0))
                    parts[k] = (s0 + s, n0 + n)
        return {k: s / max(n, 1) for k, (s, n) in sorted(parts.items())}

    summary, base = merged(results), merged(base) if baseline else {}
    plus = merged(plus) if plus_kw else {}
    with_niqe = niqe_params is not None
    niqe = merged(niqe) if with_niqe else {}
    niqe_base = merged(niqe_base) if with_niqe and baseline else {}
    niqe_plus = merged(niqe_plus) if with_niqe and plus_kw else {}

    def mean(d):
        return sum(d.values()) / max(len(d), 1)

    if rank == 0:
        beside = (lambda v: f' (bicubic {v:.4f} dB)') if baseline else (lambda v: '')
        with_plus = (lambda v: f', self-ensemble {label} {v:.4f} dB') if plus_kw else (lambda v: '')
        nan = float('nan')

        def niqe_part(q, qp, qb):  # the NIQEs in the order of the PSNRs: model, second pass, baseline
            if not with_niqe:
                return ''
            return (f'; NIQE {q:.4f}' + (f', self-ensemble {label} {qp:.4f}' if plus_kw else '') + (f' (bicubic {qb:.4f})' if baseline else ''))

        for k, v in summary.items():
            log(f'{k}: PSNR {v:.4f} dB' + with_plus(plus.get(k, nan)) + beside(base.get(k, nan)) +
                niqe_part(niqe.get(k, nan), niqe_plus.get(k, nan), niqe_base.get(k, nan)))
        if summary:  # the average of the per-folder averages
            log(f'average over {len(summary)} folder(s): {sum(summary.values()) / len(summary):.4f} dB' +
                with_plus(sum(plus.values()) / max(len(plus), 1)) + beside(sum(base.values()) / max(len(base), 1)) +
                niqe_part(mean(niqe), mean(niqe_plus), mean(niqe_base)))
        if getattr(args, 'json', None):
            import json
            record = {'psnr': summary, 'average': sum(summary.values()) / max(len(summary), 1),
                      'degradation': degradation if args.lq is None else None}  # None: the LQ folder's, whatever made it
            if args.lq is None and getattr(args, 'mpeg_qscale', None) is not None:
                record.update(mpeg_qscale=args.mpeg_qscale, mpeg_gop=getattr(args, 'mpeg_gop', 12), mpeg_search=getattr(args, 'mpeg_search', 7))
            if args.lq is None and getattr(args, 'jpeg_quality', None) is not None:
                record.update(jpeg_quality=args.jpeg_quality, jpeg_subsampling=getattr(args, 'jpeg_subsampling', None) or '420')
            if args.lq is None and getattr(args, 'degrade', None) is not None:
                record.update(degrade=args.degrade, degrade_seed=getattr(args, 'degrade_seed', 0))
            if plus_kw:
                record.update(self_ensemble=ensemble, self_ensemble_psnr=plus, self_ensemble_average=sum(plus.values()) / max(len(plus), 1))
                if reverse:
                    record.update(time_reverse=True)
            if baseline:
                record.update(bicubic_psnr=base, bicubic_average=sum(base.values()) / max(len(base), 1))
            if with_niqe:
                record.update(niqe=niqe, niqe_average=mean(niqe))
                if plus_kw:
                    record.update(self_ensemble_niqe=niqe_plus, self_ensemble_niqe_average=mean(niqe_plus))
                if baseline:
                    record.update(bicubic_niqe=niqe_base, bicubic_niqe_average=mean(niqe_base))
            with open(args.json, 'w') as f:
                json.dump(record, f, indent=1)
    return summary


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--lq', default=None, help='LQ folder; optional with --lq-from-gt')
    ap.add_argument('--lq-from-gt', type=int, default=None, metavar='SCALE',
                    help='make the LQ frames from the GT frames on the device: MATLAB bicubic reduction by SCALE, 8-bit (GT mod-cropped to SCALE)')
    ap.add_argument('--degradation', choices=('bi', 'bd'), default='bi',
                    help="with --lq-from-gt: bi = MATLAB bicubic, 8-bit; bd = DUF's Gaussian blur and subsampling, float (SCALE 2, 3 or 4)")
    ap.add_argument('--jpeg-quality', type=int, default=None, metavar='Q',
                    help='with --lq-from-gt: the 8-bit LQ frames go through a baseline JPEG round trip at quality Q (1..100)')
    ap.add_argument('--jpeg-subsampling', choices=('420', '444'), default='420', help='chroma subsampling of --jpeg-quality')
    ap.add_argument('--mpeg-qscale', type=int, default=None, metavar='Q',
                    help='with --lq-from-gt: code the 8-bit LQ frames of each folder, one clip read whole, with the MPEG-style I / P round trip at '
                         'quantiser scale Q (1..31; edvr_amd.ops.mpeg_roundtrip), after blur and noise and before the JPEG round trip')
    ap.add_argument('--mpeg-gop', type=int, default=12, metavar='N', help='with --mpeg-qscale: an intra frame every N frames (0: the first alone)')
    ap.add_argument('--mpeg-search', type=int, default=7, metavar='R', help='with --mpeg-qscale: the motion search range, 0..15')
    ap.add_argument('--blur-sigma', type=float, nargs='+', default=None, metavar='S',
                    help='with --lq-from-gt: Gaussian blur of the 8-bit LQ frames (edvr_amd.ops.degrade, before the JPEG round trip): SX, or SX SY THETA')
    ap.add_argument('--blur-size', type=int, default=None, metavar='K', help='with --blur-sigma: the kernel size, odd, 3..21 (default: 3 sigma each side)')
    ap.add_argument('--noise-sigma', type=float, default=None, metavar='S', help='with --lq-from-gt: read noise, standard deviation in levels of 0..255')
    ap.add_argument('--noise-shot', type=float, default=None, metavar='A', help='with --lq-from-gt: shot noise, variance per level')
    ap.add_argument('--noise-gray', action='store_true', help='one noise draw for the three channels of a pixel')
    ap.add_argument('--degrade-seed', type=int, default=0, metavar='N', help='the 64-bit key of the noise fields')
    ap.add_argument('--bicubic-baseline', action='store_true', help='also report the PSNR of the bicubic enlargement of the LQ frames')
    ap.add_argument('--niqe', default=None, metavar='PARAMS.npz',
                    help="also report the no-reference NIQE of every output; PARAMS.npz is BasicSR's basicsr/metrics/niqe_pris_params.npz")
    ap.add_argument('--json', default=None, metavar='FILE', help='write the per-folder and average results there')
    ap.add_argument('--gt', required=True)
    ap.add_argument('--weights', default=None)
    ap.add_argument('--name', default='REDS4', help='REDS4 | Vid4 | REDSofficial (folder layout of VideoTestDataset)')
    ap.add_argument('--num-feat', type=int, default=128)
    ap.add_argument('--num-reconstruct-block', type=int, default=40)
    ap.add_argument('--num-frame', type=int, default=5)
    ap.add_argument('--hr-in', action='store_true')
    ap.add_argument('--with-predeblur', action='store_true')
    ap.add_argument('--no-tsa', action='store_true')
    ap.add_argument('--padding', default='reflection_circle')
    ap.add_argument('--crop-border', type=int, default=0)
    ap.add_argument('--test-y-channel', action='store_true')
    ap.add_argument('--batch', type=int, default=8, help='output frames per pass (VideoRestorer chunk)')
    ap.add_argument('--pad-mode', default=None, choices=['reflect', 'replicate'],
                    help='frames of any size: extend them at the bottom and right to the size multiple (4; 16 with --hr-in), crop the output')
    ap.add_argument('--tile', type=int, nargs=2, default=None, metavar=('TH', 'TW'), help='restore tile by tile (input pixels, multiples of the size multiple)')
    ap.add_argument('--tile-overlap', type=int, default=None, help='input pixels neighbouring tiles share (default 8 x the size multiple)')
    ap.add_argument('--tile-blend', type=int, default=None, metavar='N',
                    help='with --tile: cross-fade neighbouring tiles over N input pixels around each cut (a multiple of twice the size multiple, '
                         'at most the overlap)')
    ap.add_argument('--self-ensemble', default=None, choices=['flip4', 'd4'],
                    help='also restore under the 4 flips / the 8 symmetries of the square and average; reported beside the plain PSNR (n x the time)')
    ap.add_argument('--scene-cuts', type=float, nargs='?', const=10.0, default=None, metavar='THR',
                    help="find scene cuts in every clip (VideoRestorer's cuts='auto': a frame whose scene score reaches THR, default 10, "
                         'begins a shot) and restore every shot as a video of its own')
    ap.add_argument('--time-reverse', action='store_true',
                    help='also restore the video in reversed frame order and average (x2; composes with --self-ensemble); reported beside the '
                         'plain PSNR')
    args = ap.parse_args(argv)
    if (args.lq is None) == (args.lq_from_gt is None):
        ap.error('give exactly one of --lq and --lq-from-gt')
    if args.lq_from_gt is not None and not 1 <= args.lq_from_gt <= 8:
        ap.error('--lq-from-gt takes a scale in 1..8')
    if args.mpeg_qscale is not None and (args.lq_from_gt is None or not 1 <= args.mpeg_qscale <= 31):
        ap.error('--mpeg-qscale takes a quantiser scale in 1..31 and needs --lq-from-gt')
    if args.mpeg_gop < 0 or not 0 <= args.mpeg_search <= 15:
        ap.error('--mpeg-gop must not be negative, --mpeg-search is an integer in 0..15')
    if args.jpeg_quality is not None and (args.lq_from_gt is None or not 1 <= args.jpeg_quality <= 100):
        ap.error('--jpeg-quality takes a quality in 1..100 and needs --lq-from-gt')
    from edvr_amd.data import degrade_options
    try:
        args.degrade = degrade_options(args.blur_sigma, args.blur_size, args.noise_sigma, args.noise_shot, args.noise_gray)
    except ValueError as e:
        ap.error(str(e))
    if args.degrade is not None and args.lq_from_gt is None:
        ap.error('--blur-sigma, --noise-sigma and --noise-shot need --lq-from-gt')
    if args.tile_blend is not None and args.tile is None:
        ap.error('--tile-blend needs --tile')
    if args.degradation == 'bd' and args.lq_from_gt not in (2, 3, 4):
        ap.error('--degradation bd needs --lq-from-gt 2, 3 or 4')
    return args


def main():
    evaluate(parse_args())


if __name__ == '__main__':
    main()
