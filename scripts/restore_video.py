"""Restore a video that has no ground truth: YUV4MPEG2 in, YUV4MPEG2 out, `-` for stdin / stdout.

    ffmpeg -i in.mp4 -f yuv4mpegpipe - | python scripts/restore_video.py - - --weights EDVR_L_x4_SR_REDS_official.pth | ffmpeg -i - out.mp4
    python scripts/restore_video.py in.y4m out.y4m --weights ... --pad-mode reflect --tile 256 256 --self-ensemble flip4
    ffmpeg -i hevc10.mp4 -strict -1 -f yuv4mpegpipe - | python scripts/restore_video.py - - --weights ... | ffmpeg -i - out.mkv
    ffmpeg -i in.mp4 -f yuv4mpegpipe - | python scripts/restore_video.py - - --weights ... --out-format 420p10 | ffmpeg -i - out.mkv
    ffmpeg -i tape.avi -f yuv4mpegpipe - | python scripts/restore_video.py - - --weights ... --deinterlace | ffmpeg -i - out.mp4
    ffmpeg -i dvd.vob -f yuv4mpegpipe - | python scripts/restore_video.py - - --weights ... --deinterlace film --out-height 1080 --square-pixels | ffmpeg -i - out.mp4

`--out-size WxH`, `--out-height N` or `--out-width N` deliver the result at that size instead of 4 W x 4 H: the float32 frames are
resampled on the device (edvr_amd.ops.resample; `--resample lanczos3|bicubic|bilinear`) before the one quantisation, so no
scaler behind the pipe quantises them again and the pipe carries the delivered bytes only.  With `--square-pixels` the sample aspect (the
A tag) is folded into the size and A1:1 is written: a 720 x 480 A32:27 disc at `--out-height 1080` leaves as 1920 x 1080; without it the A
tag is corrected for the rounding, so the display aspect stays.

`--crop auto` drops letterbox / pillarbox bars on the device, on the bytes as decoded, before the network pays for them
(edvr_amd.ops.bar_profile / yuv_crop): the rect is decided on the first `--crop-probe` frames that are not blank, aligned
inward to the chroma steps and the network's size multiple, and everything after - the restorer, `--out-height`, the matrix defaults -
sees the picture alone; the A tag is kept.  `--crop W:H:X:Y` (ffmpeg's order) gives the rect; `scripts/detect_bars.py IN` prints one
for a whole stream, for films whose picture grows after the first minute.  `--bars-json FILE` writes what was found.

Interlaced input (It / Ib: tape, DVD, 1080i) needs `--deinterlace`: the fields are deinterlaced on the device (edvr_amd.ops.deinterlace,
DESIGN 4.19) before anything else sees them and every field becomes a frame - the output is progressive at twice the frame rate;
`--deinterlace frame` keeps the rate (one frame per input frame, from its first field).  `--field-order tff|bff` overrides a wrong
tag; the default `auto` follows the header and passes a progressive stream through untouched.  `--deinterlace film` is for film shown
as video (NTSC DVDs, broadcast captures: 24000/1001 frames/s stretched to 60000/1001 fields/s by 2:3 pulldown): the fields of every film
frame are woven back together, bit for bit, and the repeated frame of every five is dropped (edvr_amd.y4m.inverse_telecined) -
the output is progressive at 4 / 5 of the frame rate; `--no-decimate` keeps every frame and the rate, `--film-json FILE` writes every
frame's match, the frames that had no clean match (deinterlaced from one field instead: many of them mean video, use `field`) and the
dropped frames with their scores.

The input is 4:2:0, 4:2:2 or 4:4:4 at 8 ... 16 bits (C420jpeg, C422p10, C444p12 ...: 10-bit phone and camera footage, 4:2:2 intermediates
and 4:4:4 screen captures go in as they are - ffmpeg's yuv4mpegpipe muxer writes anything but 8-bit 4:2:0 only with `-strict -1`, and
no `-pix_fmt yuv420p` in front of the pipe throws bits or chroma away).  `--out-format NAME` picks the output's format (default: the
input's): `420p10` or `444p10` on 8-bit input quantises the network's float32 result once, to 10 bits, which keeps skies and gradients
free of the banding that 8 bits add.

edvr_amd.y4m.restore_y4m: the frames go to the device as the decoder wrote them, are converted to RGB there (edvr_amd.ops.yuv420_to_rgb;
ops.yuv_to_rgb for every other format), restored by VideoRestorer with every frame's features extracted once, converted back
(ops.rgb_to_yuv420 / ops.rgb_to_yuv) and written as they arrive - bounded memory, no intermediate files, one quantisation.  The network options are those of scripts/eval_video.py, `--batch` is the
number of output frames per pass; `--matrix-in` / `--matrix-out` default to the player rule for each side's own size (BT.709 from 1280
columns or 577 rows, BT.601 below; `bt2020nc` - BT.2020 non-constant luminance, what 10-bit UHD / HDR footage is - is given by name), `--chroma`
picks the chroma upsampling filter of the decode.  `--siting` says where the input's chroma samples lie: `center` (the default: JPEG / MPEG-1),
`left` (H.264, HEVC and AV1 4:2:0, every 4:2:2), `topleft` (BT.2020 / UHD) or `auto` - the stream's tag (C420jpeg / C420mpeg2 / C420paldv) and
`left` where the tag is silent.  `--siting auto` is right for nearly all decoded video: read with the wrong siting, the colour lands half an
input pixel - two output pixels - beside the luma.  `--siting-out` is the siting the output is encoded for (default: the input's); 8-bit 4:2:0
output carries it in its tag, for every other format tell the encoder (ffmpeg: `-chroma_sample_location left` on the output side).  The
transfer function (gamma, PQ, HLG) is never touched: the network sees R'G'B' as coded.  `--niqe PARAMS.npz` scores the result with
the no-reference NIQE (metrics.calculate_niqe against BasicSR's niqe_pris_params.npz; lower is better) on the float32 frames before they
are converted back, and the decoded input at its own size beside it where at least two 96 x 96 blocks fit; `--niqe-json FILE` writes
both lists.  `--scene-cuts [THR]` finds hard cuts (VideoRestorer's cuts='auto': ffmpeg's scene score on the 0 ... 255 scale, default 10) and
restores every shot as a video of its own, so that no frame's window mixes two scenes; `--min-shot N` bounds the shot length from below,
`--cuts I [I ...]` gives the cuts instead, `--cuts-json FILE` writes the cuts, every frame's mafd and score, the threshold and min_shot.
Everything this script prints goes to stderr: stdout may be the video.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def restore(args, log=log):
    import torch
    from edvr_amd import EDVR
    from edvr_amd.optim import load_network
    from edvr_amd import metrics, ops
    from edvr_amd.bars import crop_string
    from edvr_amd.y4m import ALL_FORMATS, FRAME, Y4MReader, default_matrix, resolve_field_order, resolve_siting, restore_y4m
    device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', 0)))
    torch.cuda.set_device(device)
    net = EDVR(num_in_ch=3, num_out_ch=3, num_feat=args.num_feat, num_frame=args.num_frame, deformable_groups=8,
               num_extract_block=5, num_reconstruct_block=args.num_reconstruct_block, center_frame_idx=None, hr_in=args.hr_in,
               with_predeblur=args.with_predeblur, with_tsa=not args.no_tsa).to(device).eval()
    if args.weights:
        load_network(net, args.weights, strict=True)
    kwargs = {k: (tuple(v) if k == 'tile' else v) for k in ('pad_mode', 'tile', 'tile_overlap', 'tile_blend', 'self_ensemble')
              for v in [getattr(args, k, None)] if v is not None}
    if getattr(args, 'time_reverse', False):
        kwargs['time_reverse'] = True
    kwargs.update(cut_kwargs(args))
    stats = {}
    src = sys.stdin.buffer if args.input == '-' else open(args.input, 'rb')
    dst = sys.stdout.buffer if args.output == '-' else open(args.output, 'wb')
    try:
        deint = getattr(args, 'deinterlace', None)
        reader = Y4MReader(src, formats=ALL_FORMATS, interlaced=True) if deint else Y4MReader(src, formats=ALL_FORMATS)
        log(f'{args.input}: {reader.width} x {reader.height}, F{reader.fps}, C{reader.chroma}, {reader.range} range')
        if deint:
            first, _ = resolve_field_order(deint, args.field_order, reader)
            kwargs.update(deinterlace=deint, field_order=args.field_order)
            if deint == 'film':
                kwargs.update(film_decimate=not getattr(args, 'no_decimate', False))
                how = 'pulldown undone' + ('' if kwargs['film_decimate'] else ', every frame kept')
            else:
                how = f'deinterlaced at {deint} rate'
            log(f'{args.input}: I{reader.interlace}, ' + (f'{how}, {first} field first' if first else 'progressive: nothing to deinterlace'))
            deint = first is not None
        siting_in = resolve_siting(getattr(args, 'siting', 'center'), reader)
        siting_out = getattr(args, 'siting_out', None)
        if (siting_in, siting_out) != ('center', None):
            kwargs.update(siting_in=siting_in, siting_out=siting_out)
            log(f'{args.input}: chroma siting {siting_in} in, {resolve_siting(siting_out or siting_in, reader)} out')
        fit = {k: v for k in ('out_size', 'out_height', 'out_width') for v in [getattr(args, k, None)] if v is not None}
        if fit:
            kwargs.update(fit, square_pixels=bool(getattr(args, 'square_pixels', False)), resample=getattr(args, 'resample', 'lanczos3'))
            log(f'{args.output}: delivered at ' + ', '.join(f'{k} {v}' for k, v in fit.items()) + (', square pixels' if kwargs['square_pixels'] else '')
                + f' ({kwargs["resample"]})')
        if getattr(args, 'crop', None) is not None:
            kwargs.update(crop=args.crop, crop_probe=args.crop_probe, crop_limit=args.crop_limit, crop_margin=args.crop_margin)
            log(f'{args.input}: bars ' + (f'detected on the first {args.crop_probe} frames that are not blank (limit {args.crop_limit})'
                                         if args.crop == 'auto' else f'cropped to {crop_string(args.crop)}'))
        niqe_path, niqe_out, niqe_in = getattr(args, 'niqe', None), [], []
        if niqe_path:
            params = metrics.load_niqe_params(niqe_path)
            kwargs['on_chunk'] = lambda chunk: niqe_out.extend(metrics.calculate_niqe(chunk, params=params))
            H, W = reader.height, reader.width
            # (one block leaves no covariance to estimate; woven frames are not what the network sees: a deinterlaced input is not scored)
            if (H // metrics.NIQE_BLOCK) * (W // metrics.NIQE_BLOCK) >= 2 and not deint:
                read, matrix_in = reader.read, args.matrix_in or default_matrix(H, W)

                def scored_read(k):  # the input as restore_y4m decodes it, scored at its own size
                    host = read(k)
                    if host.shape[0]:
                        rgb = ops.yuv_to_rgb(host.to(device, non_blocking=True)[:, len(FRAME):], H, W, reader.format, matrix_in, reader.range,
                                             args.chroma, siting_in)
                        niqe_in.extend(metrics.calculate_niqe(rgb, params=params))
                    return host

                reader.read = scored_read
        t0 = time.time()
        with torch.no_grad():
            n = restore_y4m(net, reader, dst, matrix_in=args.matrix_in, matrix_out=args.matrix_out, chroma=args.chroma,
                            read_frames=args.read_frames, num_frame=args.num_frame, padding=args.padding, chunk=args.batch, stats=stats,
                            out_format=getattr(args, 'out_format', None), **kwargs)
        net.check_offsets()
        torch.cuda.synchronize()
        dt = time.time() - t0
        log(f'{args.output}: {n} frames in {dt:.1f} s ({n / max(dt, 1e-9):.2f} frames/s)')
        if 'cuts' in stats:
            report_cuts(args, stats, log)
        if 'film_matches' in stats:
            report_film(args, stats, log)
        if 'crop' in stats:
            report_bars(args, stats, log)
        if niqe_path:
            report_niqe(args, niqe_out, niqe_in, log)
    finally:
        if src is not sys.stdin.buffer:
            src.close()
        if dst is not sys.stdout.buffer:
            dst.close()
    return n


def cut_kwargs(args):
    """VideoRestorer's scene-cut arguments from --scene-cuts / --min-shot / --cuts ({} without them)."""
    if getattr(args, 'cuts', None) is not None:
        return {'cuts': list(args.cuts)}
    if getattr(args, 'scene_cuts', None) is None:
        return {}
    out = {'cuts': 'auto', 'cut_threshold': float(args.scene_cuts)}
    if getattr(args, 'min_shot', None) is not None:
        out['min_shot'] = args.min_shot
    return out


def report_film(args, stats, log=log):
    """What inverse telecine decided; with --film-json every frame's match, the combed and the dropped frames with their scores."""
    m = stats['film_matches']
    log(f'{args.input}: {len(m)} frames read, {sum(m)} matched to the frame before, {len(stats["film_dropped"])} dropped, '
        f'{len(stats["film_combed"])} without a clean match' + (f' (frames {stats["film_combed"][:8]} ...)' if stats['film_combed'] else ''))
    if getattr(args, 'film_json', None):
        import json
        record = {'frames_in': len(m), 'frames': stats['frames'], 'matches': ['cp'[v] for v in m], 'combed': stats['film_combed'],
                  'dropped': stats['film_dropped'], 'dropped_scores': stats['film_dropped_scores']}
        with open(args.film_json, 'w') as f:
            json.dump(record, f, indent=1)


def report_bars(args, stats, log=log):
    """The rect a run cropped to; with crop='auto' also the probe's box, the blank frames and - a warning - the frames whose picture reaches
    beyond the rect; with --bars-json all of it."""
    from edvr_amd.bars import crop_string
    rect, outside = stats['crop'], stats.get('bars_outside', [])
    if rect is None:
        log(f'{args.input}: no bars cropped' + (f' (the box {stats["crop_box"]} is under half the frame: not believed)' if stats.get('crop_box') else ''))
    else:
        log(f'{args.input}: cropped to {crop_string(rect)} (W:H:X:Y)' + (f', {len(stats["bars_blank"])} blank frames' if stats.get('bars_blank') else ''))
    if outside:
        log(f'{args.input}: WARNING: the picture of {len(outside)} frames (from frame {outside[0]}) reaches beyond the rect - it grew after the '
            f'probe; run scripts/detect_bars.py on the whole stream and give its rect with --crop')
    if getattr(args, 'bars_json', None):
        import json
        record = {'frames': stats['frames'], 'crop': None if rect is None else crop_string(rect), 'rect': rect, 'box': stats.get('crop_box'),
                  'blank': stats.get('bars_blank', []), 'outside': outside}
        with open(args.bars_json, 'w') as f:
            json.dump(record, f, indent=1)


def report_cuts(args, stats, log=log):
    """The cuts a run found or was given; with --cuts-json the cuts, every frame's mafd and score, the threshold and min_shot."""
    cuts = stats['cuts']
    log(f'{args.input}: {len(cuts) + 1} shot(s) in {stats["frames"]} frames, cuts at {cuts}')
    if getattr(args, 'cuts_json', None):
        import json
        auto = getattr(args, 'cuts', None) is None
        record = {'frames': stats['frames'], 'cuts': cuts, 'mafd': stats['cut_mafd'], 'score': stats['cut_scores'],
                  'threshold': float(args.scene_cuts) if auto else None,
                  'min_shot': (args.min_shot if args.min_shot is not None else max(args.num_frame, 2))}
        with open(args.cuts_json, 'w') as f:
            json.dump(record, f, indent=1)


def report_niqe(args, niqe_out, niqe_in, log=log):
    """Mean and per-frame NIQE of the output, and of the decoded input where it was scored; the same as JSON with --niqe-json."""
    def mean(v):
        return sum(v) / len(v) if v else float('nan')

    log(f'{args.output}: NIQE {mean(niqe_out):.4f} over {len(niqe_out)} frames  [' + ' '.join(f'{v:.3f}' for v in niqe_out) + ']')
    if niqe_in:
        log(f'{args.input}: NIQE {mean(niqe_in):.4f} over {len(niqe_in)} frames  [' + ' '.join(f'{v:.3f}' for v in niqe_in) + ']')
    else:
        log(f'{args.input}: not scored (fewer than two 96 x 96 blocks fit its frames)')
    if getattr(args, 'niqe_json', None):
        import json
        record = {'output': {'niqe': niqe_out, 'average': mean(niqe_out)}, 'input': {'niqe': niqe_in, 'average': mean(niqe_in)} if niqe_in else None}
        with open(args.niqe_json, 'w') as f:
            json.dump(record, f, indent=1)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Restore a YUV4MPEG2 video with EDVR (4:2:0, 4:2:2 or 4:4:4 at 8 ... 16 bits in and out).')
    ap.add_argument('input', metavar='IN', help='Y4M file, or - for stdin')
    ap.add_argument('output', metavar='OUT', help='Y4M file, or - for stdout')
    ap.add_argument('--weights', default=None)
    ap.add_argument('--num-feat', type=int, default=128)
    ap.add_argument('--num-reconstruct-block', type=int, default=40)
    ap.add_argument('--num-frame', type=int, default=5)
    ap.add_argument('--hr-in', action='store_true')
    ap.add_argument('--with-predeblur', action='store_true')
    ap.add_argument('--no-tsa', action='store_true')
    ap.add_argument('--padding', default='reflection_circle')
    ap.add_argument('--batch', type=int, default=8, help='output frames per pass (VideoRestorer chunk)')
    ap.add_argument('--read-frames', type=int, default=8, help='frames per read and per copy to the device')
    ap.add_argument('--pad-mode', default=None, choices=['reflect', 'replicate'],
                    help='frames of any size: extend them at the bottom and right to the size multiple (4; 16 with --hr-in), crop the output')
    ap.add_argument('--tile', type=int, nargs=2, default=None, metavar=('TH', 'TW'), help='restore tile by tile (input pixels, multiples of the size multiple)')
    ap.add_argument('--tile-overlap', type=int, default=None, help='input pixels neighbouring tiles share (default 8 x the size multiple)')
    ap.add_argument('--tile-blend', type=int, default=None, metavar='N',
                    help='with --tile: cross-fade neighbouring tiles over N input pixels around each cut')
    ap.add_argument('--self-ensemble', default=None, choices=['flip4', 'd4'],
                    help='restore under the 4 flips / the 8 symmetries of the square and average (n x the time)')
    ap.add_argument('--time-reverse', action='store_true', help='also restore the video in reversed frame order and average (x2)')
    ap.add_argument('--matrix-in', default=None, choices=['bt601', 'bt709', 'bt2020nc'], help="the input's matrix (default: by its size)")
    ap.add_argument('--matrix-out', default=None, choices=['bt601', 'bt709', 'bt2020nc'], help="the output's matrix (default: by ITS size)")
    ap.add_argument('--chroma', default='bilinear', choices=['bilinear', 'nearest'], help='chroma upsampling of the decode')
    ap.add_argument('--siting', default='center', choices=['center', 'left', 'topleft', 'auto'],
                    help="where the input's chroma samples lie; auto: by the stream's tag, left where it is silent (recommended for decoded video)")
    ap.add_argument('--siting-out', default=None, choices=['center', 'left', 'topleft', 'auto'],
                    help="the siting the output is encoded for (default: the input's)")
    ap.add_argument('--out-format', default=None, metavar='NAME',
                    help="the output's format: 420 | 422 | 444 with an optional depth p9 ... p16, e.g. 420p10 (default: the input's)")
    ap.add_argument('--out-size', default=None, metavar='WxH', help='deliver at exactly this size (resampled on the device before the one quantisation)')
    ap.add_argument('--out-height', type=int, default=None, metavar='N', help='deliver N rows; the width follows the frame (and, with --square-pixels, its A tag)')
    ap.add_argument('--out-width', type=int, default=None, metavar='N', help='deliver N columns; the height follows')
    ap.add_argument('--square-pixels', action='store_true',
                    help='with --out-height / --out-width: fold the sample aspect (A tag) into the size and write A1:1 - a 720 x 480 A32:27 disc at '
                         '--out-height 1080 leaves as 1920 x 1080')
    ap.add_argument('--resample', default='lanczos3', choices=['lanczos3', 'bicubic', 'bilinear'], metavar='NAME',
                    help='the filter of the delivery resampling: lanczos3 (default), bicubic or bilinear')
    ap.add_argument('--crop', default=None, metavar='auto|W:H:X:Y',
                    help="drop letterbox / pillarbox bars on the device before anything else sees them: auto - detected on the first frames; "
                         "W:H:X:Y - that rect, in ffmpeg's crop order (scripts/detect_bars.py prints one for a whole stream)")
    ap.add_argument('--crop-probe', type=int, default=48, metavar='N', help='with --crop auto: decide on the first N frames that are not blank')
    ap.add_argument('--crop-limit', type=int, default=24, metavar='L',
                    help='with --crop auto: a row or column whose mean luma does not exceed the 8-bit level L is dark (default 24)')
    ap.add_argument('--crop-margin', type=int, default=0, metavar='G', help='with --crop auto: G more samples off every side that has a bar')
    ap.add_argument('--bars-json', default=None, metavar='FILE', help='with --crop: write the rect, the box, the blank and the outside frames there')
    ap.add_argument('--deinterlace', nargs='?', const='field', default=None, choices=['field', 'frame', 'film'],
                    help='deinterlace an interlaced stream (It / Ib) on the device first: field - every field becomes a frame, the rate doubles '
                         '(the default of a bare --deinterlace); frame - one frame per input frame, from its first field; film - undo 2:3 '
                         'pulldown: matching fields are woven back into film frames and the repeated frame of every 5 is dropped')
    ap.add_argument('--no-decimate', action='store_true', help='with --deinterlace film: keep every frame and the frame rate')
    ap.add_argument('--film-json', default=None, metavar='FILE', help='with --deinterlace film: write the matches, combed and dropped frames there')
    ap.add_argument('--field-order', default='auto', choices=['auto', 'tff', 'bff'],
                    help="with --deinterlace: auto - the stream's tag, a progressive stream passes through; tff / bff - deinterlace whatever the tag says")
    ap.add_argument('--niqe', default=None, metavar='PARAMS.npz',
                    help="score the output (and the input, where two 96 x 96 blocks fit) with NIQE; PARAMS.npz is BasicSR's niqe_pris_params.npz")
    ap.add_argument('--niqe-json', default=None, metavar='FILE', help='with --niqe: write the per-frame and mean NIQE there')
    ap.add_argument('--scene-cuts', type=float, nargs='?', const=10.0, default=None, metavar='THR',
                    help='find scene cuts and restore every shot as a video of its own: a frame whose scene score (ffmpeg\'s, 0 ... 255 scale) '
                         'reaches THR (default 10) begins a shot')
    ap.add_argument('--min-shot', type=int, default=None, metavar='N',
                    help='with --scene-cuts: no shot shorter than N frames (default and lower bound: max(--num-frame, 2))')
    ap.add_argument('--cuts', type=int, nargs='+', default=None, metavar='I', help='the cuts themselves: frame I begins a new shot')
    ap.add_argument('--cuts-json', default=None, metavar='FILE',
                    help='with --scene-cuts or --cuts: write the cuts, every frame\'s mafd and score, the threshold and min_shot there')
    args = ap.parse_args(argv)
    if args.out_format is not None:
        from edvr_amd.ops import yuv_format
        try:
            args.out_format = yuv_format(args.out_format)[3]
        except ValueError as e:
            ap.error(f'--out-format: {e}')
    if args.out_size is not None:
        w, sep, h = args.out_size.lower().partition('x')
        if not (sep and w.isascii() and h.isascii() and w.isdigit() and h.isdigit() and int(w) > 0 and int(h) > 0):
            ap.error(f'--out-size is WxH, two positive integers, got {args.out_size!r}')
        args.out_size = (int(w), int(h))
    if sum(v is not None for v in (args.out_size, args.out_height, args.out_width)) > 1:
        ap.error('--out-size, --out-height and --out-width exclude each other')
    if any(v is not None and v < 1 for v in (args.out_height, args.out_width)):
        ap.error('--out-height and --out-width are positive')
    if args.square_pixels and args.out_height is None and args.out_width is None:
        ap.error('--square-pixels needs --out-height or --out-width (--out-size states both axes)')
    if args.resample != 'lanczos3' and args.out_size is None and args.out_height is None and args.out_width is None:
        ap.error('--resample needs --out-size, --out-height or --out-width')
    if args.crop is not None and args.crop != 'auto':
        from edvr_amd.bars import parse_crop
        try:
            args.crop = parse_crop(args.crop)
        except ValueError as e:
            ap.error(f'--crop: {e}')
        if args.crop[2] < 1 or args.crop[3] < 1:
            ap.error('--crop: W and H are positive')
    if args.crop != 'auto' and (args.crop_probe != 48 or args.crop_limit != 24 or args.crop_margin != 0):
        ap.error('--crop-probe, --crop-limit and --crop-margin need --crop auto')
    if args.crop_probe < 1 or not 0 <= args.crop_limit <= 255 or args.crop_margin < 0:
        ap.error('--crop-probe is at least 1, --crop-limit an 8-bit level 0 ... 255, --crop-margin at least 0')
    if args.bars_json is not None and args.crop is None:
        ap.error('--bars-json needs --crop')
    if args.cuts is not None and args.scene_cuts is not None:
        ap.error('--cuts and --scene-cuts exclude each other')
    if args.min_shot is not None and args.scene_cuts is None:
        ap.error('--min-shot needs --scene-cuts')
    if args.min_shot is not None and args.min_shot < max(args.num_frame, 2):
        ap.error(f'--min-shot is at least max(--num-frame, 2) = {max(args.num_frame, 2)}')
    if args.cuts_json is not None and args.cuts is None and args.scene_cuts is None:
        ap.error('--cuts-json needs --scene-cuts or --cuts')
    if args.cuts is not None and (args.cuts[0] < 1 or any(b <= a for a, b in zip(args.cuts, args.cuts[1:]))):
        ap.error('--cuts are strictly increasing frame indices, at least 1')
    if args.field_order != 'auto' and args.deinterlace is None:
        ap.error('--field-order needs --deinterlace')
    if (args.no_decimate or args.film_json is not None) and args.deinterlace != 'film':
        ap.error('--no-decimate and --film-json need --deinterlace film')
    if args.niqe_json is not None and args.niqe is None:
        ap.error('--niqe-json needs --niqe')
    if args.tile_blend is not None and args.tile is None:
        ap.error('--tile-blend needs --tile')
    if args.tile_overlap is not None and args.tile is None:
        ap.error('--tile-overlap needs --tile')
    if args.batch < 1 or args.read_frames < 1:
        ap.error('--batch and --read-frames are at least 1')
    if args.input != '-' and args.input == args.output:
        ap.error('IN and OUT are the same file')
    return args


def main():
    restore(parse_args())


if __name__ == '__main__':
    main()
