"""Whole-video restoration: the windowed path (metrics.validate_clip: every frame's features once per window it appears in) against
VideoRestorer (once per frame), same seeded video, same chunk / batch, one process, arms alternated.

    python scripts/bench_video.py --config L_T5            # EDVR-L, 5 frames, 100 frames of 180x320, chunk 10
    python scripts/bench_video.py --config L_T7
    python scripts/bench_video.py --config L_deblur        # hr_in + predeblur, 720x1280
    python scripts/bench_video.py --config L_T5 --out-dtype uint8

Per arm: frames/s (median over the repeats) with the spread, peak device memory, and the per-kernel table of ONE restore (events
around every launch through ops.LAUNCH_HOOK: the gather's and the uint8 tail's share is a number).  Prints one JSON line and merges
it into --json (default profiles/video/bench_video.json) under the configuration's name.

Frames of any size (VideoRestorer pad_mode / tile), same method, merged into profiles/video/bench_video_tiles.json:

    python scripts/bench_video.py --leg pad --config L_T5 [--out-dtype uint8]   # 270x480: pad_mode='reflect' against host F.pad + slice
    python scripts/bench_video.py --leg pad --config L_deblur                   # 1080x1920
    python scripts/bench_video.py --leg tiles --config L_T5                     # 544x960 untiled against 2x2 tiles, time and peak memory
    python scripts/bench_video.py --leg seam --config L_T5                      # |tiled - untiled| near and away from the cuts, per overlap
    python scripts/bench_video.py --leg large --config L_T5                     # peak memory against frame area, extrapolated

Self-ensemble (VideoRestorer self_ensemble), same method, merged into profiles/video/bench_video_ensemble.json:

    python scripts/bench_video.py --self-ensemble flip4 --config L_T5 [--out-dtype uint8]   # frames/s against the plain path (~ 1 / n)
    python scripts/bench_video.py --self-ensemble d4 --config L_T5                          # and the new kernels' share of kernel time

Tile blending (VideoRestorer tile_blend), same method, merged into profiles/video/bench_video_blend.json:

    python scripts/bench_video.py --tile-blend 32 --config L_T5 [--out-dtype uint8]   # 544x960, 2x2 tiles: blended against unblended tiles,
                                                                                      # the blend tails' share, the seam table both ways

Temporal reversal (VideoRestorer time_reverse), same method, merged into profiles/video/bench_video_time.json:

    python scripts/bench_video.py --time-reverse --config L_T5 [--self-ensemble flip4]   # plain against both arms (share_alignment True /
                                                                                         # False): frames/s, peak memory, the pair kernel's share

Scene cuts (VideoRestorer cuts), merged into profiles/video/bench_video_cuts.json:

    python scripts/bench_video.py --scene-cuts --config L_T5   # ops.frame_sad alone (time, share of the HBM rate); a restore streamed in
                                                               # pieces of 8 with cuts=None, cuts='auto' on the same cut-free video and
                                                               # cuts='auto' on a video with a cut every 25 frames: frames/s, host waits
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

CONFIGS = {
    # name: (EDVR keywords, (h, w), frames, chunk, per-frame share of the windowed FLOPs per output frame or None)
    'L_T5': (dict(num_feat=128, num_frame=5, num_reconstruct_block=40, center_frame_idx=None), (180, 320), 100, 10, (905.0, 4231.0)),
    'L_T7': (dict(num_feat=128, num_frame=7, num_reconstruct_block=40, center_frame_idx=None), (180, 320), 100, 10, (1267.0, 5251.0)),
    'L_deblur': (dict(num_feat=128, num_frame=5, num_reconstruct_block=40, center_frame_idx=None, hr_in=True, with_predeblur=True),
                 (720, 1280), 100, 4, None),
    'toy': (dict(num_feat=64, num_frame=5, num_reconstruct_block=4, center_frame_idx=None), (32, 48), 12, 4, None),
}


def kernel_table(run):
    from edvr_amd import ops
    records = []

    def hook(name, flops, launch, nbytes, executed=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        records.append((name, flops, e0, e1))

    ops.LAUNCH_HOOK = hook
    try:
        run()
        torch.cuda.synchronize()
    finally:
        ops.LAUNCH_HOOK = None
    per = {}
    for name, flops, e0, e1 in records:
        d = per.setdefault(name, [0, 0.0, 0.0])
        d[0] += 1
        d[1] += e0.elapsed_time(e1)
        d[2] += flops
    total = sum(d[1] for d in per.values())
    rows = sorted(per.items(), key=lambda kv: -kv[1][1])
    return {'kernel_ms': round(total, 3), 'gflop': round(sum(d[2] for d in per.values()) * 1e-9, 1),
            'kernels': [{'name': k, 'launches': d[0], 'ms': round(d[1], 3), 'share': round(d[1] / total, 4)} for k, d in rows]}


RECT_KERNELS = ('crop_pad_frames', 'upsample4x_add_rect', 'upsample4x_add_u8_rect', 'f32_to_u8_hwc_rect', 'copy_rect')
LEG_HW = {'pad': {'L_T5': (270, 480), 'L_T7': (270, 480), 'L_deblur': (1080, 1920), 'toy': (30, 46)},
          'tiles': {'L_T5': (544, 960), 'L_T7': (544, 960), 'L_deblur': (2176, 3840), 'toy': (64, 96)}}


def _build_net(kwargs, dev):
    from edvr_amd import EDVR
    torch.manual_seed(10)
    net = EDVR(**kwargs).eval()
    g = torch.Generator().manual_seed(123)
    with torch.no_grad():  # sub-pixel offsets instead of the all-zero default init (as main() below)
        for name, p in net.named_parameters():
            if name.endswith('conv_offset.weight'):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            elif name.endswith('conv_offset.bias'):
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    return net.to(dev)


def _two_arms(arms, frames, repeats, net):
    """The measurement of main() for two callables: warm-up, peak memory of one run, `repeats` alternated timed runs, kernel tables."""
    res = {k: {'s': []} for k in arms}
    outs = {}
    for k, fn in arms.items():
        fn()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        outs[k] = fn()
        torch.cuda.synchronize()
        res[k]['peak_mem_mb'] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    for _ in range(repeats):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            res[k]['s'].append(e0.elapsed_time(e1) * 1e-3)
    net.check_offsets()
    for k, fn in arms.items():
        tab = kernel_table(fn)
        res[k]['kernel_ms'] = tab['kernel_ms']
        res[k]['crop_and_rect_store_ms'] = round(sum(r['ms'] for r in tab['kernels'] if r['name'] in RECT_KERNELS), 3)
        res[k]['crop_and_rect_store_share'] = round(res[k]['crop_and_rect_store_ms'] / tab['kernel_ms'], 5)
        res[k]['gather_share'] = round(sum(r['ms'] for r in tab['kernels'] if r['name'] == 'gather_images') / tab['kernel_ms'], 5)
        res[k]['launches'] = sum(r['launches'] for r in tab['kernels'])
    net.check_offsets()
    for r in res.values():
        sec = r.pop('s')
        r['seconds'] = [round(v, 4) for v in sec]
        r['frames_per_s'] = round(frames / statistics.median(sec), 3)
        r['spread'] = round((max(sec) - min(sec)) / statistics.median(sec), 4)
    return res, outs


def leg_pad(args, net, kwargs, dev, frames, chunk):
    """pad_mode='reflect' against the caller-side way: F.pad of the float frames, the plain restore, slice + .contiguous()."""
    import torch.nn.functional as F
    from edvr_amd import VideoRestorer
    h, w = LEG_HW['pad'][args.config]
    m, s = (16, 1) if kwargs.get('hr_in') else (4, 4)
    hp, wp = -(-h // m) * m, -(-w // m) * m
    dt = getattr(torch, args.out_dtype)
    lq = torch.rand(frames, 3, h, w, generator=torch.Generator().manual_seed(0)).to(dev)
    plain = VideoRestorer(net, padding=args.padding, chunk=chunk, out_dtype=dt)
    padded = VideoRestorer(net, padding=args.padding, chunk=chunk, out_dtype=dt, pad_mode='reflect')

    def host_pad():
        out = plain.restore(F.pad(lq, (0, wp - w, 0, hp - h), mode='reflect'))
        return (out[:, :s * h, :s * w] if dt == torch.uint8 else out[..., :s * h, :s * w]).contiguous()

    res, outs = _two_arms({'host_pad': host_pad, 'pad_mode': lambda: padded.restore(lq)}, frames, args.repeats, net)
    ratio = res['pad_mode']['frames_per_s'] / res['host_pad']['frames_per_s']
    return {'leg': 'pad', 'hw': [h, w], 'padded_hw': [hp, wp], 'bit_identical': bool(torch.equal(outs['host_pad'], outs['pad_mode'])),
            'ratio_pad_mode_over_host_pad': round(ratio, 4), 'not_slower_beyond_parent_spread': bool(ratio >= 1.0 - res['host_pad']['spread']),
            **res}


def _default_2x2(h, w, m):
    """Tile of a 2 x 2 grid at the default overlap of 8 m: two tiles per axis sharing exactly the overlap."""
    ov = 8 * m
    return (-(-(h + ov) // (2 * m)) * m, -(-(w + ov) // (2 * m)) * m), ov


def leg_tiles(args, net, kwargs, dev, frames, chunk):
    from edvr_amd import VideoRestorer, tile_grid
    h, w = LEG_HW['tiles'][args.config]
    m = 16 if kwargs.get('hr_in') else 4
    tile, ov = _default_2x2(h, w, m)
    grid = tile_grid(h, w, tile, None, m)
    assert len(grid) == 4, grid
    dt = getattr(torch, args.out_dtype)
    lq = torch.rand(frames, 3, h, w, generator=torch.Generator().manual_seed(0)).to(dev)
    plain = VideoRestorer(net, padding=args.padding, chunk=chunk, out_dtype=dt)
    tiled = VideoRestorer(net, padding=args.padding, chunk=chunk, out_dtype=dt, tile=tile)
    # (the tiled arm first: the kernels' grow-only workspaces (ops.workspace) stay allocated, and the untiled arm's larger ones would
    # otherwise be booked on the tiled arm's peak)
    res, outs = _two_arms({'tiled': lambda: tiled.restore(lq), 'untiled': lambda: plain.restore(lq)}, frames, args.repeats, net)
    area = sum(t.src[2] * t.src[3] for t in grid) / float(-(-h // m) * m * (-(-w // m) * m))
    t_ratio = res['untiled']['frames_per_s'] / res['tiled']['frames_per_s']
    return {'leg': 'tiles', 'hw': [h, w], 'tile': list(tile), 'tile_overlap': ov, 'tiles': len(grid),
            'derived_time_ratio_sum_of_tile_areas_over_frame_area': round(area, 4), 'measured_time_ratio_tiled_over_untiled': round(t_ratio, 4),
            'kernel_time_ratio_tiled_over_untiled': round(res['tiled']['kernel_ms'] / res['untiled']['kernel_ms'], 4),
            'peak_memory_ratio_tiled_over_untiled': round(res['tiled']['peak_mem_mb'] / res['untiled']['peak_mem_mb'], 4), **res}


def leg_seam(args, net, kwargs, dev, frames, chunk):
    """max / mean |tiled - untiled| relative to the output scale inside a band of `overlap` output pixels around the cuts and outside
    it, per overlap.  Weights: random init with sub-pixel offsets - NOT a trained model's; input: structured synthetic motion."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
    from util_edvr import motion_frames
    from edvr_amd import VideoRestorer, tile_grid
    m, s = (16, 1) if kwargs.get('hr_in') else (4, 4)
    h, w = (256, 384) if args.config != 'toy' else (96, 128)
    frames = min(frames, 12)
    lq = motion_frames(1, (frames, 3, h, w), seed=0)[0].to(dev)
    ref = VideoRestorer(net, padding=args.padding, chunk=chunk).restore(lq)
    scale = ref.abs().max().item()
    rows = []
    for ov in (0, 2 * m, 8 * m, 16 * m):
        tile = (-(-(h + ov) // (2 * m)) * m, -(-(w + ov) // (2 * m)) * m)
        grid = tile_grid(h, w, tile, ov, m)
        out = VideoRestorer(net, padding=args.padding, chunk=chunk, tile=tile, tile_overlap=ov).restore(lq)
        d = (out - ref).abs() / scale
        band = torch.zeros(s * h, s * w, dtype=torch.bool, device=dev)
        width = max(ov, 2 * m) * s  # (overlap 0: a band of 2 m, or there would be nothing to report)
        for t in grid:
            oy, ox = t.dst
            if oy > 0:
                band[max(s * oy - width, 0):s * oy + width] = True
            if ox > 0:
                band[:, max(s * ox - width, 0):s * ox + width] = True
        inside, outside = d[..., band], d[..., ~band]
        rows.append({'overlap': ov, 'tile': list(tile), 'tiles': len(grid), 'band_output_pixels': width,
                     'band_max': inside.max().item(), 'band_mean': inside.mean().item(),
                     'outside_max': outside.max().item() if outside.numel() else None,  # (a toy frame can be all band)
                     'outside_mean': outside.mean().item() if outside.numel() else None})
    net.check_offsets()
    return {'leg': 'seam', 'hw': [h, w], 'frames': frames, 'weights': 'random init, conv_offset N(0, 0.02) / bias N(0, 0.5): not a trained model',
            'input': 'util_edvr.motion_frames', 'output_scale': scale, 'overlaps': rows}


def leg_large(args, net, kwargs, dev, frames, chunk):
    """Peak memory of a chunk-1 restore of 7 frames against the frame area, untiled and 2 x 2 tiles, on sizes far from the limit; a
    line through the points gives the largest frame that fits.  Nothing is run near the limit."""
    from edvr_amd import VideoRestorer
    m = 16 if kwargs.get('hr_in') else 4
    sizes = [(180, 320), (360, 640), (544, 960)] if args.config != 'toy' else [(64, 96), (96, 144), (128, 192)]
    total = torch.cuda.get_device_properties(dev).total_memory
    pts = {'untiled': [], 'tiled': []}
    for h, w in sizes:
        lq = torch.rand(7, 3, h, w, generator=torch.Generator().manual_seed(0)).to(dev)
        for key in pts:
            kw = {'tile': _default_2x2(h, w, m)[0]} if key == 'tiled' else {}
            vr = VideoRestorer(net, padding=args.padding, chunk=1, out_dtype=torch.uint8, **kw)
            vr.restore(lq)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            vr.restore(lq)
            torch.cuda.synchronize()
            pts[key].append([h * w, round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)])
        del lq
    net.check_offsets()

    def line(p):  # through the two largest points: MB = a + b * area
        (x0, y0), (x1, y1) = p[-2], p[-1]
        b = (y1 - y0) / (x1 - x0)
        return y0 - b * x0, b
    out = {'leg': 'large', 'frames': 7, 'chunk': 1, 'device_memory_mb': round(total / 2 ** 20, 1), 'points_area_peak_mb': pts}
    budget = 0.85 * total / 2 ** 20
    for key in pts:
        a, b = line(pts[key])
        out[key + '_mb_per_megapixel'] = round(b * 1e6, 1)
        out[key + '_largest_lq_megapixels_at_85_percent_of_memory_extrapolated'] = round((budget - a) / b * 1e-6, 3)
    a, b = line(pts['tiled'])
    area4 = 4e6 * out['untiled_largest_lq_megapixels_at_85_percent_of_memory_extrapolated']
    out['tiled_2x2_peak_mb_at_4x_the_largest_untiled_area_extrapolated'] = round(a + b * area4, 1)
    out['fits'] = bool(a + b * area4 < budget)
    return out


D4_KERNELS = ('crop_pad_frames_d4', 'upsample4x_add_rect_d4', 'upsample4x_add_u8_rect_d4', 'f32_to_u8_hwc_rect_d4', 'copy_rect_d4')


def leg_ensemble(args, net, kwargs, dev, frames, chunk):
    """self_ensemble against the plain VideoRestorer at the same chunk: frames/s (expected about 1 / n), peak memory, and the share of
    kernel time spent in the oriented reads and accumulating tails of csrc/ensemble.hip."""
    from edvr_amd import VideoRestorer, ensemble_elements
    h, w = CONFIGS[args.config][1]
    dt = getattr(torch, args.out_dtype)
    elements = ensemble_elements(args.self_ensemble)
    lq = torch.rand(frames, 3, h, w, generator=torch.Generator().manual_seed(0)).to(dev)
    plain = VideoRestorer(net, padding=args.padding, chunk=chunk, out_dtype=dt)
    plus = VideoRestorer(net, padding=args.padding, chunk=chunk, out_dtype=dt, self_ensemble=elements)
    res, outs = _two_arms({'ensemble': lambda: plus.restore(lq), 'plain': lambda: plain.restore(lq)}, frames, args.repeats, net)
    tab = kernel_table(lambda: plus.restore(lq))
    net.check_offsets()
    new_ms = sum(r['ms'] for r in tab['kernels'] if r['name'] in D4_KERNELS)
    diff = (outs['ensemble'].float() - outs['plain'].float()).abs().max().item()
    ratio = res['ensemble']['frames_per_s'] / res['plain']['frames_per_s']
    return {'leg': 'ensemble', 'hw': [h, w], 'self_ensemble': args.self_ensemble, 'elements': list(elements), 'banks': len(plus.pairs),
            'ratio_ensemble_over_plain_frames_per_s': round(ratio, 4), 'expected_ratio_one_over_n': round(1.0 / len(elements), 4),
            'new_kernels_ms': round(new_ms, 3), 'new_kernels_share_of_kernel_time': round(new_ms / tab['kernel_ms'], 5),
            'new_kernels': [r for r in tab['kernels'] if r['name'] in D4_KERNELS],
            'max_abs_difference_to_plain_output': diff, **res}


BLEND_KERNELS = ('upsample4x_add_rect_blend', 'upsample4x_add_u8_rect_blend', 'f32_to_u8_hwc_rect_blend', 'copy_rect_blend')


def _seam_rows(out, ref, scale, cuts_y, cuts_x, width):
    """leg_seam's numbers: max / mean |out - ref| / scale inside a band of `width` output pixels either side of the cuts, and outside."""
    d = (out.float() - ref.float()).abs() / scale
    band = torch.zeros(d.shape[-2], d.shape[-1], dtype=torch.bool, device=d.device)
    for c in cuts_y:
        band[max(c - width, 0):c + width] = True
    for c in cuts_x:
        band[:, max(c - width, 0):c + width] = True
    inside, outside = d[..., band], d[..., ~band]
    return {'band_output_pixels': width, 'band_max': inside.max().item(), 'band_mean': inside.mean().item(),
            'outside_max': outside.max().item() if outside.numel() else None, 'outside_mean': outside.mean().item() if outside.numel() else None}


def leg_blend(args, net, kwargs, dev, frames, chunk):
    """tile_blend against the unblended tiled path with the SAME tiles (2 x 2 at the default overlap, the frame of --leg tiles): frames/s,
    peak memory, the share of kernel time in the blend tails, and - float32 output - leg_seam's table for both against the untiled
    result of a shorter structured video.  Blending adds no network launch: the expectation is a ratio of 1 within the arms' spread."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
    from util_edvr import motion_frames
    from edvr_amd import VideoRestorer, tile_grid
    h, w = LEG_HW['tiles'][args.config]
    m, s = (16, 1) if kwargs.get('hr_in') else (4, 4)
    tile, ov = _default_2x2(h, w, m)
    grid = tile_grid(h, w, tile, None, m)
    dt = getattr(torch, args.out_dtype)
    lq = torch.rand(frames, 3, h, w, generator=torch.Generator().manual_seed(0)).to(dev)
    cut = VideoRestorer(net, padding=args.padding, chunk=chunk, out_dtype=dt, tile=tile)
    blended = VideoRestorer(net, padding=args.padding, chunk=chunk, out_dtype=dt, tile=tile, tile_blend=args.tile_blend)
    res, outs = _two_arms({'blended': lambda: blended.restore(lq), 'unblended': lambda: cut.restore(lq)}, frames, args.repeats, net)
    tab = kernel_table(lambda: blended.restore(lq))
    net.check_offsets()
    new_ms = sum(r['ms'] for r in tab['kernels'] if r['name'] in BLEND_KERNELS)
    ratio = res['blended']['frames_per_s'] / res['unblended']['frames_per_s']
    del outs, lq
    seam = None
    if dt == torch.float32:  # the seam table of leg_seam: a short structured video, against the untiled result
        n = min(frames, 12)
        mv = motion_frames(1, (n, 3, h, w), seed=0)[0].to(dev)
        ref = VideoRestorer(net, padding=args.padding, chunk=chunk).restore(mv)
        scale = ref.abs().max().item()
        cuts_y = sorted({s * t.dst[0] for t in grid if t.dst[0] > 0})
        cuts_x = sorted({s * t.dst[1] for t in grid if t.dst[1] > 0})
        seam = {'frames': n, 'input': 'util_edvr.motion_frames', 'output_scale': scale,
                'weights': 'random init, conv_offset N(0, 0.02) / bias N(0, 0.5): not a trained model',
                'unblended': _seam_rows(cut.restore(mv), ref, scale, cuts_y, cuts_x, s * ov),
                'blended': _seam_rows(blended.restore(mv), ref, scale, cuts_y, cuts_x, s * ov)}
        net.check_offsets()
    return {'leg': 'blend', 'hw': [h, w], 'tile': list(tile), 'tile_overlap': ov, 'tile_blend': args.tile_blend, 'tiles': len(grid),
            'ratio_blended_over_unblended_frames_per_s': round(ratio, 4),
            'within_unblended_spread': bool(ratio >= 1.0 - res['unblended']['spread']),
            'kernel_time_ratio_blended_over_unblended': round(res['blended']['kernel_ms'] / res['unblended']['kernel_ms'], 4),
            'blend_tails_ms': round(new_ms, 3), 'blend_tails_share_of_kernel_time': round(new_ms / tab['kernel_ms'], 5),
            'blend_tails': [r for r in tab['kernels'] if r['name'] in BLEND_KERNELS], 'seam': seam, **res}


def leg_time(args, net, kwargs, dev, frames, chunk):
    """time_reverse, both arms (share_alignment True / False), against the VideoRestorer without it at the same chunk and the same
    spatial ensemble: frames/s (the unshared arm: expected about 1 / 2 of that), peak memory, and the share of the shared arm's kernel
    time spent in the attention kernel with two outputs."""
    from edvr_amd import VideoRestorer
    h, w = CONFIGS[args.config][1]
    dt = getattr(torch, args.out_dtype)
    base = dict(padding=args.padding, chunk=chunk, out_dtype=dt, **({'self_ensemble': args.self_ensemble} if args.self_ensemble else {}))
    lq = torch.rand(frames, 3, h, w, generator=torch.Generator().manual_seed(0)).to(dev)
    plain = VideoRestorer(net, **base)
    shared = VideoRestorer(net, time_reverse=True, **base)
    unshared = VideoRestorer(net, time_reverse=True, share_alignment=False, **base)
    res, outs = _two_arms({'shared': lambda: shared.restore(lq), 'unshared': lambda: unshared.restore(lq), 'plain': lambda: plain.restore(lq)},
                          frames, args.repeats, net)
    tab = kernel_table(lambda: shared.restore(lq))
    net.check_offsets()
    pair_ms = sum(r['ms'] for r in tab['kernels'] if r['name'] == 'tsa_temporal_pair')
    fps = {k: res[k]['frames_per_s'] for k in res}
    gain = fps['shared'] / fps['unshared']
    return {'leg': 'time', 'hw': [h, w], 'self_ensemble': args.self_ensemble,
            'ratio_unshared_over_plain_frames_per_s': round(fps['unshared'] / fps['plain'], 4),
            'ratio_shared_over_plain_frames_per_s': round(fps['shared'] / fps['plain'], 4),
            'ratio_shared_over_unshared_frames_per_s': round(gain, 4),
            'shared_faster_beyond_plain_spread': bool(gain - 1.0 > res['plain']['spread']),
            'kernel_time_ratio_shared_over_unshared': round(res['shared']['kernel_ms'] / res['unshared']['kernel_ms'], 4),
            'arms_bit_identical': bool(torch.equal(outs['shared'], outs['unshared'])),
            'pair_kernel_ms': round(pair_ms, 3), 'pair_kernel_share_of_kernel_time': round(pair_ms / tab['kernel_ms'], 5),
            'max_abs_difference_to_plain_output': (outs['shared'].float() - outs['plain'].float()).abs().max().item(), **res}


HBM_MEASURED_TBS = 6.29  # the rate the copy benchmark of this project reaches on an MI355X


def _moving_texture(n, h, w, seed, dev, k=17):
    """One shot: a smooth random texture seen through a window that moves one pixel down and right per frame, float32 (n, 3, h, w)."""
    import torch.nn.functional as F
    base = torch.rand(1, 3, h + n + k - 1, w + n + k - 1, generator=torch.Generator().manual_seed(seed)).to(dev)
    x = F.pad(base, (k // 2,) * 4, mode='reflect')
    x = F.avg_pool2d(F.avg_pool2d(x, k, stride=1), k, stride=1)
    x = (x - x.min()) / (x.max() - x.min())
    return torch.stack([x[0, :, t:t + h, t:t + w] for t in range(n)]).contiguous()


def _time_frame_sad(make, copies, launches=200):
    """Mean time of one ops.frame_sad call (the clear of the result and the kernel) over `launches` calls that walk through `copies`
    distinct inputs - more bytes than the caches hold, so that every call reads its frames from memory."""
    from edvr_amd import ops
    bufs = [make(i) for i in range(copies)]
    out = torch.empty(bufs[0].shape[0], dtype=torch.int64, device=bufs[0].device)
    for b in bufs[:4]:
        ops.frame_sad(b, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(launches):
        ops.frame_sad(bufs[i % copies], out=out)
    e1.record()
    e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / launches
    n, per = bufs[0].shape[0], bufs[0][0].numel() * bufs[0].element_size()
    once, asked = n * per, 2 * (n - 1) * per  # every frame once; what the n - 1 pairs load (each inner frame twice, the second time from a cache)
    return {'shape': list(bufs[0].shape), 'dtype': str(bufs[0].dtype).replace('torch.', ''), 'distinct_inputs': copies, 'launches': launches,
            'microseconds': round(us, 2), 'bytes_each_frame_once': once, 'bytes_loaded': asked,
            'share_of_hbm_rate_each_frame_once': round(once / (us * 1e-6) / (HBM_MEASURED_TBS * 1e12), 4),
            'share_of_hbm_rate_bytes_loaded': round(asked / (us * 1e-6) / (HBM_MEASURED_TBS * 1e12), 4)}


def leg_cuts(args, net, kwargs, dev, frames, chunk):
    """Scene cuts: ops.frame_sad on its own, and what cuts='auto' costs a streamed restore - (a) cuts=None, (b) cuts='auto' on the same
    cut-free video (the detector's whole cost: its launches and the host's waits), (c) cuts='auto' on a video with a cut every 25 frames
    (the short chunks at the shots' ends on top).  Pieces of 8 frames, the arms alternated, median and spread of `repeats` runs."""
    import time
    from edvr_amd import VideoRestorer
    h, w = CONFIGS[args.config][1]
    g = torch.Generator().manual_seed(0)
    sad = {'f32_8x3x180x320': _time_frame_sad(lambda i: torch.rand(8, 3, 180, 320, generator=g).to(dev), 64),
           'u8_8x720x1280x3': _time_frame_sad(lambda i: torch.randint(0, 256, (8, 720, 1280, 3), generator=g, dtype=torch.uint8).to(dev), 24)}
    one_shot = _moving_texture(frames, h, w, 100, dev)
    shot = 25
    several = torch.cat([_moving_texture(min(shot, frames - a), h, w, 200 + a, dev) for a in range(0, frames, shot)])
    want_cuts = list(range(shot, frames, shot)) if frames % shot == 0 or frames % shot >= kwargs['num_frame'] else None
    base = dict(padding=args.padding, chunk=chunk, out_dtype=getattr(torch, args.out_dtype))
    plain, auto = VideoRestorer(net, **base), VideoRestorer(net, cuts='auto', **base)
    waited = [0.0]
    wait_sad = auto._wait_sad

    def timed_wait(host, event):
        t0 = time.perf_counter()
        v = wait_sad(host, event)
        waited[0] += time.perf_counter() - t0
        return v

    auto._wait_sad = timed_wait

    def stream(vr, lq):
        def run():
            for out in vr.restore_chunks(lq.split(8)):
                del out
        return run

    arms = {'a_cuts_none': stream(plain, one_shot), 'b_auto_no_cut': stream(auto, one_shot), 'c_auto_cut_every_25': stream(auto, several)}
    res = {k: {'s': [], 'host_wait_s': []} for k in arms}
    for k, fn in arms.items():  # warm-up, and what the detector found
        fn()
        torch.cuda.synchronize()
        if k != 'a_cuts_none':
            res[k]['cuts_found'] = list(auto.cuts_found)
            res[k]['largest_score_off_the_cuts'] = round(max(s for i, s in enumerate(auto.cut_scores) if i not in auto.cuts_found), 3)
            if auto.cuts_found:
                res[k]['smallest_score_at_a_cut'] = round(min(auto.cut_scores[i] for i in auto.cuts_found), 3)
    assert res['b_auto_no_cut']['cuts_found'] == [], res['b_auto_no_cut']
    assert want_cuts is None or res['c_auto_cut_every_25']['cuts_found'] == want_cuts, res['c_auto_cut_every_25']
    for _ in range(args.repeats):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            waited[0] = 0.0
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            res[k]['s'].append(e0.elapsed_time(e1) * 1e-3)
            res[k]['host_wait_s'].append(round(waited[0], 4))
    net.check_offsets()
    for r in res.values():
        sec = r.pop('s')
        r['seconds'] = [round(v, 4) for v in sec]
        r['frames_per_s'] = round(frames / statistics.median(sec), 3)
        r['spread'] = round((max(sec) - min(sec)) / statistics.median(sec), 4)
    res['a_cuts_none'].pop('host_wait_s')
    a, b, c = (res[k]['frames_per_s'] for k in ('a_cuts_none', 'b_auto_no_cut', 'c_auto_cut_every_25'))
    return {'leg': 'cuts', 'hw': [h, w], 'piece': 8, 'hbm_measured_tbs': HBM_MEASURED_TBS, 'frame_sad': sad,
            'detector_cost_b_over_a': round(1.0 - b / a, 4), 'detector_cost_beyond_spread_of_a': bool(1.0 - b / a > res['a_cuts_none']['spread']),
            'short_chunks_cost_c_over_a': round(1.0 - c / a, 4), **res}


def main_leg(args):
    from edvr_amd import _lib
    from edvr_amd.build import source_hash
    kwargs, _, frames, chunk, _ = CONFIGS[args.config]
    frames, chunk = args.frames or frames, args.chunk or chunk
    dev = torch.device('cuda:0')
    net = _build_net(kwargs, dev)
    with torch.no_grad():
        legs = {'pad': leg_pad, 'tiles': leg_tiles, 'seam': leg_seam, 'large': leg_large, 'ensemble': leg_ensemble, 'blend': leg_blend,
                'time': leg_time, 'cuts': leg_cuts}
        result = legs[args.leg](args, net, kwargs, dev, frames, chunk)
    result = {'config': args.config, 'edvr': dict(kwargs), 'frames': frames, 'chunk': chunk, 'padding': args.padding, 'out_dtype': args.out_dtype,
              'repeats': args.repeats, **result, 'csrc_sha16': source_hash(), 'library': _lib.lib().edvr_version().decode(),
              'device': torch.cuda.get_device_name(0)}
    default = {'ensemble': 'bench_video_ensemble.json', 'blend': 'bench_video_blend.json',
               'time': 'bench_video_time.json', 'cuts': 'bench_video_cuts.json'}.get(args.leg, 'bench_video_tiles.json')
    path = os.path.abspath(args.json or os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'video', default))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    merged = json.load(open(path)) if os.path.exists(path) else {}
    key = (f'{args.self_ensemble}_{args.config}' if args.leg == 'ensemble' else f'blend{args.tile_blend}_{args.config}' if args.leg == 'blend'
           else f'time_{args.self_ensemble}_{args.config}' if args.leg == 'time' and args.self_ensemble else f'{args.leg}_{args.config}')
    merged[key + ('' if args.out_dtype == 'float32' else '_' + args.out_dtype)] = result
    with open(path, 'w') as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(result))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='L_T5', choices=sorted(CONFIGS))
    ap.add_argument('--frames', type=int, default=None)
    ap.add_argument('--chunk', type=int, default=None)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--padding', default='reflection_circle')
    ap.add_argument('--out-dtype', default='float32', choices=['float32', 'uint8'])
    ap.add_argument('--json', default=None, help='default: profiles/video/bench_video.json (bench_video_tiles.json with --leg)')
    ap.add_argument('--leg', default=None, choices=['pad', 'tiles', 'seam', 'large'], help='frames of any size: pad_mode / tile measurements')
    ap.add_argument('--self-ensemble', default=None, choices=['flip4', 'd4'],
                    help='timing arm: self_ensemble against the plain VideoRestorer (profiles/video/bench_video_ensemble.json)')
    ap.add_argument('--tile-blend', type=int, default=None, metavar='N',
                    help='timing arm: tile_blend=N against the unblended tiled path, same 2 x 2 tiles (profiles/video/bench_video_blend.json)')
    ap.add_argument('--time-reverse', action='store_true',
                    help='timing arm: time_reverse (both share_alignment arms) against the VideoRestorer without it, with --self-ensemble on '
                         'top of that ensemble (profiles/video/bench_video_time.json)')
    ap.add_argument('--scene-cuts', action='store_true',
                    help="ops.frame_sad on its own, and a streamed restore with cuts=None against cuts='auto' without and with cuts "
                         '(profiles/video/bench_video_cuts.json)')
    args = ap.parse_args(argv)
    if args.scene_cuts:
        if args.leg or args.self_ensemble or args.time_reverse or args.tile_blend is not None:
            ap.error('--scene-cuts is a leg of its own: give it without --leg / --self-ensemble / --time-reverse / --tile-blend')
        args.leg = 'cuts'
        return args
    if args.tile_blend is not None:
        if args.leg or args.self_ensemble or args.time_reverse:
            ap.error('--tile-blend is a leg of its own: give it without --leg / --self-ensemble / --time-reverse')
        args.leg = 'blend'
    if args.time_reverse:
        if args.leg:
            ap.error('--time-reverse is a leg of its own: give it without --leg (it composes with --self-ensemble)')
        args.leg = 'time'
    elif args.self_ensemble:
        if args.leg:
            ap.error('--self-ensemble is a leg of its own: give it without --leg')
        args.leg = 'ensemble'
    return args


def main():
    args = parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_video.py measures on the GPU: none found')
    if args.leg:
        return main_leg(args)
    args.json = args.json or os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'video', 'bench_video.json')
    from edvr_amd import EDVR, VideoRestorer, _lib, metrics
    from edvr_amd.build import source_hash
    kwargs, (h, w), frames, chunk, share = CONFIGS[args.config]
    frames, chunk = args.frames or frames, args.chunk or chunk
    dev = torch.device('cuda:0')
    torch.manual_seed(10)
    net = EDVR(**kwargs).eval()
    g = torch.Generator().manual_seed(123)
    with torch.no_grad():  # default init zeroes conv_offset: every tap on the integer grid; give the offsets sub-pixel values instead
        for name, p in net.named_parameters():
            if name.endswith('conv_offset.weight'):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            elif name.endswith('conv_offset.bias'):
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    net = net.to(dev)
    lq = torch.rand(frames, 3, h, w, generator=torch.Generator().manual_seed(0)).to(dev)
    t = kwargs['num_frame']
    out_dtype = getattr(torch, args.out_dtype)
    vr = VideoRestorer(net, padding=args.padding, chunk=chunk, out_dtype=out_dtype)

    def windowed():
        return metrics.validate_clip(net, lq, num_frame=t, padding=args.padding, batch=chunk)[0]

    def video():
        return vr.restore(lq)

    arms = {'windowed': windowed, 'video': video}
    res = {k: {'s': []} for k in arms}
    with torch.no_grad():
        outs = {}
        for k, fn in arms.items():  # warm-up: every shape of the timed window; peak memory of one restore
            fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            outs[k] = fn()
            torch.cuda.synchronize()
            res[k]['peak_mem_mb'] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
        if out_dtype == torch.float32:
            diff = (outs['video'] - outs['windowed']).abs().max().item() / outs['windowed'].abs().max().item()
        else:
            ref = (outs['windowed'].clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1)
            diff = (outs['video'].int() - ref.int()).abs().max().item()
        del outs
        for _ in range(args.repeats):  # alternate the arms: drift of the shared machine hits both alike
            for k, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                res[k]['s'].append(e0.elapsed_time(e1) * 1e-3)
        net.check_offsets()
        for k, fn in arms.items():
            res[k]['table'] = kernel_table(fn)
        net.check_offsets()
    for k, r in res.items():
        s = r.pop('s')
        r['seconds'] = [round(v, 4) for v in s]
        r['frames_per_s'] = round(frames / statistics.median(s), 3)
        r['spread'] = round((max(s) - min(s)) / statistics.median(s), 4)  # (max - min) / median over the repeats
    ratio = res['video']['frames_per_s'] / res['windowed']['frames_per_s']
    tab = res['video']['table']
    glue = sum(k['ms'] for k in tab['kernels'] if k['name'] in ('gather_images', 'upsample4x_add_u8', 'f32_to_u8_hwc'))
    result = {'config': args.config, 'edvr': {k: v for k, v in kwargs.items()}, 'hw': [h, w], 'frames': frames, 'chunk': chunk,
              'padding': args.padding, 'out_dtype': args.out_dtype, 'repeats': args.repeats, 'speedup': round(ratio, 4),
              'flop_ceiling': round(share[1] / (share[1] - share[0] * (t - 1) / t), 4) if share else None,
              'measured_flop_ratio': round(res['windowed']['table']['gflop'] / max(tab['gflop'], 1e-9), 4),
              'faster_beyond_spread': bool(ratio - 1.0 > res['windowed']['spread']),
              'gather_and_u8_share_of_video_kernel_time': round(glue / tab['kernel_ms'], 5),
              'max_output_difference': diff, 'windowed': res['windowed'], 'video': res['video'],
              'csrc_sha16': source_hash(), 'library': _lib.lib().edvr_version().decode(), 'device': torch.cuda.get_device_name(0)}
    for r in (result['windowed'], result['video']):
        r['table']['kernels'] = r['table']['kernels'][:14]  # the table's head; the shares are of the whole
    path = os.path.abspath(args.json)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    merged = json.load(open(path)) if os.path.exists(path) else {}
    merged[args.config + ('' if args.out_dtype == 'float32' else '_' + args.out_dtype)] = result
    with open(path, 'w') as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
