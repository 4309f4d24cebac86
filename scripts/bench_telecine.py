"""Times ops.field_match and ops.field_weave (csrc/telecine.hip) and the Y4M path with inverse telecine in it.

  (a) ops.field_match and ops.field_weave on 8 frames of 480 x 720 '420', 1080 x 1920 '420' and 1080 x 1920 '422p10', the input inside
      a Y4M buffer (stride framesize + 6, 6 bytes in: how restore_y4m calls them) with dense context frames, the output dense: device
      events around one call (everything the op issues included: field_match's clear of the table, field_weave's copy of its table to
      the device) after warm-up, the median of --iters calls and their spread, and the bytes that must cross HBM - field_match: the luma
      plane of the 8 frames and of the two context frames once, and the table; field_weave: every output byte read once and written once -
      with the share of the 6.29 TB/s measured HBM rate they amount to; beside them, in the same process at the same shape,
      ops.deinterlace(mode='frame') and ops.yuv_to_rgb (bilinear chroma) on the same buffer;
  (b) restore_y4m on an in-memory telecined stream (`It`, 720 x 480, F30000:1001: film frames through 2:3 pulldown; EDVR-L as trained,
      T = 5) with deinterlace='film' against deinterlace='field' on the SAME stream, alternated, three runs each, host clock around
      the call ending in a synchronise: output frames/s and seconds of source per second (input frames over 30000/1001 per second).

    python scripts/bench_telecine.py [--out profiles/telecine/bench_telecine.json] [--skip-video] [--video-frames 10]
"""
import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))

HBM_TBS = 6.29
CASES = [('8x480x720 420', 8, 480, 720, '420'), ('8x1080x1920 420', 8, 1080, 1920, '420'), ('8x1080x1920 422p10', 8, 1080, 1920, '422p10')]
WEAVE_MATCHES = [0, 0, 1, 1, 0, 0, 0, 1]  # what 2:3 pulldown asks for, give or take the phase


def timed(fn, warmup, iters):
    """Median, min, max over `iters` of the device time of fn() in microseconds (events around each call, after `warmup` calls)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times), min(times), max(times)


def twice(fn, args):
    """(median, [both medians], [min, max]): two timed passes, the first ran on a colder device."""
    first, second = timed(fn, args.warmup, args.iters), timed(fn, 5, args.iters)
    return min(first[0], second[0]), [round(first[0], 2), round(second[0], 2)], [round(min(first[1], second[1]), 2), round(max(first[2], second[2]), 2)]


def git_head(tree):
    try:
        return subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=tree, stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def share(nbytes, us):
    return round(nbytes / (us * 1e-6) / (HBM_TBS * 1e12), 4)


def kernel_rows(args, dev):
    from edvr_amd import ops
    rows = []
    for name, n, H, W, fmt in CASES:
        fs = ops.yuv_frame_size(H, W, fmt)
        depth = ops.yuv_format(fmt)[2]
        bps = 2 if depth > 8 else 1
        gen = torch.Generator().manual_seed(0)
        frames = torch.randint(0, 256, (n + 2, fs), generator=gen, dtype=torch.uint8)
        if depth > 8:
            frames[:, 1::2] &= (1 << (depth - 8)) - 1  # little-endian words below 2^depth
        buf = torch.zeros((n, fs + 6), dtype=torch.uint8, device=dev)
        buf[:, 6:] = frames[:n].to(dev)
        yuv, prev, prev2 = buf[:, 6:], frames[n].to(dev), frames[n + 1].to(dev)
        table = torch.empty((n, 7), dtype=torch.int64, device=dev)
        out = torch.empty((n, fs), dtype=torch.uint8, device=dev)
        idx = list(range(n))
        assert torch.equal(ops.field_match(yuv, H, W, fmt, prev=prev, prev2=prev2, out=table), ops.field_match(yuv.contiguous(), H, W, fmt, prev=prev, prev2=prev2))
        assert torch.equal(ops.field_weave(yuv, H, W, fmt, frames=idx, matches=WEAVE_MATCHES, prev=prev, out=out),
                           ops.field_weave(yuv.contiguous(), H, W, fmt, frames=idx, matches=WEAVE_MATCHES, prev=prev))
        dec = timed(lambda: ops.yuv_to_rgb(yuv, H, W, fmt, 'bt709', 'limited'), args.warmup, args.iters)
        dei = timed(lambda: ops.deinterlace(yuv, H, W, fmt, mode='frame', out=out), args.warmup, args.iters)
        ops_ = (('field_match', lambda: ops.field_match(yuv, H, W, fmt, prev=prev, prev2=prev2, out=table), (n + 2) * H * W * bps + n * 56),
                ('field_weave', lambda: ops.field_weave(yuv, H, W, fmt, frames=idx, matches=WEAVE_MATCHES, prev=prev, out=out), 2 * n * fs))
        for op, fn, hbm in ops_:
            med, runs, span = twice(fn, args)
            row = dict(case=name, op=op, frames=n, size=[H, W], format=fmt, us=round(med, 2), us_runs=runs, us_min_max=span, bytes_hbm=hbm,
                       hbm_fraction=share(hbm, med), deinterlace_frame_us=round(dei[0], 2), deinterlace_frame_us_min_max=[round(dei[1], 2), round(dei[2], 2)],
                       over_deinterlace_frame=round(med / dei[0], 3), decode_us=round(dec[0], 2), decode_us_min_max=[round(dec[1], 2), round(dec[2], 2)],
                       over_decode=round(med / dec[0], 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def video_row(args, dev):
    """restore_y4m(deinterlace='film') against deinterlace='field' on one resident telecined 480i stream: EDVR-L, chunk 10."""
    from edvr_amd import EDVR, ops
    from edvr_amd.y4m import restore_y4m
    H, W, n, chunk = 480, 720, args.video_frames, 10
    torch.manual_seed(10)
    net = EDVR(num_feat=128, num_frame=5, num_reconstruct_block=40, center_frame_idx=None).to(dev).eval()
    fs = ops.yuv420_frame_size(H, W)
    # smooth moving film frames (random samples would make the network's offsets run away) through 2:3 pulldown, top field first
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    fields = [j for j in range(n) for _ in range(3 if j % 2 else 2)][:2 * n]
    film = [((torch.sin((xx + 5 * t) / 17.0) * torch.cos(yy / 23.0) * 90 + 128).clamp(0, 255)).to(torch.uint8) for t in range(max(fields) + 1)]
    frames = torch.full((n, fs), 128, dtype=torch.uint8)
    for i in range(n):
        luma = film[fields[2 * i]].clone()
        luma[1::2] = film[fields[2 * i + 1]][1::2]
        frames[i, :H * W] = luma.reshape(-1)
    woven = f'YUV4MPEG2 W{W} H{H} F30000:1001 It A10:11 C420jpeg\n'.encode() + b''.join(b'FRAME\n' + f.numpy().tobytes() for f in frames)
    n_film = n - n // 5

    def run(mode):
        src, dst, stats = io.BytesIO(woven), io.BytesIO(), {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = restore_y4m(net, src, dst, chunk=chunk, read_frames=chunk, deinterlace=mode, stats=stats)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert got == (n_film if mode == 'film' else 2 * n)
        return got / dt, n * 1001 / 30000 / dt, stats

    with torch.no_grad():
        _, _, stats = run('film')
        run('field')
        film_runs, field_runs = [], []
        for _ in range(3):
            field_runs.append(run('field')[:2])
            film_runs.append(run('film')[:2])
    net.check_offsets()
    med = lambda runs, k: round(statistics.median(r[k] for r in runs), 4)
    row = dict(case='EDVR-L T5 telecined 480i (720 x 480)', frames_in=n, chunk=chunk, film_frames_out=n_film, field_frames_out=2 * n,
               film_matches=''.join('cp'[m] for m in stats['film_matches']), film_combed=stats['film_combed'], film_dropped=stats['film_dropped'],
               film_fps_runs=[round(r[0], 3) for r in film_runs], field_fps_runs=[round(r[0], 3) for r in field_runs],
               film_fps=med(film_runs, 0), field_fps=med(field_runs, 0), film_source_seconds_per_second=med(film_runs, 1),
               field_source_seconds_per_second=med(field_runs, 1),
               film_over_field_source_rate=round(statistics.median(r[1] for r in film_runs) / statistics.median(r[1] for r in field_runs), 4))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, '..', 'profiles', 'telecine', 'bench_telecine.json'))
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--video-frames', type=int, default=10, help='input frames of the restore_y4m arms')
    ap.add_argument('--skip-video', action='store_true', help='kernels only')
    ap.add_argument('--head', default=None, help='commit to record where the tree is not a git checkout (default: git rev-parse HEAD)')
    args = ap.parse_args()
    assert args.iters >= 20, 'the median of at least 20 calls'
    assert torch.cuda.is_available(), 'bench_telecine needs the GPU: there is no CPU path to time'
    from edvr_amd import _lib
    from edvr_amd.build import source_hash
    dev = torch.device('cuda:0')
    record = dict(bench='bench_telecine', lib=_lib.lib().edvr_version().decode(), source_hash=source_hash(),
                  git_head=args.head or git_head(os.path.join(HERE, '..')), device=torch.cuda.get_device_name(0), hbm_tbs=HBM_TBS, warmup=args.warmup,
                  iters=args.iters, kernels=kernel_rows(args, dev))
    if not args.skip_video:
        record['restore_y4m'] = video_row(args, dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
        print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
