"""Times ops.bar_profile / ops.yuv_crop (csrc/bars.hip) and the Y4M path with the crop in it.

  (a) the two kernels on 8 frames in a Y4M buffer (`buf[:, 6:]`) at 480 x 720 4:2:0, 1080 x 1920 4:2:0 and 1080 x 1920 4:2:2 10-bit, the
      crop taking the 2.35:1 picture of a 16:9 frame (3 / 4 of the rows): device events around one call after warm-up, the lower of two
      medians of --iters calls and the range of single calls, the bytes each must move (bar_profile: luma once and the table; yuv_crop:
      every output byte read and written) and the share of the 6.29 TB/s measured HBM rate they amount to; beside them
      ops.field_match (the same luma, more arithmetic) and ops.yuv_to_rgb on the same buffer;
  (b) restore_y4m on a resident letterboxed 480 x 720 stream with 360 picture rows (EDVR-L as trained, T = 5): crop='auto' against no
      crop on the SAME stream, alternated, three runs each, host clock around the call ending in a synchronise: output frames/s of both
      arms and their ratio (area alone says 480 / 360 = 1.33).

    python scripts/bench_bars.py [--out profiles/bars/bench_bars.json] [--skip-video] [--video-frames 10]
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
CASES = [  # name, frames, (H, W), format
    ('sd 8 x 480x720 420', 8, (480, 720), '420'),
    ('hd 8 x 1080x1920 420', 8, (1080, 1920), '420'),
    ('hd 8 x 1080x1920 422p10', 8, (1080, 1920), '422p10'),
]


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


def git_head(tree):
    try:
        return subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=tree, stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def kernel_rows(args, dev):
    from edvr_amd import ops
    rows = []
    for name, n, (H, W), fmt in CASES:
        fs = ops.yuv_frame_size(H, W, fmt)
        bps = 2 if ops.yuv_format(fmt)[2] > 8 else 1
        buf = torch.randint(0, 256, (n, 6 + fs), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
        if bps == 2:  # keep the words inside the depth
            buf[:, 7::2] &= (1 << (ops.yuv_format(fmt)[2] - 8)) - 1
        yuv = buf[:, 6:]
        rect = (H // 16 * 2, 0, H * 3 // 4, W)  # (an even first row: 4:2:0)
        table = torch.empty((n, H + W), dtype=torch.int64, device=dev)
        match = torch.empty((n, 7), dtype=torch.int64, device=dev)
        small = torch.empty((n, ops.yuv_frame_size(rect[2], rect[3], fmt)), dtype=torch.uint8, device=dev)
        arms = {
            'bar_profile': (lambda: ops.bar_profile(yuv, H, W, fmt, out=table), n * (H * W * bps + 8 * (H + W))),
            'yuv_crop': (lambda: ops.yuv_crop(yuv, H, W, fmt, rect=rect, out=small), 2 * small.numel()),
            'field_match': (lambda: ops.field_match(yuv, H, W, fmt, out=match), n * (H * W * bps + 8 * 7)),
            'yuv_to_rgb': (lambda: ops.yuv_to_rgb(yuv, H, W, fmt, 'bt709' if H > 576 else 'bt601'), n * (fs + 4 * 3 * H * W)),
        }
        first = {k: timed(fn, args.warmup, args.iters) for k, (fn, _) in arms.items()}
        second = {k: timed(fn, 5, args.iters) for k, (fn, _) in arms.items()}  # once more, in the same order: the lower median counts
        row = dict(case=name, frames=n, size=[H, W], format=fmt, crop_rect=list(rect))
        for k, (_, nbytes) in arms.items():
            med = min(first[k][0], second[k][0])
            row[k] = dict(us=round(med, 2), us_runs=[round(first[k][0], 2), round(second[k][0], 2)],
                          us_min_max=[round(min(first[k][1], second[k][1]), 2), round(max(first[k][2], second[k][2]), 2)], bytes=nbytes,
                          hbm_fraction=round(nbytes / (med * 1e-6) / (HBM_TBS * 1e12), 4))
        row['bar_profile_over_field_match'] = round(row['bar_profile']['us'] / row['field_match']['us'], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del buf, yuv, table, match, small
    return rows


def video_row(args, dev):
    """restore_y4m on one resident letterboxed 480 x 720 stream, 360 picture rows: EDVR-L, chunk 10, crop='auto' against no crop."""
    from edvr_amd import EDVR, ops
    from edvr_amd.y4m import restore_y4m
    H, W, n, chunk, bar = 480, 720, args.video_frames, 10, 60
    torch.manual_seed(10)
    net = EDVR(num_feat=128, num_frame=5, num_reconstruct_block=40, center_frame_idx=None).to(dev).eval()
    fs = ops.yuv420_frame_size(H, W)
    # smooth moving frames (random samples would make the network's offsets run away) between bars at limited-range black
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    frames = torch.full((n, fs), 128, dtype=torch.uint8)
    for t in range(n):
        luma = (torch.sin((xx + 5 * t) / 17.0) * torch.cos(yy / 23.0) * 80 + 128).clamp(0, 255).to(torch.uint8)
        luma[:bar] = 16
        luma[H - bar:] = 16
        frames[t, :H * W] = luma.reshape(-1)
    data = f'YUV4MPEG2 W{W} H{H} F24000:1001 Ip A32:27 C420jpeg\n'.encode() + b''.join(b'FRAME\n' + f.numpy().tobytes() for f in frames)
    arms = {'no_crop': {}, 'auto': dict(crop='auto', crop_probe=min(48, n))}

    def run(arm):
        src, dst, stats = io.BytesIO(data), io.BytesIO(), {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = restore_y4m(net, src, dst, chunk=chunk, read_frames=chunk, stats=stats, **arms[arm])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert got == n
        out = dst.getvalue()
        return got / dt, out[:out.index(b'\n')].decode(), stats.get('crop')

    with torch.no_grad():
        for arm in arms:  # warm: weights packed, the allocator filled
            run(arm)
        runs = {arm: [] for arm in arms}
        for _ in range(3):
            for arm in arms:
                runs[arm].append(run(arm))
    net.check_offsets()
    row = dict(case='EDVR-L T5 letterboxed 480 x 720 (360 picture rows)', frames=n, chunk=chunk, area_ratio=round(H / (H - 2 * bar), 4))
    for arm in arms:
        row[arm] = dict(header=runs[arm][0][1], crop=runs[arm][0][2], fps_runs=[round(r[0], 3) for r in runs[arm]],
                        fps=round(statistics.median(r[0] for r in runs[arm]), 4))
    row['auto_over_no_crop_fps'] = round(row['auto']['fps'] / row['no_crop']['fps'], 4)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, '..', 'profiles', 'bars', 'bench_bars.json'))
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--video-frames', type=int, default=10, help='input frames of the restore_y4m arms')
    ap.add_argument('--skip-video', action='store_true', help='kernels only')
    ap.add_argument('--head', default=None, help='commit to record where the tree is not a git checkout (default: git rev-parse HEAD)')
    args = ap.parse_args()
    assert args.iters >= 20, 'the median of at least 20 calls'
    assert torch.cuda.is_available(), 'bench_bars needs the GPU: there is no CPU path to time'
    from edvr_amd import _lib
    from edvr_amd.build import source_hash
    dev = torch.device('cuda:0')
    record = dict(bench='bench_bars', lib=_lib.lib().edvr_version().decode(), source_hash=source_hash(),
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
