"""Find the letterbox / pillarbox bars of a whole Y4M stream: prints `W:H:X:Y`, ffmpeg's crop order, for `restore_video.py --crop W:H:X:Y`.

    python scripts/detect_bars.py in.y4m
    ffmpeg -i dvd.vob -f yuv4mpegpipe - | python scripts/detect_bars.py - --multiple 4 --json bars.json

`restore_video.py --crop auto` decides on the first frames; this is the exact two-pass use: every frame is profiled on the device
(edvr_amd.ops.bar_profile) and the rect is that of the union of all their boxes (edvr_amd/bars.py, B2 - B6), aligned
inward to the format's chroma steps and to `--multiple` (4: what EDVR takes; 16 with --hr-in; 1 with --pad-mode).  Interlaced streams
are profiled as they are: the deinterlace and film stages keep the frame size and every row where it is.  The rect goes to stdout,
everything else to stderr; without believable bars the whole frame is printed.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def detect(args, log=log):
    import torch
    from edvr_amd import ops
    from edvr_amd.bars import BarDetector, crop_string
    from edvr_amd.y4m import ALL_FORMATS, FRAME, Y4MReader
    device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', 0)))
    torch.cuda.set_device(device)
    src = sys.stdin.buffer if args.input == '-' else open(args.input, 'rb')
    try:
        reader = Y4MReader(src, formats=ALL_FORMATS, interlaced=True)
        H, W = reader.height, reader.width
        steps = tuple(1 << s for s in reversed(reader.subsampling))
        multiple = tuple(s * args.multiple // math.gcd(s, args.multiple) for s in steps)
        det = BarDetector(H, W, reader.depth, args.limit)
        tables = []
        while True:
            host = reader.read(args.read_frames)
            if host.shape[0] == 0:
                break
            tables.append(ops.bar_profile(host.to(device, non_blocking=True)[:, len(FRAME):], H, W, reader.format))
            if len(tables) >= 64:  # bounded memory: the tables are small, the wait is rare
                det.push(torch.cat(tables).cpu())
                tables = []
        if tables:
            det.push(torch.cat(tables).cpu())
    finally:
        if src is not sys.stdin.buffer:
            src.close()
    box = det.box()
    rect = det.rect(steps, multiple, args.margin, args.min_bar)
    log(f'{args.input}: {W} x {H}, {det.frames} frames, {len(det.blank)} blank; box {box}')
    if rect is None:
        log(f'{args.input}: no believable bars: the whole frame')
    print(crop_string(rect or (0, 0, H, W)))
    if args.json:
        record = {'frames': det.frames, 'crop': crop_string(rect) if rect else None, 'rect': rect, 'box': box, 'blank': det.blank,
                  'boxes': det.boxes, 'limit': args.limit, 'margin': args.margin, 'multiple': args.multiple}
        with open(args.json, 'w') as f:
            json.dump(record, f, indent=1)
    return rect


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Find the letterbox / pillarbox bars of a whole YUV4MPEG2 stream; prints W:H:X:Y.')
    ap.add_argument('input', metavar='IN', help='Y4M file, or - for stdin')
    ap.add_argument('--limit', type=int, default=24, metavar='L', help='a row or column whose mean luma does not exceed the 8-bit level L is dark (default 24)')
    ap.add_argument('--margin', type=int, default=0, metavar='G', help='G more samples off every side that has a bar')
    ap.add_argument('--multiple', type=int, default=4, metavar='M', help="the rect's height and width are multiples of M (default 4)")
    ap.add_argument('--min-bar', type=int, default=8, metavar='N', help='an axis that would lose fewer than N samples is left alone (default 8)')
    ap.add_argument('--read-frames', type=int, default=8, help='frames per read and per copy to the device')
    ap.add_argument('--json', default=None, metavar='FILE', help="write the rect, the box and every frame's box there")
    args = ap.parse_args(argv)
    if not 0 <= args.limit <= 255:
        ap.error('--limit is an 8-bit level, 0 ... 255')
    if args.margin < 0 or args.min_bar < 0:
        ap.error('--margin and --min-bar are at least 0')
    if args.multiple < 1 or args.read_frames < 1:
        ap.error('--multiple and --read-frames are at least 1')
    return args


def main():
    detect(parse_args())


if __name__ == '__main__':
    main()
