"""Writes tests/golden/jpeg_roundtrip.pt: what PIL's libjpeg returns for small seeded frames written as baseline JPEG and read back - the
fixture of tests/test_jpeg_cpu.py and tests/test_gpu_jpeg.py, the third-party codec that pins ops.jpeg_roundtrip.

    python scripts/make_jpeg_golden.py

Host only; needs PIL (Image.save(format='JPEG', quality=q, subsampling=2 | 0), Image.open(...).convert('RGB')).  The file holds
{'pil': PIL's version, 'cases': [{'name', 'input': uint8 (H, W, 3), 'outputs': [(quality, subsampling, uint8 (H, W, 3))]}]}: tensors,
numbers and names only.  Frames: seeded noise over a sinusoid and a hard-edged checker (coefficients near rounding boundaries, the sample
clamps fire) at 1 x 1, 7 x 9 (less than a block), 8 x 8 (an even height short of an MCU: the encoder's chroma row padding), 16 x 16,
17 x 33 (one past an MCU, odd chroma), 37 x 53, 64 x 64 (the training crop) and 130 x 131 (more than two of the kernel's 64 x 64 tiles on
both axes: a chroma ring crosses a tile seam each way); flat grey, all 0, all 255 and a pure magenta / green checker (the out-of-gamut
clamps of the colour conversion back) at 17 x 33; 20 x 4 (a chroma plane 2 samples wide, which the decoder replicates instead of
filtering).
"""
import argparse
import io
import os

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'jpeg_roundtrip.pt')
QUALITIES = (1, 10, 50, 75, 95, 100)
BOTH = ('420', '444')
ALL = [(q, s) for q in QUALITIES for s in BOTH]


def noise_frame(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    base = 128 + 70 * np.sin(xx / 3.0 + yy / 5.0) + 60 * ((((xx // 5) + (yy // 3)) & 1) * 2 - 1)
    return np.clip(base[..., None] + rng.normal(0, 30, (h, w, 3)), 0, 255).astype(np.uint8)


def checker(h, w, a, b):
    yy, xx = np.mgrid[:h, :w]
    return np.where((((xx // 3) + (yy // 2)) & 1)[..., None] == 0, np.uint8(a), np.uint8(b)).astype(np.uint8)


def cases():
    out = [(f'noise_{h}x{w}', noise_frame(h, w, 100 + i), ALL) for i, (h, w) in enumerate(((1, 1), (7, 9), (8, 8), (16, 16), (17, 33)))]
    out.append(('noise_37x53', noise_frame(37, 53, 200), [(1, '420'), (50, '420'), (95, '420'), (50, '444')]))
    out.append(('noise_64x64', noise_frame(64, 64, 201), [(10, '420'), (75, '420'), (100, '444')]))
    out.append(('noise_130x131', noise_frame(130, 131, 202), [(50, '420')]))
    out.append(('noise_20x4', noise_frame(20, 4, 203), [(10, '420'), (75, '420'), (75, '444')]))
    some = [(10, '420'), (95, '420'), (10, '444'), (95, '444')]
    out.append(('grey_17x33', np.full((17, 33, 3), 117, np.uint8), some))
    out.append(('zeros_17x33', np.zeros((17, 33, 3), np.uint8), some))
    out.append(('ones_17x33', np.full((17, 33, 3), 255, np.uint8), some))
    out.append(('magenta_green_17x33', checker(17, 33, (255, 0, 255), (0, 255, 0)), some))
    return out


def pil_roundtrip(img, quality, subsampling):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format='JPEG', quality=quality, subsampling={'444': 0, '420': 2}[subsampling])
    buf.seek(0)
    return np.asarray(Image.open(buf).convert('RGB'))


def main():
    import PIL
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    rec = []
    for name, img, combos in cases():
        outs = [(int(q), s, torch.from_numpy(pil_roundtrip(img, q, s).copy())) for q, s in combos]
        assert all(o.shape == img.shape and o.dtype == torch.uint8 for _, _, o in outs)
        rec.append({'name': name, 'input': torch.from_numpy(img.copy()), 'outputs': outs})
        print(f'{name}: {len(outs)} round trip(s)')
    torch.save({'pil': PIL.__version__, 'cases': rec}, args.out)
    print(f'{args.out}: {os.path.getsize(args.out)} bytes')


if __name__ == '__main__':
    main()
