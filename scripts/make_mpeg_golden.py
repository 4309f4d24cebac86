"""Writes tests/golden/mpeg_roundtrip.pt: what the NumPy restatement tests/mpeg_ref.py returns for a few tiny seeded clips - their bytes,
motion vectors and non-zero counts - so that the restatement of DESIGN 4.18 cannot drift (tests/test_mpeg_cpu.py) and the kernels
are pinned to the same bytes (tests/test_gpu_mpeg.py).

    python scripts/make_mpeg_golden.py

Host only.  The file holds {'cases': [{'name', 'input': uint8 (t, H, W, 3), 'qscale', 'gop', 'search', 'output': uint8 (t, H, W, 3),
'vectors': int8 (t, Hp / 16, Wp / 16, 2) of (dy, dx), zero for intra frames, 'nonzero': [int per frame]}]}: tensors, numbers and names
only.  Clips: a moving texture at 33 x 47 (odd sizes, odd chroma), one at 16 x 16 with R = 15 (every displaced read clamps), noise at
20 x 4 and 8 x 8 (the two bold rules of DESIGN 4.16), the inverted stripes (the largest residual) and the period-8 tie clip.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
OUT = os.path.join(ROOT, 'tests', 'golden', 'mpeg_roundtrip.pt')
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def cases():
    from util_mpeg import inverted_stripes_clip, moving_clip, noise_clip, tie_clip
    return [('moving_33x47', moving_clip(4, 33, 47, (1, -2), 21), 5, 3, 7),
            ('moving_16x16_r15', moving_clip(3, 16, 16, (3, 2), 22), 12, 0, 15),
            ('noise_20x4', noise_clip(1, 2, 20, 4, 23)[0], 3, 12, 7),
            ('noise_8x8', noise_clip(1, 3, 8, 8, 24)[0], 31, 2, 4),
            ('stripes_32x32', inverted_stripes_clip(3, 32, 32), 1, 0, 0),
            ('tie_48x64', tie_clip(48, 64), 1, 12, 7)]


def main():
    import mpeg_ref
    out = []
    for name, clip, qscale, gop, search in cases():
        got, stats = mpeg_ref.roundtrip_clip(clip.numpy(), qscale, gop, search, details=True)
        shape = next(v.shape for v in stats['vectors'] if v is not None)
        vectors = np.stack([np.zeros(shape, np.int8) if v is None else v.astype(np.int8) for v in stats['vectors']])
        out.append({'name': name, 'input': clip, 'qscale': qscale, 'gop': gop, 'search': search, 'output': torch.from_numpy(got),
                    'vectors': torch.from_numpy(vectors), 'nonzero': [int(v) for v in stats['nonzero']]})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save({'cases': out}, OUT)
    print(f'{OUT}: {len(out)} cases, {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    main()
