"""Writes tests/golden/imresize.pt: what the reference's imresize (basicsr/utils/matlab_functions.py:88-170, the Python statement of
MATLAB's antialiased bicubic imresize) returns for small seeded inputs - the fixture of tests/test_gpu_imresize.py.

    python scripts/make_imresize_golden.py --reference /path/to/EDVR

Host only (the reference runs on the CPU), and only where a checkout of the reference exists: its matlab_functions.py is loaded by path at
run time, nothing of it is copied.  Each case holds the uint8 (h, w, 3) input, `scale`, `antialiasing` and the reference's float32
(3, h', w') output for input / 255.  Shapes the reference cannot run (a mirrored tail of length 0: `img[:, -0:]` selects the whole
image) are left out; the GPU test checks those against the formula.
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

CASES = [  # (h, w), scale - all with antialiasing
    ((64, 96), 1 / 4), ((37, 53), 1 / 4), ((48, 60), 1 / 2), ((45, 63), 1 / 3), ((50, 70), 0.3), ((30, 44), 2), ((30, 44), 4),
]
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'imresize.pt')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of a checkout of the reference (xinntao/EDVR)')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location('ref_matlab_functions', os.path.join(args.reference, 'basicsr', 'utils', 'matlab_functions.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    cases = []
    for i, ((h, w), scale) in enumerate(CASES):
        g = torch.Generator().manual_seed(1000 + i)
        img = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
        x = torch.from_numpy(img.numpy().astype(np.float32) / np.float32(255)).permute(2, 0, 1).contiguous()  # imfrombytes(float32=True) + img2tensor
        out = ref.imresize(x, scale, antialiasing=True)
        assert out.dtype == torch.float32 and torch.isfinite(out).all()
        cases.append({'input': img, 'scale': float(scale), 'antialiasing': True, 'output': out.contiguous()})
        print(f'{(h, w)} x {scale:.4g} -> {tuple(out.shape[1:])}')
    torch.save({'cases': cases}, args.out)
    print(f'{args.out}: {os.path.getsize(args.out)} bytes')


if __name__ == '__main__':
    main()
