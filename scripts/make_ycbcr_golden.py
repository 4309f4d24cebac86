"""Writes tests/golden/ycbcr.pt: what the reference's rgb2ycbcr / ycbcr2rgb (basicsr/utils/matlab_functions.py:173-270, MATLAB's BT.601
limited-range conversion) return for a small seeded input - the fixture of tests/test_yuv_cpu.py and tests/test_gpu_yuv.py.

    python scripts/make_ycbcr_golden.py --reference /path/to/EDVR

Host only, and only where a checkout of the reference exists: its matlab_functions.py (numpy and torch, nothing else) is loaded by path at
run time; nothing of it is copied.  The file holds tensors only:
  rgb    uint8 (2, 48, 64, 3): seeded (2, 24, 32, 3) bytes enlarged x2 by replication, so that every 2 x 2 block is constant - 4:2:0
         subsampling then loses nothing and the 4:4:4 reference can be compared plane by plane
  ycbcr  uint8 (2, 48, 64, 3): the reference's rgb2ycbcr(rgb)
  back   uint8 (2, 48, 64, 3): the reference's ycbcr2rgb(ycbcr)
  mask   bool  (2, 48, 64): pixels where the reference's inverse BEFORE rounding lies in [0, 255] in all three channels - outside, the
         reference's uint8 cast wraps around where this package clamps (read off the function's own post-processing step, called with it)
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'ycbcr.pt')
SEED, SMALL = 4110, (2, 24, 32, 3)


def load_reference(root):
    spec = importlib.util.spec_from_file_location('ref_matlab_functions', os.path.join(root, 'basicsr', 'utils', 'matlab_functions.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of a checkout of the reference (xinntao/EDVR)')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    ref = load_reference(args.reference)
    g = torch.Generator().manual_seed(SEED)
    small = torch.randint(0, 256, SMALL, generator=g, dtype=torch.uint8)
    rgb = small.repeat_interleave(2, 1).repeat_interleave(2, 2).contiguous()
    unrounded = []
    post = ref._convert_output_type_range

    def recording(img, dst_type):
        unrounded.append(np.array(img, dtype=np.float64))
        return post(img, dst_type)

    ycbcr = np.stack([ref.rgb2ycbcr(f) for f in rgb.numpy()])
    ref._convert_output_type_range = recording
    try:
        back = np.stack([ref.ycbcr2rgb(f) for f in ycbcr])
    finally:
        ref._convert_output_type_range = post
    raw = np.stack(unrounded)
    mask = ((raw >= 0.0) & (raw <= 255.0)).all(-1)
    assert ycbcr.dtype == np.uint8 and back.dtype == np.uint8 and ycbcr.shape == back.shape == tuple(rgb.shape) and mask.shape == tuple(rgb.shape[:3])
    torch.save({'rgb': rgb, 'ycbcr': torch.from_numpy(ycbcr), 'back': torch.from_numpy(back), 'mask': torch.from_numpy(mask)}, args.out)
    print(f'{args.out}: {os.path.getsize(args.out)} bytes, {mask.mean() * 100:.2f} % of pixels in gamut, '
          f'max |back - rgb| on them {np.abs(back.astype(int) - rgb.numpy().astype(int))[mask].max()}')


if __name__ == '__main__':
    main()
