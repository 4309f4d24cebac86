"""Writes tests/golden/bd_downsample.pt: what the reference's duf_downsample (basicsr/data/data_util.py:281-331, the "BD" degradation of
the DUF code) returns for small seeded inputs - the fixture of tests/test_gpu_bd.py.

    python scripts/make_bd_golden.py --reference /path/to/EDVR

Host only (the reference runs on the CPU; it needs scipy), and only where a checkout of the reference exists: its data_util.py is loaded by
path at run time with empty stand-ins for the modules it imports and duf_downsample does not use (cv2, basicsr.data.transforms,
basicsr.utils); nothing of it is copied.  Each case holds the uint8 (2, h, w, 3) input, `scale` and the reference's float32
(2, 3, h', w') output for input / 255: tensors and numbers only.
"""
import argparse
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

CASES = [((h, w), s) for (h, w) in ((64, 96), (37, 53), (45, 63), (30, 44)) for s in (2, 3, 4)]
FRAMES = 2
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'bd_downsample.pt')


def load_reference(root):
    stubs = {'cv2': {}, 'basicsr': {}, 'basicsr.data': {}, 'basicsr.data.transforms': {'mod_crop': None},
             'basicsr.utils': {'img2tensor': None, 'scandir': None}}
    saved = {k: sys.modules.get(k) for k in stubs}
    for name, attrs in stubs.items():
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        if name in ('basicsr', 'basicsr.data'):
            mod.__path__ = []
        sys.modules[name] = mod
    try:
        spec = importlib.util.spec_from_file_location('ref_data_util', os.path.join(root, 'basicsr', 'data', 'data_util.py'))
        ref = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ref)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of a checkout of the reference (xinntao/EDVR)')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    ref = load_reference(args.reference)
    warnings.simplefilter('ignore', DeprecationWarning)  # the reference imports scipy.ndimage.filters
    cases = []
    for i, ((h, w), scale) in enumerate(CASES):
        g = torch.Generator().manual_seed(2000 + i)
        img = torch.randint(0, 256, (FRAMES, h, w, 3), generator=g, dtype=torch.uint8)
        x = torch.from_numpy(img.numpy().astype(np.float32) / np.float32(255)).permute(0, 3, 1, 2).contiguous()  # (t, c, h, w) as read_img_seq
        out = ref.duf_downsample(x, kernel_size=13, scale=scale)
        assert out.dtype == torch.float32 and torch.isfinite(out).all() and tuple(out.shape) == (FRAMES, 3, -(-h // scale), -(-w // scale))
        cases.append({'input': img, 'scale': int(scale), 'output': out.contiguous().clone()})
        print(f'{(h, w)} / {scale} -> {tuple(out.shape[2:])}')
    torch.save({'cases': cases}, args.out)
    print(f'{args.out}: {os.path.getsize(args.out)} bytes')


if __name__ == '__main__':
    main()
