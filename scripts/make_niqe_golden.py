"""Writes tests/golden/niqe.pt and copies niqe_pris_params.npz next to it: what the reference's calculate_niqe (basicsr/metrics/niqe.py)
returns for a few small seeded images - the fixture of tests/test_niqe_cpu.py and tests/test_gpu_niqe.py.

    python scripts/make_niqe_golden.py --reference /path/to/EDVR

Host only, and only where a checkout of the reference exists: its matlab_functions.py, metric_util.py and niqe.py are loaded by path at
run time under stand-in package modules (`basicsr`, `basicsr.utils`, `basicsr.metrics`); nothing of them is copied.  niqe.py needs scipy
and cv2; OpenCV is no dependency of this repository, so the stand-in `cv2` offers INTER_LINEAR and a `resize` that asserts an exact halving of even
sides and returns the 2 x 2 mean in the input's dtype.  That is a RESTATEMENT of OpenCV's INTER_LINEAR at the factor 1/2 (both source
pixels of each axis get weight 1/2 there), not OpenCV itself.  The script runs with the reference root as the working directory, because
calculate_niqe opens 'basicsr/metrics/niqe_pris_params.npz' by a relative path.

Cases (uint8 RGB bytes):
  noise    (2, 96, 192, 3)  uniform noise, two seeds, scored as one batch: the minimum of two blocks, every edge replicated
  smooth   (1, 192, 288, 3) a seeded (h/4+2) x (w/4+2) field enlarged bicubically + N(0, 0.03^2), clamped: 2 x 3 blocks
  cropped  (1, 203, 301, 3) the same kind with crop_border=4: 195 x 293 left, 192 x 288 kept at offset (4, 4), a discarded row and column
           right beside the kept edge
  grey     (1, 96, 192)     the first noise frame's red channel as one grey channel ('HW' order)
Per case: ref (calculate_niqe), ref64 (the reference's own niqe() on the same plane cast to float64) and the reference's per-block
36-feature table.  tol = 4 x max |ref - ref64| over all frames: the reference's own float32 noise - the device's float64 moments sit
between the two evaluations, and the argmin over the 0.001 grid may move one step in either.  The script asserts that no 7 x 7
neighbourhood is constant and that the smallest non-zero |z| is above 1e-7, so that no sign hangs on a float32 ulp.
"""
import argparse
import importlib.util
import os
import shutil
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, '..', 'tests', 'golden')
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(root):
    def resize(img, dsize, interpolation=None):
        h, w = img.shape
        assert interpolation == cv2.INTER_LINEAR and h % 2 == 0 and w % 2 == 0 and tuple(dsize) == (w // 2, h // 2), (img.shape, dsize)
        return ((img[0::2, 0::2] + img[0::2, 1::2]) + (img[1::2, 0::2] + img[1::2, 1::2])) * img.dtype.type(0.25)

    cv2 = types.ModuleType('cv2')
    cv2.INTER_LINEAR, cv2.resize = 1, resize
    sys.modules['cv2'] = cv2
    for pkg in ('basicsr', 'basicsr.utils', 'basicsr.metrics'):
        sys.modules[pkg] = types.ModuleType(pkg)
        sys.modules[pkg].__path__ = []
    try:
        import scipy.ndimage.filters  # noqa: F401  (a deprecated alias of scipy.ndimage that niqe.py imports)
    except ImportError:
        import scipy.ndimage
        sys.modules['scipy.ndimage.filters'] = scipy.ndimage
    base = os.path.join(root, 'basicsr')
    _load('basicsr.utils.matlab_functions', os.path.join(base, 'utils', 'matlab_functions.py'))
    _load('basicsr.metrics.metric_util', os.path.join(base, 'metrics', 'metric_util.py'))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', DeprecationWarning)
        return _load('basicsr.metrics.niqe', os.path.join(base, 'metrics', 'niqe.py'))


def to_bytes(x):
    return (x.clamp(0, 1) * 255).round().to(torch.uint8)


def noise(seed, h, w):
    return torch.randint(0, 256, (h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def smooth(seed, h, w):
    g = torch.Generator().manual_seed(seed)
    field = torch.rand(1, 3, h // 4 + 2, w // 4 + 2, generator=g)
    big = torch.nn.functional.interpolate(field, scale_factor=4, mode='bicubic', align_corners=False)[0, :, 4:4 + h, 4:4 + w]
    assert big.shape == (3, h, w)
    return to_bytes(big + 0.03 * torch.randn(3, h, w, generator=g)).permute(1, 2, 0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of a checkout of the reference (xinntao/EDVR)')
    ap.add_argument('--out', default=os.path.join(GOLDEN, 'niqe.pt'))
    args = ap.parse_args()
    root, out = os.path.abspath(args.reference), os.path.abspath(args.out)
    ref = load_reference(root)
    import util_niqe

    frames = [noise(9601, 96, 192), noise(9602, 96, 192)]
    cases = [dict(name='noise', img=torch.stack(frames), crop_border=0),
             dict(name='smooth', img=smooth(9603, 192, 288)[None], crop_border=0),
             dict(name='cropped', img=smooth(9604, 203, 301)[None], crop_border=4),
             dict(name='grey', img=frames[0][None, :, :, 0].contiguous(), crop_border=0)]

    table = []
    compute_feature = ref.compute_feature

    def recording(block):
        table.append(compute_feature(block))
        return table[-1]

    ref.compute_feature = recording
    os.chdir(root)
    par = np.load('basicsr/metrics/niqe_pris_params.npz')
    worst = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for case in cases:
            case['ref'], case['ref64'], feats = [], [], []
            for img in case['img'].numpy():
                crop, grey = case['crop_border'], img.ndim == 2
                del table[:]
                r = float(ref.calculate_niqe(img if grey else img[..., ::-1], crop, input_order='HW' if grey else 'HWC', convert_to='y'))
                k = len(table) // 2
                feats.append(np.concatenate([np.array(table[:k]), np.array(table[k:])], 1))
                # the plane calculate_niqe hands to niqe(), once more in float64
                plane = img.astype(np.float32) if grey else np.squeeze(ref.to_y_channel(img[..., ::-1].astype(np.float32)))
                if crop:
                    plane = plane[crop:-crop, crop:-crop]
                assert plane.dtype == np.float32
                r64 = float(ref.niqe(plane.astype(np.float64), par['mu_pris_param'], par['cov_pris_param'], par['gaussian_window']))
                case['ref'].append(r)
                case['ref64'].append(r64)
                worst = max(worst, abs(r - r64))
                # no sign may hang on a float32 ulp, no neighbourhood may be constant
                x, _, _ = util_niqe.kept(plane, 0)
                assert np.array_equal(x, util_niqe.kept(util_niqe.y_plane(img), crop)[0]), 'the restated Y plane is not the reference one'
                for scale in (1, 2):
                    xp = np.pad(x, 3, mode='edge')
                    win = np.lib.stride_tricks.sliding_window_view(xp, (7, 7))
                    assert (win.max((2, 3)) > win.min((2, 3))).all(), f'{case["name"]}: a constant 7x7 neighbourhood at scale {scale}'
                    z = np.abs(util_niqe.mscn(x))
                    assert z[z > 0].min() > 1e-7, f'{case["name"]}: |z| = {z[z > 0].min()} at scale {scale}'
                    x = util_niqe.half(x)
                print(f'{case["name"]}: ref {r:.9f}  ref64 {r64:.9f}  |d| {abs(r - r64):.2e}')
            case['feat'] = torch.from_numpy(np.stack(feats))
    tol = 4.0 * worst
    torch.save({'tol': tol, 'cases': cases}, out)
    shutil.copyfile('basicsr/metrics/niqe_pris_params.npz', os.path.join(os.path.dirname(out), 'niqe_pris_params.npz'))
    print(f'{out}: {os.path.getsize(out)} bytes, tol = 4 x {worst:.3e} = {tol:.3e}')


if __name__ == '__main__':
    main()
