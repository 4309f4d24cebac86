"""Input pipeline of the EDVR hot path, MI355X-first.

Reference: REDSDataset (basicsr/data/reds_dataset.py:12-237) decodes PNGs to float32 HWC in DataLoader worker processes, crops
and flips float arrays per image (transforms.py:25-151), converts to CHW tensors (img_util.py:9-33), the default collate copies
them again and CUDAPrefetcher moves 4 bytes per sample over PCIe (prefetch_dataloader.py:84-126).

Here the host does only what must be on the host - frame selection (the reference's random draws, in its order), PNG decode and
a byte crop straight into pinned staging - in threads of ONE process per GPU (PIL's decoder releases the GIL), uint8 patches
cross PCIe on a side stream (1 byte per sample), and one HIP launch per tensor (`edvr_frames_u8_to_f32`, csrc/data.hip) does
flip / transpose / HWC->CHW / division by 255 for the whole batch.  `REDSDeviceLoader.next()` hands out device tensors like
CUDAPrefetcher.next() does, already waited for on the current stream.

The storage formats are the reference's: PNG folders `<root>/<clip>/<frame:08d>.png` (disk backend) and its LMDB layout (keys
`<clip>/<frame:08d>`, PNG-encoded values; file_client.py:76-144) when the `lmdb` module is importable.
"""
import contextlib
import io
import math
import os
import queue
import random
import threading
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

AUG_HFLIP, AUG_VFLIP, AUG_ROT90 = 1, 2, 4


# ------------------------------------------------------------------------------------------------ storage + decode (host)
class DiskClient:
    """Disk backend (file_client.py:60-74): `<root>/<clip>/<frame>.png`."""

    def __init__(self, roots):
        self.roots = {k: Path(v) for k, v in roots.items()}

    def path(self, kind, clip, frame):
        return self.roots[kind] / clip / f'{frame}.png'

    def get(self, kind, clip, frame):
        with open(self.path(kind, clip, frame), 'rb') as f:
            return f.read()

    def size(self, kind, clip, frame):
        from PIL import Image
        with Image.open(self.path(kind, clip, frame)) as im:  # reads the header only
            return im.size[1], im.size[0]


class LmdbClient:
    """LMDB backend (file_client.py:76-144): one environment per kind, key `<clip>/<frame>`, value = PNG bytes."""

    def __init__(self, roots):
        try:
            import lmdb
        except ImportError:
            raise ImportError('Please install lmdb to enable the lmdb io_backend.')
        self.envs = {k: lmdb.open(str(v), readonly=True, lock=False, readahead=False) for k, v in roots.items()}

    def get(self, kind, clip, frame):
        with self.envs[kind].begin(write=False) as txn:
            return bytes(txn.get(f'{clip}/{frame}'.encode('ascii')))

    def size(self, kind, clip, frame):
        return image_size(self.get(kind, clip, frame))


def decode_image(content):
    """PNG/JPEG bytes -> uint8 (h, w, 3) RGB.  Lossless formats decode to the bytes cv2.imdecode gives (imfrombytes,
    img_util.py:101-123), in RGB order instead of BGR - which is where img2tensor's bgr2rgb ends up anyway."""
    from PIL import Image
    with Image.open(io.BytesIO(content)) as im:
        return np.asarray(im.convert('RGB'))


def image_size(content):
    """(h, w) from the header only."""
    from PIL import Image
    with Image.open(io.BytesIO(content)) as im:
        return im.size[1], im.size[0]


# ------------------------------------------------------------------------------------------------ sample planning (host)
def reds_keys(meta_info_file, val_partition):
    """Keys `clip/frame` of the training split (reds_dataset.py:62-81)."""
    keys = []
    with open(meta_info_file, 'r') as fin:
        for line in fin:
            folder, frame_num, _ = line.split(' ')
            keys.extend(f'{folder}/{i:08d}' for i in range(int(frame_num)))
    if val_partition == 'REDS4':
        val = {'000', '011', '015', '020'}
    elif val_partition == 'official':
        val = {f'{v:03d}' for v in range(240, 270)}
    else:
        raise ValueError(f'Wrong validation partition {val_partition}.Supported ones are [\'official\', \'REDS4\'].')
    return [k for k in keys if k.split('/')[0] not in val]


class ClipPlan:
    """Every random decision of one training sample: which frames, where to crop, how to augment."""
    __slots__ = ('key', 'clip', 'center', 'frames', 'top', 'left', 'flags', 'jpeg_quality', 'degrade', 'mpeg_qscale')

    def __init__(self, key, clip, center, frames, top, left, flags, jpeg_quality=0, degrade=None, mpeg_qscale=0):
        self.key, self.clip, self.center, self.frames, self.top, self.left, self.flags = key, clip, center, frames, top, left, flags
        self.jpeg_quality = jpeg_quality  # of the LQ crops' JPEG round trip (lq_jpeg), all frames of the clip alike; 0 = none
        self.degrade = degrade  # blur and noise of the LQ crops (lq_degrade; _draw_degrade), all frames of the clip alike; None = none
        self.mpeg_qscale = mpeg_qscale  # of the LQ crop clip's MPEG-style round trip (lq_mpeg); 0 = none

    def __repr__(self):
        jpeg = f', jpeg {self.jpeg_quality}' if self.jpeg_quality else ''
        degrade = f", blur {self.degrade['blur']}, noise {self.degrade['noise']}" if self.degrade else ''
        mpeg = f', mpeg {self.mpeg_qscale}' if self.mpeg_qscale else ''
        return f'ClipPlan({self.key}: frames {self.frames} of {self.clip}, crop ({self.top}, {self.left}), aug {self.flags}{jpeg}{degrade}{mpeg})'


def _make_client(opt, client, with_lq):
    """The storage of a training option block: `client` if given (any object with get(kind, clip, frame) -> bytes and
    size(kind, clip, frame) -> (h, w)), else the backend opt['io_backend'] names over the GT root and - with an LQ tree - the LQ root."""
    if client is not None:
        return client
    roots = {'gt': opt['dataroot_gt']}
    if with_lq:
        roots['lq'] = opt['dataroot_lq']
    backend = dict(opt['io_backend'])['type']
    if backend == 'lmdb':
        return LmdbClient(roots)
    if backend == 'disk':
        return DiskClient(roots)
    raise ValueError(f'io_backend {backend} is not supported (disk, lmdb)')


def training_lq_jpeg(opt):
    """The `lq_jpeg` key of a TRAINING option block: None without it, else (lo, hi, subsampling, prob) of
    {'quality': q | [lo, hi], 'subsampling': '420' | '444', 'prob': 0 .. 1}: the LQ crops of a clip go through ops.jpeg_roundtrip at a
    quality drawn from lo .. hi with probability prob.  ValueError for a quality outside 1 .. 100, lo > hi, an unknown
    subsampling or key and a prob outside [0, 1]."""
    from .ops import JPEG_SUBSAMPLINGS, jpeg_quality
    if opt.get('lq_jpeg') is None:
        return None
    spec = dict(opt['lq_jpeg'])
    unknown = set(spec) - {'quality', 'subsampling', 'prob'}
    if unknown or 'quality' not in spec:
        raise ValueError(f"lq_jpeg takes 'quality' and optionally 'subsampling' and 'prob', got {sorted(spec)}")
    quality = spec['quality']
    if isinstance(quality, (list, tuple)):
        if len(quality) != 2:
            raise ValueError(f'lq_jpeg: quality is an int or [lo, hi], got {quality!r}')
        lo, hi = (jpeg_quality(q, 'lq_jpeg: quality') for q in quality)
    else:
        lo = hi = jpeg_quality(quality, 'lq_jpeg: quality')
    if lo > hi:
        raise ValueError(f'lq_jpeg: quality range [{lo}, {hi}] is empty')
    subsampling = spec.get('subsampling', '420')
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError(f'lq_jpeg: subsampling must be one of {JPEG_SUBSAMPLINGS}, got {subsampling!r}')
    prob = spec.get('prob', 1.0)
    if isinstance(prob, bool) or not isinstance(prob, (int, float)) or not 0 <= prob <= 1:
        raise ValueError(f'lq_jpeg: prob must be a number in [0, 1], got {prob!r}')
    return lo, hi, subsampling, float(prob)


def _draw_jpeg_quality(lq_jpeg, rng):
    """The planners' last draws, made only where the option block has `lq_jpeg`: [r.random() < prob where prob < 1], then
    r.randint(lo, hi) - on a stream r forked from the state `rng` is in after the reference's draws.  `rng` itself is not advanced, so
    every other decision of the epoch - this plan's and all later ones' - is what it is without the key, and a loader with the key
    yields the batches of the loader without it, compressed."""
    if lq_jpeg is None:
        return 0
    lo, hi, _, prob = lq_jpeg
    r = random.Random(repr(rng.getstate()))
    if prob < 1 and not r.random() < prob:
        return 0
    return r.randint(lo, hi)


def training_lq_mpeg(opt):
    """The `lq_mpeg` key of a TRAINING option block: None without it, else (lo, hi, search, prob) of
    {'qscale': q | [lo, hi], 'search': 0 .. 15, 'prob': 0 .. 1}: the LQ crops of a clip go through ops.mpeg_roundtrip as one clip, its
    first frame the only intra frame, at a quantiser scale drawn from lo .. hi with probability prob.  ValueError for a
    qscale outside 1 .. 31, lo > hi, a search outside 0 .. 15, an unknown key and a prob outside [0, 1]."""
    from .ops import mpeg_qscale, mpeg_search
    if opt.get('lq_mpeg') is None:
        return None
    spec = dict(opt['lq_mpeg'])
    unknown = set(spec) - {'qscale', 'search', 'prob'}
    if unknown or 'qscale' not in spec:
        raise ValueError(f"lq_mpeg takes 'qscale' and optionally 'search' and 'prob', got {sorted(spec)}")
    qscale = spec['qscale']
    if isinstance(qscale, (list, tuple)):
        if len(qscale) != 2:
            raise ValueError(f'lq_mpeg: qscale is an int or [lo, hi], got {qscale!r}')
        lo, hi = (mpeg_qscale(q, 'lq_mpeg: qscale') for q in qscale)
    else:
        lo = hi = mpeg_qscale(qscale, 'lq_mpeg: qscale')
    if lo > hi:
        raise ValueError(f'lq_mpeg: qscale range [{lo}, {hi}] is empty')
    search = mpeg_search(spec.get('search', 7), 'lq_mpeg: search')
    prob = spec.get('prob', 1.0)
    if isinstance(prob, bool) or not isinstance(prob, (int, float)) or not 0 <= prob <= 1:
        raise ValueError(f'lq_mpeg: prob must be a number in [0, 1], got {prob!r}')
    return lo, hi, search, float(prob)


def _draw_mpeg_qscale(lq_mpeg, rng):
    """The clip's quantiser scale, drawn only where the option block has `lq_mpeg`: [r.random() < prob where prob < 1], then
    r.randint(lo, hi), on a stream r = random.Random('lq_mpeg' + repr(rng.getstate())) forked from the state _draw_jpeg_quality and
    _draw_degrade fork from, so that `rng` and every other decision of the epoch - JPEG quality, blur and noise included - are what
    they are without the key."""
    if lq_mpeg is None:
        return 0
    lo, hi, _, prob = lq_mpeg
    r = random.Random('lq_mpeg' + repr(rng.getstate()))
    if prob < 1 and not r.random() < prob:
        return 0
    return r.randint(lo, hi)


LQ_DEGRADE_DEFAULTS = {'blur': {'ksize': [7, 21], 'sigma': [0.2, 3.0], 'iso_prob': 0.7, 'prob': 1.0},
                       'noise': {'sigma': [1, 30], 'shot': [0.0025, 9.0], 'shot_prob': 0.5, 'gray_prob': 0.4, 'prob': 1.0}}


def training_lq_degrade(opt):
    """The `lq_degrade` key of a TRAINING option block: None without it, else {'blur': None | {...}, 'noise': None | {...}} with every
    value of LQ_DEGRADE_DEFAULTS filled in and checked - the first-order ranges of Real-ESRGAN (its Poisson scale p is shot ~ p^2).  Either
    key is optional.  blur: 'ksize' k | [lo, hi] (the odd sizes in it, 3 .. 21), 'sigma' s | [lo, hi] > 0, 'iso_prob', 'prob'; noise:
    'sigma' (read noise, levels) s | [lo, hi] >= 0, 'shot' (variance per level) a | [lo, hi] > 0, 'shot_prob', 'gray_prob', 'prob'
    (DESIGN 4.17).  ValueError for unknown keys, empty ranges and probabilities outside [0, 1]."""
    from .ops import DEGRADE_MAX_KSIZE
    if opt.get('lq_degrade') is None:
        return None
    spec = dict(opt['lq_degrade'])
    if not spec or set(spec) - set(LQ_DEGRADE_DEFAULTS):
        raise ValueError(f"lq_degrade takes 'blur' and / or 'noise', got {sorted(spec)}")

    def number(v, what):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f'lq_degrade: {what} must be a finite number, got {v!r}')
        return v

    def span(v, what, lo_ok):
        v = list(v) if isinstance(v, (list, tuple)) else [v, v]
        if len(v) != 2:
            raise ValueError(f'lq_degrade: {what} is a number or [lo, hi], got {v!r}')
        lo, hi = (number(x, what) for x in v)
        if lo > hi or not lo_ok(lo):
            raise ValueError(f'lq_degrade: {what} range [{lo}, {hi}] is empty or out of range')
        return lo, hi

    out = {'blur': None, 'noise': None}
    for part, defaults in LQ_DEGRADE_DEFAULTS.items():
        if spec.get(part) is None:
            continue
        given = dict(spec[part])
        if set(given) - set(defaults):
            raise ValueError(f'lq_degrade: {part} takes {sorted(defaults)}, got {sorted(given)}')
        full = dict(defaults, **given)
        for k in full:
            if k.endswith('prob'):
                if not 0 <= number(full[k], f'{part}.{k}') <= 1:
                    raise ValueError(f'lq_degrade: {part}.{k} must lie in [0, 1], got {full[k]!r}')
                full[k] = float(full[k])
        if part == 'blur':
            lo, hi = span(full['ksize'], 'blur.ksize', lambda v: True)
            if lo != int(lo) or hi != int(hi):
                raise ValueError(f"lq_degrade: blur.ksize takes ints, got {full['ksize']!r}")
            full['ksize'] = [k for k in range(max(int(lo), 3) | 1, min(int(hi), DEGRADE_MAX_KSIZE) + 1, 2)]
            if not full['ksize']:
                raise ValueError(f'lq_degrade: blur.ksize range [{lo}, {hi}] holds no odd size in 3 .. {DEGRADE_MAX_KSIZE}')
            full['sigma'] = tuple(float(v) for v in span(full['sigma'], 'blur.sigma', lambda v: v > 0))
        else:
            full['sigma'] = tuple(float(v) for v in span(full['sigma'], 'noise.sigma', lambda v: v >= 0))
            full['shot'] = tuple(float(v) for v in span(full['shot'], 'noise.shot', lambda v: v > 0))
        out[part] = full
    return out


def _draw_degrade(lq_degrade, rng):
    """The blur and noise of one clip, made only where the option block has `lq_degrade`: None, or {'blur': None | (ksize, sigma_x,
    sigma_y, theta), 'kernel': None | gaussian_blur_kernel of it, 'noise': None | (read_sigma, shot, gray), 'key': 64 bits} - what
    ops.degrade takes as blur=, noise= and seed=, with frame_index = the frame's place in the clip.  The draws, on a stream
    r = random.Random('lq_degrade' + repr(rng.getstate())) forked from the state _draw_jpeg_quality forks from, so that `rng` and every
    other decision of the epoch stay what they are without the key: blur - [r.random() < prob where prob < 1], r.choice(odd sizes),
    sigma_x = r.uniform(lo, hi), r.random() < iso_prob, else sigma_y = r.uniform(lo, hi) and theta = r.uniform(-pi, pi); noise -
    [r.random() < prob where prob < 1], r.random() < shot_prob, then the read sigma r.uniform(lo, hi) or the shot exp(r.uniform(ln lo,
    ln hi)), gray = r.random() < gray_prob; last key = r.getrandbits(64)."""
    if lq_degrade is None:
        return None
    r = random.Random('lq_degrade' + repr(rng.getstate()))
    blur = noise = kernel = None
    b, n = lq_degrade['blur'], lq_degrade['noise']
    if b is not None and (b['prob'] >= 1 or r.random() < b['prob']):
        ksize = r.choice(b['ksize'])
        sx = sy = r.uniform(*b['sigma'])
        theta = 0.0
        if not r.random() < b['iso_prob']:
            sy = r.uniform(*b['sigma'])
            theta = r.uniform(-math.pi, math.pi)
        blur = (ksize, sx, sy, theta)
        kernel = gaussian_blur_kernel(*blur)
    if n is not None and (n['prob'] >= 1 or r.random() < n['prob']):
        if r.random() < n['shot_prob']:
            sigma, shot = 0.0, math.exp(r.uniform(math.log(n['shot'][0]), math.log(n['shot'][1])))
        else:
            sigma, shot = r.uniform(*n['sigma']), 0.0
        noise = (sigma, shot, r.random() < n['gray_prob'])
    if blur is None and noise is None:
        return None
    return {'blur': blur, 'kernel': kernel, 'noise': noise, 'key': r.getrandbits(64)}


class REDSClipPlanner:
    """The decisions of REDSDataset.__getitem__ (reds_dataset.py:106-234), separated from the pixels.  `opt` has the reference's
    keys (dataroot_gt, dataroot_lq, meta_info_file, val_partition, io_backend, num_frame, gt_size, interval_list, random_reverse,
    use_flip, use_rot, scale).  plan(index, rng) draws from `rng` (a random.Random or the `random` module) exactly the values the
    reference draws, in its order: interval, [new centre frames while the window leaves 0..99], [reverse], crop top, crop left,
    [hflip], [vflip], [rot90] - and after them, with an `lq_jpeg` key only (training_lq_jpeg), the clip's JPEG quality, from a fork of
    the stream (_draw_jpeg_quality) that leaves `rng` where the reference's draws left it; with an `lq_degrade` key only
    (training_lq_degrade) the clip's blur and noise, from another fork of the same state (_draw_degrade)."""

    def __init__(self, opt, client=None):
        if opt.get('dataroot_flow') is not None:
            raise NotImplementedError('optical-flow inputs (dataroot_flow) are not on the EDVR path')
        assert opt['num_frame'] % 2 == 1, f'num_frame should be odd number, but got {opt["num_frame"]}'
        self.opt = opt
        self.num_frame, self.half = opt['num_frame'], opt['num_frame'] // 2
        self.scale, self.gt_size = opt['scale'], opt['gt_size']
        self.lq_size = self.gt_size // self.scale
        self.keys = reds_keys(opt['meta_info_file'], opt['val_partition'])
        self.interval_list, self.random_reverse = opt['interval_list'], opt['random_reverse']
        self.lq_from_gt = training_lq_from_gt(opt)  # None: an LQ tree
        self.lq_jpeg = training_lq_jpeg(opt)  # None: no JPEG round trip of the LQ crops
        self.lq_degrade = training_lq_degrade(opt)  # None: no blur or noise on the LQ crops
        self.lq_mpeg = training_lq_mpeg(opt)  # None: no MPEG-style round trip of the LQ crop clips
        self.client = _make_client(opt, client, self.lq_from_gt is None)
        self._shape = {}  # clip -> ((h_lq, w_lq), (h_gt, w_gt)): all frames of a REDS clip have one size
        # the one place the two sources of LQ part: where the sizes come from and what load() stages
        if self.lq_from_gt is None:
            self.windows = None
            self._sizes = lambda clip, frame: (self.client.size('lq', clip, frame), self.client.size('gt', clip, frame))
            self.load = self._load_lq_tree
        else:
            self.windows = _WindowsFromGT(self.client, self.lq_size, self.gt_size, *self.lq_from_gt)
            self._sizes = self.windows.sizes
            self.load = self._load_gt_windows

    def __len__(self):
        return len(self.keys)

    def clip_shapes(self, clip, frame):
        if clip not in self._shape:
            self._shape[clip] = self._sizes(clip, frame)
        return self._shape[clip]

    def plan(self, index, rng=random):
        key = self.keys[index]
        clip, frame_name = key.split('/')
        center = int(frame_name)
        interval = rng.choice(self.interval_list)
        while center - self.half * interval < 0 or center + self.half * interval > 99:  # each clip has frames 0..99
            center = rng.randint(0, 99)
        frames = list(range(center - self.half * interval, center + self.half * interval + 1, interval))
        if self.random_reverse and rng.random() < 0.5:
            frames.reverse()
        assert len(frames) == self.num_frame, f'Wrong length of neighbor list: {len(frames)}'
        (h_lq, w_lq), (h_gt, w_gt) = self.clip_shapes(clip, f'{center:08d}')
        if h_gt != h_lq * self.scale or w_gt != w_lq * self.scale:
            raise ValueError(f'Scale mismatches. GT ({h_gt}, {w_gt}) is not {self.scale}x multiplication of LQ ({h_lq}, {w_lq}).')
        if h_lq < self.lq_size or w_lq < self.lq_size:
            raise ValueError(f'LQ ({h_lq}, {w_lq}) is smaller than patch size ({self.lq_size}, {self.lq_size}). '
                             f'Please remove {clip}/{center:08d}.')
        top = rng.randint(0, h_lq - self.lq_size)
        left = rng.randint(0, w_lq - self.lq_size)
        flags = 0
        if self.opt['use_flip'] and rng.random() < 0.5:
            flags |= AUG_HFLIP
        if self.opt['use_rot'] and rng.random() < 0.5:
            flags |= AUG_VFLIP
        if self.opt['use_rot'] and rng.random() < 0.5:
            flags |= AUG_ROT90
        return ClipPlan(key, clip, center, frames, top, left, flags, _draw_jpeg_quality(self.lq_jpeg, rng), _draw_degrade(self.lq_degrade, rng),
                        _draw_mpeg_qscale(self.lq_mpeg, rng))

    def _load_gt_windows(self, plan, lq_out=None, gt_out=None):
        """load() without an LQ tree: lq is the pair (windows (t, e, pitch) uint8, table (t, 8) int32) of the decoded GT frames for
        ops.lq_crops_from_windows (e = lq_window_extent, pitch = lq_window_pitch(e)), gt as below."""
        return self.windows.load(plan, [f'{f:08d}' for f in plan.frames], f'{plan.center:08d}', lq_out, gt_out)

    def _load_lq_tree(self, plan, lq_out=None, gt_out=None):
        """load(): decode the frames of `plan` and crop bytes: lq (t, p, p, 3), gt (P, P, 3) uint8 RGB, written into lq_out / gt_out
        (views of pinned staging) when given."""
        p, P, s = self.lq_size, self.gt_size, self.scale
        if lq_out is None:
            lq_out = np.empty((self.num_frame, p, p, 3), np.uint8)
        if gt_out is None:
            gt_out = np.empty((P, P, 3), np.uint8)
        for i, f in enumerate(plan.frames):
            lq_out[i] = decode_image(self.client.get('lq', plan.clip, f'{f:08d}'))[plan.top:plan.top + p, plan.left:plan.left + p]
        gt_out[...] = decode_image(self.client.get('gt', plan.clip, f'{plan.center:08d}'))[plan.top * s:plan.top * s + P,
                                                                                          plan.left * s:plan.left * s + P]
        return lq_out, gt_out


class Vimeo90KClipPlanner:
    """The decisions of Vimeo90KDataset.__getitem__ (the TRAINING set, basicsr/data/vimeo90k_dataset.py:10-134) for the same loader:
    7-frame sequences `<root>/<clip>/<seq>/im1.png .. im7.png`, keys from the meta file (`00001/0001 7 (256,448,3)`), GT = im4,
    the centred window of `num_frame` frames, and the reference's draws in its order: [reverse], crop top, crop left, [hflip],
    [vflip], [rot90].  The reference reverses its neighbour list IN PLACE (:82-83), so the orientation persists from one sample to
    the next: plan() keeps that state too (one planner = one dataset object).  With an `lq_jpeg` key the clip's JPEG quality is drawn last,
    and with an `lq_degrade` key its blur and noise, as REDSClipPlanner draws them."""

    def __init__(self, opt, client=None):
        self.opt = opt
        self.num_frame = opt['num_frame']
        self.scale, self.gt_size = opt['scale'], opt['gt_size']
        self.lq_size = self.gt_size // self.scale
        with open(opt['meta_info_file'], 'r') as fin:
            self.keys = [line.split(' ')[0] for line in fin]
        self.neighbor_list = [i + (9 - self.num_frame) // 2 for i in range(self.num_frame)]
        self.random_reverse = opt['random_reverse']
        self.lq_from_gt = training_lq_from_gt(opt)  # None: an LQ tree
        self.lq_jpeg = training_lq_jpeg(opt)  # None: no JPEG round trip of the LQ crops
        self.lq_degrade = training_lq_degrade(opt)  # None: no blur or noise on the LQ crops
        self.lq_mpeg = training_lq_mpeg(opt)  # None: no MPEG-style round trip of the LQ crop clips
        self.client = _make_client(opt, client, self.lq_from_gt is None)
        # the one place the two sources of LQ part: where the sizes come from and what load() stages
        if self.lq_from_gt is None:
            self.windows = None
            self._sizes = lambda key, frame: (self.client.size('lq', key, frame), self.client.size('gt', key, 'im4'))
            self.load = self._load_lq_tree
        else:
            self.windows = _WindowsFromGT(self.client, self.lq_size, self.gt_size, *self.lq_from_gt)
            self._sizes = lambda key, frame: self.windows.sizes(key, 'im4')
            self.load = self._load_gt_windows

    def __len__(self):
        return len(self.keys)

    def reset_epoch(self):
        """Canonical orientation of the neighbour list at the start of an epoch: what a fresh DataLoader worker's copy of the
        dataset has in the reference (workers are re-created per epoch), and what makes an epoch a function of (seed, epoch) only."""
        self.neighbor_list = [i + (9 - self.num_frame) // 2 for i in range(self.num_frame)]

    def plan(self, index, rng=random):
        if self.random_reverse and rng.random() < 0.5:
            self.neighbor_list.reverse()
        key = self.keys[index]
        frames = list(self.neighbor_list)
        (h_lq, w_lq), (h_gt, w_gt) = self._sizes(key, f'im{frames[0]}')
        if h_gt != h_lq * self.scale or w_gt != w_lq * self.scale:
            raise ValueError(f'Scale mismatches. GT ({h_gt}, {w_gt}) is not {self.scale}x multiplication of LQ ({h_lq}, {w_lq}).')
        if h_lq < self.lq_size or w_lq < self.lq_size:
            raise ValueError(f'LQ ({h_lq}, {w_lq}) is smaller than patch size ({self.lq_size}, {self.lq_size}). Please remove {key}.')
        top = rng.randint(0, h_lq - self.lq_size)
        left = rng.randint(0, w_lq - self.lq_size)
        flags = 0
        if self.opt['use_flip'] and rng.random() < 0.5:
            flags |= AUG_HFLIP
        if self.opt['use_rot'] and rng.random() < 0.5:
            flags |= AUG_VFLIP
        if self.opt['use_rot'] and rng.random() < 0.5:
            flags |= AUG_ROT90
        return ClipPlan(key, key, 4, frames, top, left, flags, _draw_jpeg_quality(self.lq_jpeg, rng), _draw_degrade(self.lq_degrade, rng),
                        _draw_mpeg_qscale(self.lq_mpeg, rng))

    def _load_gt_windows(self, plan, lq_out=None, gt_out=None):
        return self.windows.load(plan, [f'im{f}' for f in plan.frames], 'im4', lq_out, gt_out)

    def _load_lq_tree(self, plan, lq_out=None, gt_out=None):
        p, P, s = self.lq_size, self.gt_size, self.scale
        if lq_out is None:
            lq_out = np.empty((self.num_frame, p, p, 3), np.uint8)
        if gt_out is None:
            gt_out = np.empty((P, P, 3), np.uint8)
        for i, f in enumerate(plan.frames):
            lq_out[i] = decode_image(self.client.get('lq', plan.clip, f'im{f}'))[plan.top:plan.top + p, plan.left:plan.left + p]
        gt_out[...] = decode_image(self.client.get('gt', plan.clip, 'im4'))[plan.top * s:plan.top * s + P, plan.left * s:plan.left * s + P]
        return lq_out, gt_out


def make_planner(opt, client=None):
    """The planner of a training dataset option block, chosen like the reference's dataset registry does: by `type`
    (`REDSDataset` - the default - or `Vimeo90KDataset`; options/train/EDVR/*.yml use the former)."""
    kind = opt.get('type', 'REDSDataset')
    if kind == 'REDSDataset':
        return REDSClipPlanner(opt, client)
    if kind == 'Vimeo90KDataset':
        return Vimeo90KClipPlanner(opt, client)
    raise ValueError(f'dataset type {kind} is not supported (REDSDataset, Vimeo90KDataset)')


class EnlargedSampler:
    """Per-rank index order for iteration-based training (data_sampler.py:6-49): a seeded permutation of `ratio` copies of the
    dataset, strided over the ranks - the clip sharding of the data-parallel step (no data-path collective)."""

    def __init__(self, dataset, num_replicas, rank, ratio=1):
        self.dataset_size = len(dataset)
        self.num_replicas, self.rank, self.epoch = num_replicas, rank, 0
        self.num_samples = math.ceil(self.dataset_size * ratio / num_replicas)
        self.total_size = self.num_samples * num_replicas

    def __iter__(self):
        g = torch.Generator()
        g.manual_seed(self.epoch)
        indices = [v % self.dataset_size for v in torch.randperm(self.total_size, generator=g).tolist()]
        indices = indices[self.rank:self.total_size:self.num_replicas]
        assert len(indices) == self.num_samples
        return iter(indices)

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = epoch


# ------------------------------------------------------------------------------------------------ device side
def frames_to_device(frames_u8, flags=None, device='cuda', stream=None, swap_rb=False):
    """uint8 (n_clips, frames, h, w, 3) host array / tensor (pinned for an asynchronous copy) -> float32 device tensor
    (n_clips, frames, 3, h', w') in [0, 1]; flags: per-clip AUG_* bytes.  Runs on `stream` (default: the current stream)."""
    from . import ops
    t = torch.as_tensor(frames_u8)
    assert t.dtype == torch.uint8 and t.dim() == 5 and t.shape[-1] == 3, f'expected uint8 (n, f, h, w, 3), got {t.dtype} {tuple(t.shape)}'
    if not torch.cuda.is_available():
        raise RuntimeError('edvr_amd.data: no GPU - the conversion runs on the device only (there is no CPU fallback)')
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        dev = t.to(device, non_blocking=True)
        return ops.frames_u8_to_f32(dev, flags, swap_rb=swap_rb)


def read_img_seq(paths, device='cuda', require_mod_crop=False, scale=1, num_threads=8):
    """Validation frames (read_img_seq, data_util.py:11-33): image files -> (t, 3, h, w) RGB float32 in [0, 1] on the device."""
    def one(pth):
        with open(pth, 'rb') as f:
            img = decode_image(f.read())
        if require_mod_crop:
            img = img[:img.shape[0] - img.shape[0] % scale, :img.shape[1] - img.shape[1] % scale]
        return img
    with ThreadPoolExecutor(max(1, min(num_threads, len(paths)))) as pool:
        imgs = list(pool.map(one, [str(p) for p in paths]))
    return frames_to_device(np.stack(imgs)[None], None, device)[0]


# ------------------------------------------------------------------------------------------------ bicubic imresize (csrc/resize.hip)
IMRESIZE_SCALE_RANGE = (1 / 8, 8)


def _imresize_reach(n_in, n_out, scale, aa_down):
    """How many samples the taps of one axis reach before the first / beyond the last sample of the frame (sym_len_s / sym_len_e of
    calculate_weights_indices, matlab_functions.py:81-82): weights are non-zero strictly inside (u - kw / 2, u + kw / 2)."""
    kw = 4.0 / scale if aa_down else 4.0
    shift = 0.5 * (1.0 - 1.0 / scale)
    first = math.floor(1 / scale + shift - kw / 2) + 1  # 1-based
    last = math.ceil(n_out / scale + shift + kw / 2) - 1
    return max(0, 1 - first), max(0, last - n_in)


def imresize_shape(h, w, scale, antialiasing=True):
    """(h', w') = (ceil(h * scale), ceil(w * scale)) of imresize (matlab_functions.py:113).  ValueError for a scale outside [1/8, 8] and for
    a frame shorter on an axis than the symmetric extension reaches there (the reference indexes past its mirrored patch then): the
    check every caller of the kernel goes through before a launch.  Pure Python."""
    scale = float(scale)
    if not IMRESIZE_SCALE_RANGE[0] <= scale <= IMRESIZE_SCALE_RANGE[1]:
        raise ValueError(f'imresize: scale {scale} is outside [1/8, 8]')
    h, w = int(h), int(w)
    if h <= 0 or w <= 0:
        raise ValueError(f'imresize: empty {h} x {w} frame')
    out = math.ceil(h * scale), math.ceil(w * scale)
    aa_down = bool(antialiasing) and scale < 1
    for n_in, n_out, axis in ((h, out[0], 'rows'), (w, out[1], 'columns')):
        reach = _imresize_reach(n_in, n_out, scale, aa_down)
        if max(reach) > n_in:
            raise ValueError(f'imresize: {n_in} {axis} are fewer than the symmetric extension reaches at scale {scale} ({reach[0]} before, {reach[1]} after)')
    return out


def imresize(img, scale, antialiasing=True):
    """imresize (basicsr/utils/matlab_functions.py:88-170; MATLAB's antialiased bicubic, "BI") on the device: img (c, h, w) float32 in [0, 1]
    on the GPU -> (c, h', w') float32, not rounded or clamped.  Also batches: float32 (n, 3, h, w) -> (n, 3, h', w') and uint8 (n, h, w, 3)
    -> float32 (n, 3, h', w').  c = 3 (ops.imresize; its out_dtype=torch.uint8 gives the bytes a stored dataset holds).  CPU tensors raise
    NotImplementedError: there is no fallback."""
    from . import ops
    if not torch.is_tensor(img):
        raise NotImplementedError('edvr_amd.data.imresize takes device tensors (the numpy form of the reference runs on the host)')
    if img.dim() == 3 and img.dtype != torch.uint8:
        return ops.imresize(img[None], scale, antialiasing)[0]
    return ops.imresize(img, scale, antialiasing)


def gaussian_blur_kernel(ksize, sigma_x, sigma_y=None, theta=0.0):
    """A Gaussian blur kernel for ops.degrade: int32 (ksize, ksize) Q20 weights that sum to exactly 1 << 20.  The real
    weights are exp(-d' S^-1 d / 2) at the offsets d = (x, y) from the centre tap, S = R(theta) diag(sigma_x^2, sigma_y^2) R(theta)' -
    isotropic where sigma_y is None or equal, else an ellipse whose sigma_x axis is turned by theta from the x axis - normalised in
    float64 and rounded to Q20; the centre tap takes the rounding residue.  The integer blur then departs from the real-valued filter by
    at most ksize^2 255 2^-21 levels (0.054 at 21 x 21).  ValueError for a ksize that is even or outside 3 .. 21 and sigmas that are not
    finite and > 0."""
    from .ops import DEGRADE_ONE, degrade_ksize
    k = degrade_ksize(ksize)
    sx = float(sigma_x)
    sy = sx if sigma_y is None else float(sigma_y)
    theta = float(theta)
    if not (0 < sx < math.inf and 0 < sy < math.inf and math.isfinite(theta)):
        raise ValueError(f'gaussian_blur_kernel: sigmas are finite and > 0 and theta is finite, got {sigma_x!r}, {sigma_y!r}, {theta!r}')
    y, x = np.mgrid[-(k // 2):k // 2 + 1, -(k // 2):k // 2 + 1].astype(np.float64)
    c, s = math.cos(theta), math.sin(theta)
    u, v = c * x + s * y, -s * x + c * y  # R' d
    w = np.exp(-0.5 * ((u / sx) ** 2 + (v / sy) ** 2))
    q = np.rint(w / w.sum() * DEGRADE_ONE).astype(np.int64)
    q[k // 2, k // 2] += DEGRADE_ONE - q.sum()
    return q.astype(np.int32)


def degrade_spec(degrade, what='degrade'):
    """The `degrade` argument of lq_from_gt, checked: {'blur': {'ksize', 'sigma_x', 'sigma_y', 'theta'}, 'noise': {'sigma', 'shot',
    'gray'}}, either key optional -> (kernel int32 (k, k) | None, (read_sigma, shot, gray) | None).  Without 'ksize' the kernel is the
    smallest odd size that holds 3 sigma each side, 3 .. 21.  ValueError for unknown keys and bad values."""
    from .ops import DEGRADE_MAX_KSIZE, degrade_noise
    spec = dict(degrade)
    if not spec or set(spec) - {'blur', 'noise'}:
        raise ValueError(f"{what} takes 'blur' and / or 'noise', got {sorted(spec)}")
    kernel = noise = None
    if spec.get('blur') is not None:
        b = dict(spec['blur'])
        if set(b) - {'ksize', 'sigma_x', 'sigma_y', 'theta'} or 'sigma_x' not in b:
            raise ValueError(f"{what}: blur takes 'sigma_x' and optionally 'ksize', 'sigma_y' and 'theta', got {sorted(b)}")
        sy = b['sigma_x'] if b.get('sigma_y') is None else b['sigma_y']
        ksize = b.get('ksize')
        try:
            if ksize is None:
                reach = 3 * max(float(b['sigma_x']), float(sy))
                ksize = min(max(2 * math.ceil(reach) + 1, 3), DEGRADE_MAX_KSIZE) if math.isfinite(reach) else 3
            kernel = gaussian_blur_kernel(ksize, b['sigma_x'], sy, b.get('theta') or 0.0)
        except TypeError:
            raise ValueError(f'{what}: blur takes numbers, got {b!r}') from None
    if spec.get('noise') is not None:
        m = dict(spec['noise'])
        if set(m) - {'sigma', 'shot', 'gray'}:
            raise ValueError(f"{what}: noise takes 'sigma', 'shot' and 'gray', got {sorted(m)}")
        noise = degrade_noise((m.get('sigma') or 0.0, m.get('shot') or 0.0, m.get('gray', False)))
    return kernel, noise


def degrade_options(blur_sigma=None, blur_size=None, noise_sigma=None, noise_shot=None, noise_gray=False):
    """The `degrade` dict of lq_from_gt from the values the scripts take on their command lines (--blur-sigma SX [SY THETA], --blur-size K,
    --noise-sigma S, --noise-shot A, --noise-gray), checked; None where none of them asks for anything.  ValueError otherwise."""
    out = {}
    if blur_sigma is not None:
        if len(blur_sigma) not in (1, 3):
            raise ValueError('--blur-sigma takes SX or SX SY THETA')
        out['blur'] = dict(zip(('sigma_x', 'sigma_y', 'theta'), blur_sigma), ksize=blur_size)
    elif blur_size is not None:
        raise ValueError('--blur-size needs --blur-sigma')
    if noise_sigma is not None or noise_shot is not None:
        out['noise'] = {'sigma': noise_sigma or 0.0, 'shot': noise_shot or 0.0, 'gray': bool(noise_gray)}
    elif noise_gray:
        raise ValueError('--noise-gray needs --noise-sigma or --noise-shot')
    if not out:
        return None
    degrade_spec(out, 'degrade')
    return out


def lq_from_gt(gt, scale, quantize=None, degradation='bi', jpeg_quality=None, jpeg_subsampling='420', degrade=None, seed=0,
               mpeg_qscale=None, mpeg_gop=12, mpeg_search=7):
    """The x`scale` LQ frames of GT frames (t, 3, H, W) float32 on the device, H and W multiples of `scale`.  degradation 'bi': imresize
    by 1 / scale, rounded to 8 bits when `quantize` (the default; what a stored PNG dataset contains) - generate_bicubic_img.m without
    the files.  'bd': duf_downsample, NOT rounded unless `quantize` is given as True - VideoTestDUFDataset feeds the float result to the
    network.  jpeg_quality 1 .. 100: the 8-bit LQ frames go through a baseline JPEG round trip (ops.jpeg_roundtrip, DESIGN 4.16;
    jpeg_subsampling '420' or '444') before they become float - compression artifacts on top of the downsampling; it works on bytes, so
    it implies `quantize` and is a ValueError with quantize=False.  degrade = {'blur': {'ksize', 'sigma_x', 'sigma_y', 'theta'}, 'noise':
    {'sigma', 'shot', 'gray'}} (either key optional; degrade_spec): the 8-bit LQ frames are blurred and made noisy (ops.degrade, DESIGN
    4.17) after the downsampling and before the JPEG round trip - blur, noise, compression, the first-order degradation model; frame i of
    the call takes its noise field from the 64-bit key `seed` and frame index i.  It too implies `quantize`.  mpeg_qscale 1 .. 31: the
    8-bit LQ frames of the call, ONE clip in order, go through the MPEG-style I / P round trip (ops.mpeg_roundtrip; an
    intra frame every mpeg_gop frames, 0 = the first alone; motion search range mpeg_search 0 .. 15) between `degrade` and the JPEG
    round trip - optics, sensor, codec; it implies `quantize` under the same rule."""
    from . import ops
    if degradation not in DEGRADATIONS:
        raise ValueError(f'degradation must be one of {DEGRADATIONS}, got {degradation!r}')
    if jpeg_quality is not None:
        jpeg_quality = ops.jpeg_quality(jpeg_quality, 'jpeg_quality')
        if jpeg_subsampling not in ops.JPEG_SUBSAMPLINGS:
            raise ValueError(f'jpeg_subsampling must be one of {ops.JPEG_SUBSAMPLINGS}, got {jpeg_subsampling!r}')
        if quantize is not None and not quantize:
            raise ValueError('jpeg_quality compresses the 8-bit LQ frames: it cannot go with quantize=False')
        quantize = True
    if mpeg_qscale is not None:
        mpeg_qscale, mpeg_gop, mpeg_search = ops.mpeg_qscale(mpeg_qscale, 'mpeg_qscale'), ops.mpeg_gop(mpeg_gop, 'mpeg_gop'), ops.mpeg_search(mpeg_search, 'mpeg_search')
        if quantize is not None and not quantize:
            raise ValueError('mpeg_qscale compresses the 8-bit LQ frames: it cannot go with quantize=False')
        quantize = True
    if degrade is not None:
        kernel, noise = degrade_spec(degrade)
        if quantize is not None and not quantize:
            raise ValueError('degrade works on the 8-bit LQ frames: it cannot go with quantize=False')
        quantize = True
    if quantize is None:
        quantize = degradation == 'bi'
    down = (lambda **kw: ops.imresize(gt, 1 / scale, **kw)) if degradation == 'bi' else (lambda **kw: ops.bd_downsample(gt, scale, **kw))
    if not quantize:
        return down()
    lq = down(out_dtype=torch.uint8)
    if degrade is not None:
        lq = ops.degrade(lq, kernel, noise, seed)
    if mpeg_qscale is not None:
        lq = ops.mpeg_roundtrip(lq, mpeg_qscale, mpeg_gop, mpeg_search)
    if jpeg_quality is not None:
        lq = ops.jpeg_roundtrip(lq, jpeg_quality, jpeg_subsampling)
    return ops.frames_u8_to_f32(lq[None])[0]


# ------------------------------------------------------------------------------------------------ BD downsampling (csrc/bd.hip)
DEGRADATIONS = ('bi', 'bd')
BD_SCALES = (2, 3, 4)
BD_KERNEL_SIZE = 13


def bd_weights(scale):
    """The 13 float64 weights g of duf_downsample's separable form: the 1-D kernel scipy.ndimage.gaussian_filter applies per axis at
    sigma = 0.4 * scale (generate_gaussian_kernel, data_util.py:281-296), truncated at int(4 sigma + 0.5) samples = 3, 5, 6 (7, 11, 13
    non-zero taps) and normalised; np.outer(g, g) is the reference's 13 x 13 filter exactly.  Written as scipy writes it, so that the
    float64 values are the same; scipy is not needed."""
    if scale not in BD_SCALES or isinstance(scale, bool):
        raise ValueError(f'duf_downsample: scale must be one of {BD_SCALES}, got {scale!r}')
    sigma = 0.4 * int(scale)
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    g = np.zeros(BD_KERNEL_SIZE)
    g[BD_KERNEL_SIZE // 2 - radius:BD_KERNEL_SIZE // 2 + radius + 1] = phi
    return g


def bd_shape(h, w, scale):
    """(h', w') = (ceil(h / scale), ceil(w / scale)) of duf_downsample (pad 6 + 2 scale, stride scale, crop 2 per side).  ValueError for a
    scale outside {2, 3, 4} and for a frame of fewer than 7 rows or columns (one reflection must cover the kernel's reach of 6; the
    reference itself needs more than 6 + 2 scale): the check every caller of the kernel goes through before a launch.  Pure Python."""
    if isinstance(scale, bool) or scale not in BD_SCALES or int(scale) != scale:
        raise ValueError(f'duf_downsample: scale must be one of {BD_SCALES}, got {scale!r}')
    h, w, scale = int(h), int(w), int(scale)
    if min(h, w) < BD_KERNEL_SIZE // 2 + 1:
        raise ValueError(f'duf_downsample: a {h} x {w} frame has fewer than {BD_KERNEL_SIZE // 2 + 1} rows or columns, the reach of the kernel\'s one reflection')
    return -(-h // scale), -(-w // scale)


def duf_downsample(x, kernel_size=13, scale=4):
    """duf_downsample (basicsr/data/data_util.py:299-331; the "BD" degradation of the DUF code) on the device: x (t, c, h, w) or
    (b, t, c, h, w) float32 in [0, 1] on the GPU -> the same with (ceil(h / scale), ceil(w / scale)), float32, not rounded or clamped; also
    uint8 (n, h, w, 3) -> float32 (n, 3, h', w').  c = 3, scale in {2, 3, 4}, kernel_size 13 (the only size anything uses; the
    reference's other sizes change where sigma is truncated).  CPU tensors raise NotImplementedError: there is no fallback."""
    from . import ops
    if kernel_size != BD_KERNEL_SIZE:
        raise ValueError(f'duf_downsample: kernel_size must be {BD_KERNEL_SIZE}, got {kernel_size}')
    if not torch.is_tensor(x):
        raise NotImplementedError('edvr_amd.data.duf_downsample takes device tensors')
    if x.dim() == 5 and x.dtype != torch.uint8:
        bd_shape(x.shape[-2], x.shape[-1], scale)
        b, t = x.shape[:2]
        out = ops.bd_downsample(x.reshape(b * t, *x.shape[2:]), scale)
        return out.view(b, t, *out.shape[1:])
    return ops.bd_downsample(x, scale)


# ------------------------------------------------------------------------------------------------ LQ crops from GT windows (training)
LQ_WINDOW_SCALES = (2, 3, 4)
LQ_WINDOW_RECORD_INTS = 8  # y0, x0 (the window's origin in its frame), H, W (the mod-cropped frame), top, left (the LQ crop's origin), 2 unused


def _lq_taps(i, scale, degradation):
    """(first, last) unreflected GT sample, 0-based, that LQ sample `i` of one axis reads with non-zero weight.  'bi': the support of
    _imresize_reach - strictly inside (u - kw / 2, u + kw / 2), u = x / f + 0.5 (1 - 1 / f) for the 1-based x = i + 1, f = 1 / scale,
    kw = 4 / f - in exact arithmetic (u is a multiple of 1/2).  'bd': the taps i * scale - 6 .. i * scale + 6 of bd_shape's 13-tap kernel
    whose weight bd_weights does not truncate to zero."""
    if degradation == 'bi':
        from fractions import Fraction
        f = Fraction(1, scale)
        kw, u = 4 / f, (i + 1) / f + Fraction(1, 2) * (1 - 1 / f)
        return math.floor(u - kw / 2) + 1 - 1, math.ceil(u + kw / 2) - 1 - 1
    nz = np.flatnonzero(bd_weights(scale))
    return i * scale - BD_KERNEL_SIZE // 2 + int(nz[0]), i * scale - BD_KERNEL_SIZE // 2 + int(nz[-1])


def _lq_window_args(size, scale, degradation):
    if degradation not in DEGRADATIONS:
        raise ValueError(f'lq_window: degradation must be one of {DEGRADATIONS}, got {degradation!r}')
    if isinstance(scale, bool) or scale not in LQ_WINDOW_SCALES or int(scale) != scale:
        raise ValueError(f'lq_window: scale must be one of {LQ_WINDOW_SCALES}, got {scale!r} (degradation {degradation!r})')
    if int(size) != size or size < 1:
        raise ValueError(f'lq_window: a crop of {size} LQ samples is empty (gt_size is smaller than the scale)')
    return int(size), int(scale)


def lq_window_extent(size, scale, degradation):
    """How many GT samples per axis the window of ANY crop of `size` LQ samples has: the unreflected span of its taps of non-zero weight,
    first tap of the first sample to last tap of the last (the folded range of lq_window is never longer).  One number per
    (size, scale, degradation), so staging slots have one size."""
    size, scale = _lq_window_args(size, scale, degradation)
    extent = _lq_taps(size - 1, scale, degradation)[1] - _lq_taps(0, scale, degradation)[0] + 1
    reach = -_lq_taps(0, scale, degradation)[0]  # samples before the frame that the first crop reflects (their mirror images: 0 .. reach - 1 / 1 .. reach)
    if reach > extent - (degradation == 'bd'):
        raise ValueError(f'lq_window: a crop of {size} LQ samples has a window of {extent} GT samples, shorter than the {reach} one reflection reaches')
    return extent


def lq_window(start, size, n_lq, scale, degradation):
    """One axis of a training crop made from GT: LQ samples [start, start + size) of a frame of n_lq LQ samples (n_lq * scale GT samples,
    i.e. mod-cropped) read, with non-zero weight, GT samples [lo, hi) - AFTER the frame's boundary rule (imresize's symmetric extension
    ... 1 0 | 0 1 ..., duf_downsample's reflection ... 2 1 | 0 1 2 ...) has folded the taps before the first and beyond the last sample
    back in.  Returns (lo, hi, extent): extent = lq_window_extent(size, scale, degradation) >= hi - lo for every start, and the window
    [lq_window_origin(lo, n_lq * scale, extent), + extent) holds [lo, hi) and lies inside the frame.  ValueError (as imresize_shape and
    bd_shape raise it) for a scale outside {2, 3, 4}, a crop outside the frame, and a frame with fewer GT samples than the extent - one
    reflection would not land inside the window.  Pure Python."""
    extent = lq_window_extent(size, scale, degradation)
    start, n_lq = int(start), int(n_lq)
    n = n_lq * scale
    if start < 0 or start + size > n_lq:
        raise ValueError(f'lq_window: LQ samples [{start}, {start + size}) leave the frame of {n_lq}')
    if n < extent:
        raise ValueError(f'lq_window: {n} GT samples are fewer than the window of {extent} a crop of {size} LQ samples at x{scale} {degradation!r} reads')
    a, b = _lq_taps(start, scale, degradation)[0], _lq_taps(start + size - 1, scale, degradation)[1]
    ra, rb = (-a - 1, 2 * n - 1 - b) if degradation == 'bi' else (-a, 2 * (n - 1) - b)  # where the boundary rule sends a < 0 and b > n - 1
    lo, hi = max(a, 0), min(b, n - 1)
    if a < 0:
        hi = max(hi, ra)
    if b > n - 1:
        lo = min(lo, rb)
    assert 0 <= lo <= hi < n and hi - lo < extent, (lo, hi, n, extent)
    return lo, hi + 1, extent


def lq_window_origin(lo, n, extent):
    """First GT sample of the fixed-size window that holds the range lq_window returned: the range's own start, pulled back where the
    window would leave the frame of n GT samples."""
    return min(lo, n - extent)


def lq_window_pitch(extent):
    """Bytes of one window row in a staging slot: 3 * extent, rounded up so that every row starts on a 16-byte boundary."""
    return -(-3 * extent // 16) * 16


def lq_window_size(extent, scale, degradation):
    """The crop size whose window has `extent` GT samples (the inverse of lq_window_extent; ValueError if there is none)."""
    lo = lq_window_extent(1, scale, degradation)
    if extent < lo or (extent - lo) % scale:
        raise ValueError(f'lq_window: no crop has a window of {extent} GT samples at x{scale} {degradation!r}')
    return 1 + (extent - lo) // scale


def training_lq_from_gt(opt):
    """The `lq_from_gt` key of a TRAINING option block: None with an LQ tree (dataroot_lq given: nothing else is looked at), else
    (scale, degradation) after the checks VideoTestClips makes - plus scale == opt['scale'] and scale in {2, 3, 4}, and no 'quantize':
    False (the LQ crops are always the 8-bit values a stored tree holds)."""
    if opt.get('dataroot_lq') is not None:
        return None
    if not opt.get('lq_from_gt'):
        raise ValueError("dataroot_lq is None: give an LQ tree, or lq_from_gt = {'scale': s, 'degradation': 'bi' | 'bd'} to make the LQ crops from GT")
    spec = dict(opt['lq_from_gt'])
    degradation = spec.get('degradation', 'bi')
    if degradation not in DEGRADATIONS:
        raise ValueError(f'lq_from_gt: degradation must be one of {DEGRADATIONS}, got {degradation!r}')
    scale = spec['scale']
    if isinstance(scale, bool) or scale not in LQ_WINDOW_SCALES or int(scale) != scale:
        raise ValueError(f'lq_from_gt: scale {scale!r} is not one of {LQ_WINDOW_SCALES} (degradation {degradation!r})')
    if scale != opt['scale']:
        raise ValueError(f"lq_from_gt: scale {scale} is not the dataset's scale {opt['scale']}")
    if not spec.get('quantize', True):
        raise ValueError('lq_from_gt: training LQ crops are always quantised to 8 bits (what a stored LQ tree holds)')
    lq_window_extent(opt['gt_size'] // int(scale), int(scale), degradation)  # refuses a gt_size whose crop is empty
    return int(scale), degradation


class _WindowsFromGT:
    """What a planner does instead of reading an LQ tree (lq_from_gt): sizes from the GT header, and load() stages per frame the window of
    the decoded GT that the LQ crop reads plus its table record, for ops.lq_crops_from_windows."""

    def __init__(self, client, lq_size, gt_size, scale, degradation):
        self.client, self.lq_size, self.gt_size, self.scale, self.degradation = client, lq_size, gt_size, scale, degradation
        self.extent = lq_window_extent(lq_size, scale, degradation)
        self.pitch = lq_window_pitch(self.extent)

    def sizes(self, clip, frame):
        """((h_lq, w_lq), (h_gt, w_gt)) of the mod-cropped GT frame; ValueError where a frame is smaller than the window."""
        h, w = self.client.size('gt', clip, frame)
        h, w = h - h % self.scale, w - w % self.scale
        if min(h, w) < self.extent:
            raise ValueError(f'GT ({h}, {w}) is smaller than the window of {self.extent} samples that a {self.lq_size} x {self.lq_size} LQ crop '
                             f'reads at x{self.scale} {self.degradation!r}. Please remove {clip}/{frame}.')
        return (h // self.scale, w // self.scale), (h, w)

    def empty(self, num_frame):
        return np.zeros((num_frame, self.extent, self.pitch), np.uint8), np.zeros((num_frame, LQ_WINDOW_RECORD_INTS), np.int32)

    def load(self, plan, names, center, lq_out, gt_out):
        p, P, s, e = self.lq_size, self.gt_size, self.scale, self.extent
        if lq_out is None:
            lq_out = self.empty(len(names))
        if gt_out is None:
            gt_out = np.empty((P, P, 3), np.uint8)
        win, tab = lq_out
        have_gt = False
        for i, name in enumerate(names):
            img = decode_image(self.client.get('gt', plan.clip, name))
            H, W = img.shape[0] - img.shape[0] % s, img.shape[1] - img.shape[1] % s
            y0 = lq_window_origin(lq_window(plan.top, p, H // s, s, self.degradation)[0], H, e)
            x0 = lq_window_origin(lq_window(plan.left, p, W // s, s, self.degradation)[0], W, e)
            win[i, :, :3 * e] = img[y0:y0 + e, x0:x0 + e].reshape(e, 3 * e)
            tab[i] = (y0, x0, H, W, plan.top, plan.left, 0, 0)
            if name == center and not have_gt:
                gt_out[...] = img[plan.top * s:plan.top * s + P, plan.left * s:plan.left * s + P]
                have_gt = True
        if not have_gt:
            gt_out[...] = decode_image(self.client.get('gt', plan.clip, center))[plan.top * s:plan.top * s + P, plan.left * s:plan.left * s + P]
        return lq_out, gt_out


class VideoTestClips:
    """VideoTestDataset (basicsr/data/video_test_dataset.py:11-147) with the frames kept on the device.

    Same `opt` keys (dataroot_gt, dataroot_lq, io_backend, cache_data, name, num_frame, padding, optional meta_info_file), same
    `data_info` lists and the same items from __getitem__ ({'lq' (t, c, h, w), 'gt' (c, h, w), 'folder', 'idx', 'border',
    'lq_path'}), except that the tensors live on the GPU: a clip is decoded once on the host (threads), converted by
    edvr_frames_u8_to_f32 and cached there (100 REDS4 frames: 83 MB LQ + 1.1 GB GT in fp32, nothing next to 288 GB), so that
    metrics.validate_clip can batch the windows of a whole clip.  clip(folder) returns the (lq, gt) pair of one folder.

    Without an LQ folder: dataroot_lq None and lq_from_gt = {'scale': 4, 'quantize': True} derive the LQ frames from the decoded GT on
    the device (lq_from_gt above; GT mod-cropped to a multiple of the scale first, as read_img_seq(require_mod_crop=True) does);
    lq_from_gt = {'scale': 4, 'degradation': 'bd'} makes them with duf_downsample instead (not quantised unless 'quantize' says so);
    'jpeg_quality': q (and 'jpeg_subsampling': '420' | '444') adds the JPEG round trip of lq_from_gt above, which implies 'quantize'
    and is a ValueError with 'quantize': False; 'degrade': {'blur': ..., 'noise': ...} (and 'degrade_seed': a 64-bit key) adds the blur
    and noise of lq_from_gt above, before the JPEG round trip, under the same rule - frame i of a read takes the noise field of index i;
    'mpeg_qscale': q (and 'mpeg_gop', 'mpeg_search') adds the MPEG-style round trip of lq_from_gt above, the frames of a read being one
    clip, between the two, under the same rule; it needs 'cache_data': True, so that a folder is read and coded whole."""

    def __init__(self, opt, device='cuda'):
        import glob
        import os.path as osp
        from .metrics import generate_frame_indices
        self._indices = generate_frame_indices
        self.opt, self.device = opt, device
        self.cache_data = opt['cache_data']
        self.gt_root, self.lq_root = opt['dataroot_gt'], opt['dataroot_lq']
        self.lq_from_gt = dict(opt['lq_from_gt']) if self.lq_root is None and opt.get('lq_from_gt') else None
        if self.lq_from_gt is not None:
            degradation = self.lq_from_gt.get('degradation', 'bi')
            if degradation not in DEGRADATIONS:
                raise ValueError(f'lq_from_gt: degradation must be one of {DEGRADATIONS}, got {degradation!r}')
            jpeg = {k: self.lq_from_gt[k] for k in ('jpeg_quality', 'jpeg_subsampling') if self.lq_from_gt.get(k) is not None}
            if jpeg.get('jpeg_quality') is None:
                jpeg = {}
            extra = {'degrade': self.lq_from_gt['degrade'], 'seed': self.lq_from_gt.get('degrade_seed')} if self.lq_from_gt.get('degrade') is not None else {}
            mpeg = {k: self.lq_from_gt[k] for k in ('mpeg_qscale', 'mpeg_gop', 'mpeg_search') if self.lq_from_gt.get(k) is not None}
            if mpeg.get('mpeg_qscale') is None:
                mpeg = {}
            self.lq_from_gt = {'scale': int(self.lq_from_gt['scale']),
                               'quantize': bool(self.lq_from_gt.get('quantize', degradation == 'bi' or bool(jpeg) or bool(extra) or bool(mpeg))),
                               'degradation': degradation}
            if mpeg:
                from . import ops
                mpeg = {'mpeg_qscale': ops.mpeg_qscale(mpeg['mpeg_qscale'], 'lq_from_gt: mpeg_qscale'),
                        'mpeg_gop': ops.mpeg_gop(mpeg.get('mpeg_gop', 12), 'lq_from_gt: mpeg_gop'),
                        'mpeg_search': ops.mpeg_search(mpeg.get('mpeg_search', 7), 'lq_from_gt: mpeg_search')}
                if not self.lq_from_gt['quantize']:
                    raise ValueError("lq_from_gt: mpeg_qscale compresses the 8-bit LQ frames: it cannot go with 'quantize': False")
                if not self.cache_data:  # (a window read on its own repeats and reorders frames at the clip's ends)
                    raise ValueError("lq_from_gt: mpeg_qscale codes a folder's frames as one clip: it needs 'cache_data': True")
            self._lq_mpeg = mpeg
            if jpeg:
                from .ops import JPEG_SUBSAMPLINGS, jpeg_quality
                jpeg['jpeg_quality'] = jpeg_quality(jpeg['jpeg_quality'], 'lq_from_gt: jpeg_quality')
                if jpeg.setdefault('jpeg_subsampling', '420') not in JPEG_SUBSAMPLINGS:
                    raise ValueError(f"lq_from_gt: jpeg_subsampling must be one of {JPEG_SUBSAMPLINGS}, got {jpeg['jpeg_subsampling']!r}")
                if not self.lq_from_gt['quantize']:
                    raise ValueError("lq_from_gt: jpeg_quality compresses the 8-bit LQ frames: it cannot go with 'quantize': False")
            self._lq_jpeg = jpeg
            if extra:
                degrade_spec(extra['degrade'], 'lq_from_gt: degrade')  # ValueError now, not at the first clip
                if not self.lq_from_gt['quantize']:
                    raise ValueError("lq_from_gt: degrade works on the 8-bit LQ frames: it cannot go with 'quantize': False")
                extra['seed'] = int(extra.get('seed') or 0)
            self._lq_degrade = extra
            if degradation == 'bd':
                if self.lq_from_gt['scale'] not in BD_SCALES:
                    raise ValueError(f"lq_from_gt: scale {self.lq_from_gt['scale']} is not one of {BD_SCALES} (degradation 'bd')")
            elif not 1 <= self.lq_from_gt['scale'] <= 1 / IMRESIZE_SCALE_RANGE[0]:
                raise ValueError(f"lq_from_gt: scale {self.lq_from_gt['scale']} is outside 1..8")
            self.lq_root = self.gt_root  # the 'LQ' files of data_info are the GT files the frames are made from
        assert dict(opt['io_backend'])['type'] != 'lmdb', 'No need to use lmdb during validation/test.'
        self.data_info = {'lq_path': [], 'gt_path': [], 'folder': [], 'idx': [], 'border': []}
        self.imgs_lq, self.imgs_gt, self._cache = {}, {}, {}
        if 'meta_info_file' in opt:
            with open(opt['meta_info_file'], 'r') as fin:
                subfolders = [line.split(' ')[0] for line in fin]
            subfolders_lq = [osp.join(self.lq_root, key) for key in subfolders]
            subfolders_gt = [osp.join(self.gt_root, key) for key in subfolders]
        else:
            subfolders_lq = sorted(glob.glob(osp.join(self.lq_root, '*')))
            subfolders_gt = sorted(glob.glob(osp.join(self.gt_root, '*')))
        if opt['name'].lower() not in ['vid4', 'reds4', 'redsofficial']:
            raise ValueError(f'Non-supported video test dataset: {type(opt["name"])}')

        def files(folder):  # scandir(full_path=True): plain files, no dot files, sorted by the caller
            return sorted(osp.join(folder, e.name) for e in os.scandir(folder) if not e.name.startswith('.') and e.is_file())

        for sub_lq, sub_gt in zip(subfolders_lq, subfolders_gt):
            name = osp.basename(sub_lq)
            paths_lq, paths_gt = files(sub_lq), files(sub_gt)
            max_idx = len(paths_lq)
            assert max_idx == len(paths_gt), f'Different number of images in lq ({max_idx}) and gt folders ({len(paths_gt)})'
            self.data_info['lq_path'].extend(paths_lq)
            self.data_info['gt_path'].extend(paths_gt)
            self.data_info['folder'].extend([name] * max_idx)
            self.data_info['idx'].extend(f'{i}/{max_idx}' for i in range(max_idx))
            border = [0] * max_idx
            for i in range(opt['num_frame'] // 2):
                border[i] = 1
                border[max_idx - i - 1] = 1
            self.data_info['border'].extend(border)
            self.imgs_lq[name], self.imgs_gt[name] = paths_lq, paths_gt

    def __len__(self):
        return len(self.data_info['gt_path'])

    @property
    def folders(self):
        return list(self.imgs_lq)

    def clip(self, folder):
        """(lq (t, 3, h, w), gt (t, 3, H, W)) of one folder on the device."""
        if folder in self._cache:
            return self._cache[folder]
        pair = self._read(self.imgs_lq[folder], self.imgs_gt[folder])
        if self.cache_data:
            self._cache[folder] = pair
        return pair

    def _read(self, paths_lq, paths_gt):
        """(lq, gt) frames of the listed files; with lq_from_gt the LQ frames come from the GT files at paths_lq."""
        if self.lq_from_gt is None:
            return read_img_seq(paths_lq, self.device), read_img_seq(paths_gt, self.device)
        scale, quantize = self.lq_from_gt['scale'], self.lq_from_gt['quantize']
        gt = read_img_seq(paths_gt, self.device, require_mod_crop=True, scale=scale)
        src = gt if list(paths_lq) == list(paths_gt) else read_img_seq(paths_lq, self.device, require_mod_crop=True, scale=scale)
        return lq_from_gt(src, scale, quantize, self.lq_from_gt['degradation'], **self._lq_jpeg, **self._lq_degrade, **self._lq_mpeg), gt

    def __getitem__(self, index):
        folder = self.data_info['folder'][index]
        idx, max_idx = (int(v) for v in self.data_info['idx'][index].split('/'))
        select_idx = self._indices(idx, max_idx, self.opt['num_frame'], padding=self.opt['padding'])
        if self.cache_data:
            lq, gt = self.clip(folder)
            imgs_lq = lq.index_select(0, torch.tensor(select_idx, device=lq.device))
            img_gt = gt[idx]
        else:
            imgs_lq, gts = self._read([self.imgs_lq[folder][i] for i in select_idx], [self.imgs_gt[folder][idx]])
            img_gt = gts[0]
        return {'lq': imgs_lq, 'gt': img_gt, 'folder': folder, 'idx': self.data_info['idx'][index],
                'border': self.data_info['border'][index], 'lq_path': self.data_info['lq_path'][index]}


class VideoTestDUFClips(VideoTestClips):
    """VideoTestDUFDataset (basicsr/data/video_test_dataset.py:231-290): VideoTestClips with the reference's two extra keys.  With
    opt['use_duf_downsampling'] true the LQ windows are made from the GT frames - mod-cropped to opt['scale'], duf_downsample on the
    device, not quantised - and dataroot_lq only names the items: data_info['lq_path'] is each GT file's path under dataroot_lq (the
    folder need not exist; None keeps the GT paths).  With the key false or absent this is VideoTestClips."""

    def __init__(self, opt, device='cuda'):
        import os.path as osp
        self.use_duf_downsampling = bool(opt.get('use_duf_downsampling', False))
        if not self.use_duf_downsampling:
            super().__init__(opt, device)
            return
        if opt.get('scale') not in BD_SCALES:
            raise ValueError(f"use_duf_downsampling: opt['scale'] must be one of {BD_SCALES}, got {opt.get('scale')!r}")
        names_root = opt.get('dataroot_lq')
        super().__init__(dict(opt, dataroot_lq=None, lq_from_gt={'scale': opt['scale'], 'degradation': 'bd', 'quantize': False}), device)
        self.opt = opt
        if names_root is not None:
            self.data_info['lq_path'] = [osp.join(names_root, osp.relpath(p, self.gt_root)) for p in self.data_info['gt_path']]


class VideoTestVimeo90KClips:
    """VideoTestVimeo90KDataset (basicsr/data/video_test_dataset.py:150-233; options/test/EDVR/test_EDVR_L_x4_SR_Vimeo90K.yml):
    one item per septuplet listed in `meta_info_file`, the `num_frame` centre frames `im{i}.png` of the sequence as LQ window and
    `im4.png` as GT; same `data_info` and item keys as the reference, tensors decoded on the host and converted on the device."""

    def __init__(self, opt, device='cuda'):
        import os.path as osp
        self.opt, self.device = opt, device
        if opt['cache_data']:
            raise NotImplementedError('cache_data in Vimeo90K-Test dataset is not implemented.')
        assert dict(opt['io_backend'])['type'] != 'lmdb', 'No need to use lmdb during validation/test.'
        self.gt_root, self.lq_root = opt['dataroot_gt'], opt['dataroot_lq']
        self.data_info = {'lq_path': [], 'gt_path': [], 'folder': [], 'idx': [], 'border': []}
        neighbor_list = [i + (9 - opt['num_frame']) // 2 for i in range(opt['num_frame'])]
        with open(opt['meta_info_file'], 'r') as fin:
            subfolders = [line.split(' ')[0] for line in fin]
        for idx, subfolder in enumerate(subfolders):
            self.data_info['gt_path'].append(osp.join(self.gt_root, subfolder, 'im4.png'))
            self.data_info['lq_path'].append([osp.join(self.lq_root, subfolder, f'im{i}.png') for i in neighbor_list])
            self.data_info['folder'].append('vimeo90k')
            self.data_info['idx'].append(f'{idx}/{len(subfolders)}')
            self.data_info['border'].append(0)

    def __len__(self):
        return len(self.data_info['gt_path'])

    def __getitem__(self, index):
        lq_path = self.data_info['lq_path'][index]
        return {'lq': read_img_seq(lq_path, self.device), 'gt': read_img_seq([self.data_info['gt_path'][index]], self.device)[0],
                'folder': self.data_info['folder'][index], 'idx': self.data_info['idx'][index],
                'border': self.data_info['border'][index], 'lq_path': lq_path[self.opt['num_frame'] // 2]}


def epoch_rng(seed, epoch):
    """The random stream of one epoch of one rank: a function of (seed, epoch) only, so an epoch is reproducible however far the
    prefetch of the previous one had run when reset() cut it."""
    return random.Random(seed * 1000003 + epoch)


class REDSDeviceLoader:
    """REDSDataset (or Vimeo90KDataset: `opt['type']`) + DataLoader + EnlargedSampler + CUDAPrefetcher in one object, one per rank.

    next() -> {'lq': (b, t, 3, p, p), 'gt': (b, 3, P, P) float32 device tensors, 'key': [str]} or None at the end of the epoch
    (CUDAPrefetcher.next, prefetch_dataloader.py:118-122); reset() starts the next epoch.  A planner thread makes the random
    decisions serially from epoch_rng(seed + rank, epoch) (deterministic whatever the thread count and prefetch depth), `num_threads` workers decode into pinned staging
    slots, the copy + conversion of batch k+1 run on a side stream while batch k trains.

    opt['lq_jpeg'] = {'quality': q | [lo, hi], 'subsampling': '420', 'prob': 1.0} (training_lq_jpeg; either source of LQ): the LQ crop
    bytes of the batch go through ONE ops.jpeg_roundtrip launch at each clip's planned quality before the conversion to float - GT is
    untouched, and the 8 x 8 block grid starts at the crop's corner.

    opt['lq_degrade'] = {'blur': {...}, 'noise': {...}} (training_lq_degrade; either source of LQ): before that, ONE ops.degrade launch
    blurs the LQ crop bytes with each clip's planned kernel and adds its planned noise, an independent field per frame, in crop
    coordinates and before flip / rotation.

    opt['lq_mpeg'] = {'qscale': q | [lo, hi], 'search': 7, 'prob': 1.0} (training_lq_mpeg; either source of LQ): between the two, ONE
    ops.mpeg_roundtrip call codes the (n, t, p, p, 3) LQ crop bytes as n clips at each clip's planned quantiser scale - frame 0 of the
    crop clip is the only intra frame, the macroblock grid and the clamp of the motion search are anchored at the crop."""

    def __init__(self, opt, batch_size, device='cuda', rank=0, world_size=1, ratio=1, seed=0, num_threads=8, depth=3, drop_last=True,
                 client=None):
        if not torch.cuda.is_available():
            raise RuntimeError('REDSDeviceLoader needs a GPU (uint8 staging is converted on the device; there is no CPU fallback)')
        self.planner = make_planner(opt, client)  # REDSDataset (default) or Vimeo90KDataset, by opt['type']
        self.sampler = EnlargedSampler(self.planner, world_size, rank, ratio)
        self.batch_size, self.device, self.drop_last = batch_size, torch.device(device), drop_last
        self.seed = seed + rank  # the reference seeds every worker with seed + rank * workers + id (data/__init__.py)
        self.pool = ThreadPoolExecutor(num_threads)
        t, p, P = self.planner.num_frame, self.planner.lq_size, self.planner.gt_size
        # the one place the two sources of LQ part: what a slot's LQ half holds and how it becomes (b, t, p, p, 3) bytes on the device
        if self.planner.lq_from_gt is None:
            lq_slots = [torch.empty((batch_size, t, p, p, 3), dtype=torch.uint8).pin_memory() for _ in range(depth)]
            self._lq_views = [s.numpy() for s in lq_slots]  # [slot][sample] -> what load() writes the LQ into
            self._lq_upload = self._upload_lq_crops
        else:
            w = self.planner.windows
            n_win, n_tab = batch_size * t * w.extent * w.pitch, batch_size * t * LQ_WINDOW_RECORD_INTS * 4
            lq_slots = [torch.zeros(n_win + n_tab, dtype=torch.uint8).pin_memory() for _ in range(depth)]  # windows, then their table: one copy
            self._win_shape, self._n_win = (batch_size * t, w.extent, w.pitch), n_win
            self._tables = [s[n_win:].view(torch.int32).view(batch_size * t, LQ_WINDOW_RECORD_INTS) for s in lq_slots]
            self._lq_views = [list(zip(s[:n_win].view(batch_size, t, w.extent, w.pitch).numpy(), tab.view(batch_size, t, -1).numpy()))
                              for s, tab in zip(lq_slots, self._tables)]
            self._lq_upload = self._upload_gt_windows
        self.slots = [(lq, torch.empty((batch_size, 1, P, P, 3), dtype=torch.uint8).pin_memory()) for lq in lq_slots]
        # lq_jpeg: one quality per LQ frame, in a pinned table per slot (copied on the loader's stream before the slot is handed back)
        self._jpeg_tables = [torch.zeros(batch_size * t, dtype=torch.int32).pin_memory() for _ in lq_slots] if self.planner.lq_jpeg else None
        # lq_mpeg: one quantiser scale per clip, likewise
        self._mpeg_tables = [torch.zeros(batch_size, dtype=torch.int32).pin_memory() for _ in lq_slots] if self.planner.lq_mpeg else None
        from . import ops
        # lq_degrade: one record per LQ frame, then room for one 21 x 21 kernel per clip, in a pinned int32 buffer per slot: one copy
        self._n_degrade_table = batch_size * t * ops.DEGRADE_RECORD_INTS
        self._degrade_slots = ([torch.zeros(self._n_degrade_table + batch_size * ops.DEGRADE_MAX_KSIZE ** 2, dtype=torch.int32).pin_memory() for _ in lq_slots]
                               if self.planner.lq_degrade else None)
        self.stream = torch.cuda.Stream(self.device)
        self.epoch = 0
        self._start()

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    # ---- producer
    def _start(self):
        self.free = queue.Queue()
        for i in range(len(self.slots)):
            self.free.put((i, None))
        self.ready = queue.Queue()
        self.stop = threading.Event()
        self.sampler.set_epoch(self.epoch)
        self.rng = epoch_rng(self.seed, self.epoch)
        if hasattr(self.planner, 'reset_epoch'):
            self.planner.reset_epoch()
        self.thread = threading.Thread(target=self._produce, args=(list(self.sampler), self.stop, self.free, self.ready), daemon=True)
        self.thread.start()
        self.batch = None
        self._preload()

    def _produce(self, order, stop, free, ready):
        try:
            for b0 in range(0, len(order), self.batch_size):
                idx = order[b0:b0 + self.batch_size]
                if len(idx) < self.batch_size and self.drop_last:
                    break
                plans = [self.planner.plan(i, self.rng) for i in idx]
                slot, copied = free.get()
                if stop.is_set():
                    return
                if copied is not None:
                    copied.synchronize()  # the H2D copy that last read this slot
                lqn, gtn = self._lq_views[slot], self.slots[slot][1].numpy()
                list(self.pool.map(lambda a: self.planner.load(a[1], lqn[a[0]], gtn[a[0], 0]), enumerate(plans)))
                ready.put((slot, plans))
            ready.put(None)
        except BaseException as e:  # surfaces in next()
            ready.put(e)

    # ---- consumer
    def _upload_lq_crops(self, slot, n):
        return self.slots[slot][0][:n].to(self.device, non_blocking=True)

    def _upload_gt_windows(self, slot, n):
        """The slot's windows and table in one copy, then the LQ crops of the n samples: (n, t, p, p, 3) bytes, what an LQ tree holds there."""
        from . import ops
        scale, degradation = self.planner.lq_from_gt
        t, p = self.planner.num_frame, self.planner.lq_size
        dev = self.slots[slot][0].to(self.device, non_blocking=True)
        windows = dev[:self._n_win].view(self._win_shape)[:n * t]
        table = dev[self._n_win:].view(torch.int32).view(-1, LQ_WINDOW_RECORD_INTS)[:n * t]
        return ops.lq_crops_from_windows(windows, table, scale, degradation, table_host=self._tables[slot][:n * t]).view(n, t, p, p, 3)

    def _degrade(self, slot, plans, lq_d):
        """ONE ops.degrade launch on the LQ crop bytes (n, t, p, p, 3) of a batch: the t frames of a clip share its kernel and noise
        setting and differ in the frame index, i.e. in their noise fields."""
        from . import ops
        n, t, p = len(plans), self.planner.num_frame, self.planner.lq_size
        host = self._degrade_slots[slot]
        table, weights = host[:n * t * ops.DEGRADE_RECORD_INTS].view(n, t, ops.DEGRADE_RECORD_INTS), host[self._n_degrade_table:]
        offset = 0
        for i, pl in enumerate(plans):
            d = pl.degrade or {'kernel': None, 'noise': None, 'key': 0}
            ksize = 0 if d['kernel'] is None else d['kernel'].shape[0]
            if ksize:
                weights[offset:offset + ksize * ksize] = torch.from_numpy(d['kernel'].ravel())
            read, shot, gray = ops.degrade_noise(d['noise'])
            table[i] = torch.tensor([ops.degrade_record(ksize, offset, read, shot, gray, d['key'], f) for f in range(t)], dtype=torch.int32)
            offset += ksize * ksize
        dev = host.to(self.device, non_blocking=True)
        return ops.degrade(lq_d.view(n * t, p, p, 3), table=dev[:n * t * ops.DEGRADE_RECORD_INTS].view(n * t, ops.DEGRADE_RECORD_INTS),
                           weights=dev[self._n_degrade_table:], table_host=table.view(n * t, ops.DEGRADE_RECORD_INTS),
                           weights_host=weights).view(n, t, p, p, 3)

    def _preload(self):
        from . import ops
        item = self.ready.get()
        if isinstance(item, BaseException):
            raise item
        if item is None:
            self.batch = None
            return
        slot, plans = item
        lq, gt = self.slots[slot]
        n = len(plans)
        flags = bytes(p.flags for p in plans)
        with torch.cuda.stream(self.stream):
            lq_d, gt_d = self._lq_upload(slot, n), gt[:n].to(self.device, non_blocking=True)
            if self._degrade_slots is not None and any(pl.degrade for pl in plans):  # blur and noise come first, on the upright crop
                lq_d = self._degrade(slot, plans, lq_d)
            if self._mpeg_tables is not None and any(pl.mpeg_qscale for pl in plans):  # the video codec, on the upright crop clip
                table = self._mpeg_tables[slot][:n]
                table.copy_(torch.tensor([pl.mpeg_qscale for pl in plans], dtype=torch.int32))
                lq_d = ops.mpeg_roundtrip(lq_d, table.to(self.device, non_blocking=True), 0, self.planner.lq_mpeg[2])
            if self._jpeg_tables is not None:  # compression comes before flip / rotation: the block grid is anchored at the crop's corner
                t, p = self.planner.num_frame, self.planner.lq_size
                table = self._jpeg_tables[slot][:n * t]
                table.view(n, t).copy_(torch.tensor([pl.jpeg_quality for pl in plans], dtype=torch.int32)[:, None])
                lq_d = ops.jpeg_roundtrip(lq_d.view(n * t, p, p, 3), table.to(self.device, non_blocking=True), self.planner.lq_jpeg[2]).view(n, t, p, p, 3)
            copied = torch.cuda.Event()
            copied.record(self.stream)
            out = {'lq': ops.frames_u8_to_f32(lq_d, flags), 'gt': ops.frames_u8_to_f32(gt_d, flags)[:, 0], 'key': [p.key for p in plans]}
        self.free.put((slot, copied))
        self.batch = out

    def next(self):
        batch = self.batch
        if batch is None:
            return None
        cur = torch.cuda.current_stream(self.device)
        cur.wait_stream(self.stream)
        for v in batch.values():
            if torch.is_tensor(v):
                v.record_stream(cur)
        self._preload()
        return batch

    def reset(self, epoch=None):
        """Start the next epoch (CUDAPrefetcher.reset after train_sampler.set_epoch(epoch) in train.py)."""
        self.stop.set()
        self.free.put((0, None))  # wake a producer waiting for a slot
        self.thread.join()
        torch.cuda.synchronize(self.device)
        self.epoch = self.epoch + 1 if epoch is None else epoch
        self._start()

    def close(self):
        self.stop.set()
        self.free.put((0, None))
        self.thread.join()
        self.pool.shutdown()
