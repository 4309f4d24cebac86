"""The scene-cut definition restated in NumPy / plain Python for the tests, and the synthetic three-shot video.

Y8, SAD, scores and select_cuts below share no code with edvr_amd/shots.py or csrc/shots.hip."""
import numpy as np
import torch
import torch.nn.functional as F

SHOTS = (7, 9, 6)      # frames per shot of the synthetic video
CUTS = [7, 16]


def bytes_of(frames):
    """(n, H, W, 3) int64 bytes of uint8 (n, H, W, 3) or float32 (n, 3, H, W) frames (CPU tensors): tensor2img for floats - clamp,
    x 255 in float32, round half to even, NaN -> 0."""
    a = frames.cpu().numpy()
    if a.dtype == np.uint8:
        return a.astype(np.int64)
    assert a.dtype == np.float32
    a = np.where(np.isnan(a), np.float32(0), a)
    q = np.rint(np.clip(a, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.int64)
    return np.ascontiguousarray(q.transpose(0, 2, 3, 1))


def y8(frames):
    b = bytes_of(frames)
    return ((66 * b[..., 0] + 129 * b[..., 1] + 25 * b[..., 2] + 128) >> 8) + 16


def sad(frames, prev=None):
    """int64 (n,) CPU tensor: what ops.frame_sad(frames, prev) must return."""
    y = y8(frames)
    out = np.zeros(y.shape[0], dtype=np.int64)
    out[1:] = np.abs(y[1:] - y[:-1]).reshape(y.shape[0] - 1, -1).sum(1)
    if prev is not None:
        out[0] = np.abs(y[0] - y8(prev[None] if prev.dim() == 3 else prev)[0]).sum()
    return torch.from_numpy(out)


def scores(sads, pixels):
    """(mafd, score) float64 lists from the SAD list of a whole video."""
    mafd = [int(s) / pixels for s in sads]
    score = [0.0] + [min(mafd[i], abs(mafd[i] - mafd[i - 1])) for i in range(1, len(mafd))]
    if mafd:
        score[0] = min(mafd[0], abs(mafd[0] - 0.0))  # (mafd_0 = 0 for a video's first frame: 0)
    return mafd, score


def select_cuts(score, n, threshold=10.0, min_shot=2):
    cuts, start = [], 0
    for i in range(1, n):
        if score[i] >= threshold and i - start >= min_shot and n - i >= min_shot:
            cuts.append(i)
            start = i
    return cuts


def cuts_of(frames, threshold=10.0, min_shot=5):
    """The restatement end to end on a video (CPU tensor): (cuts, mafd, score)."""
    H, W = (frames.shape[1:3] if frames.dtype == torch.uint8 else frames.shape[2:4])
    mafd, score = scores(sad(frames).tolist(), H * W)
    return select_cuts(score, frames.shape[0], threshold, min_shot), mafd, score


def synthetic_shot(s, n, H, W, k=17):
    """Shot s: a smooth random texture (uniform noise, reflect-padded, box-filtered twice, stretched to [0, 1]) seen through a window
    that moves one pixel down and right per frame: float32 (n, 3, H, W)."""
    base = torch.rand(1, 3, H + n + k - 1, W + n + k - 1, generator=torch.Generator().manual_seed(100 + s))
    x = F.pad(base, (k // 2,) * 4, mode='reflect')
    x = F.avg_pool2d(F.avg_pool2d(x, k, stride=1), k, stride=1)
    x = (x - x.min()) / (x.max() - x.min())
    return torch.stack([x[0, :, t:t + H, t:t + W] for t in range(n)]).contiguous()


def synthetic_video(H, W, dtype=torch.float32):
    """Three shots of 7, 9 and 6 frames: float32 (22, 3, H, W) in [0, 1], or its tensor2img bytes as uint8 (22, H, W, 3)."""
    v = torch.cat([synthetic_shot(s, n, H, W) for s, n in enumerate(SHOTS)])
    if dtype == torch.uint8:
        return torch.from_numpy(bytes_of(v).astype(np.uint8))
    return v


def shot_bounds(cuts, n):
    b = [0] + list(cuts) + [n]
    return list(zip(b, b[1:]))
