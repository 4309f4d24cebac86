"""The NumPy restatement of inverse telecine's definition, on whole frames of a Y4M format.  Integers only; nothing
here is tuned to the kernels or to edvr_amd/telecine.py - it is written from the definition.  T9's fallback calls deint_ref.deinterlace.

q is the row parity of a frame's first field (0 'top', 1 'bottom'), L_i the luma plane of frame i; frames -1 and -2 are `prev` and
`prev2` where given.  A table row is (S_c, S_p, mic_c, mic_p, A, B, C); a match is 0 for c and 1 for p."""
import numpy as np

import deint_ref as D

NT, CT, MI, BLOCK, CYCLE = 2, 9, 80, 16, 5


def comb(W):
    """T2: k for every sample of an integer (R, C) plane; rows 0 and R - 1 are 0."""
    W = np.asarray(W).astype(np.int64)
    k = np.zeros_like(W)
    d1, d2 = W[1:-1] - W[:-2], W[1:-1] - W[2:]
    both = ((d1 > 0) & (d2 > 0)) | ((d1 < 0) & (d2 < 0))
    k[1:-1] = np.where(both, np.minimum(np.abs(d1), np.abs(d2)), 0)
    return k


def comb_sum(k, nt, sh):
    """T3"""
    return int(np.maximum(k - (nt << sh), 0).sum())


def comb_mic(k, ct, sh):
    """T4: the largest count of k > ct << sh in a 16 x 16 block anchored at (0, 0)."""
    hot = k > (ct << sh)
    R, C = hot.shape
    return max(int(hot[y:y + BLOCK, x:x + BLOCK].sum()) for y in range(0, R, BLOCK) for x in range(0, C, BLOCK))


def candidate_p(L, Lm1, q):
    """T1: W_p - the rows of parity q of L, the others from the frame before (W_c without one)."""
    if Lm1 is None:
        return L
    W = L.copy()
    W[1 - q::2] = Lm1[1 - q::2]
    return W


def field_match(frames, H, W, fmt='420', first='top', prev=None, prev2=None, nt=NT, ct=CT):
    """uint8 (n, framesize) -> int64 (n, 7): T1 - T5 for every frame.  prev / prev2: uint8 (framesize,) or None."""
    q = D.FIRST[first]
    sh = D.parse_format(fmt)[2] - 8
    luma = D.split(frames, H, W, fmt)[0]
    ctx = {-1: None if prev is None else D.split(np.asarray(prev).reshape(1, -1), H, W, fmt)[0][0],
           -2: None if prev2 is None else D.split(np.asarray(prev2).reshape(1, -1), H, W, fmt)[0][0]}
    L = lambda i: luma[i] if i >= 0 else ctx[i]
    table = np.zeros((luma.shape[0], 7), np.int64)
    for i in range(luma.shape[0]):
        kc, kp = comb(L(i)), comb(candidate_p(L(i), L(i - 1), q))
        a = b = c = 0
        if L(i - 1) is not None:
            a = int(np.abs(L(i)[q::2] - L(i - 1)[q::2]).sum())
            b = int(np.abs(L(i)[1 - q::2] - L(i - 1)[1 - q::2]).sum())
        if L(i - 2) is not None:
            c = int(np.abs(L(i)[1 - q::2] - L(i - 2)[1 - q::2]).sum())
        table[i] = (comb_sum(kc, nt, sh), comb_sum(kp, nt, sh), comb_mic(kc, ct, sh), comb_mic(kp, ct, sh), a, b, c)
    return table


def decide(table, mi=MI, decimate=True):
    """T6 - T8 on a whole table: (matches, combed, D, dropped)."""
    n = len(table)
    matches = [1 if int(r[1]) < int(r[0]) else 0 for r in table]
    combed = [int(r[3] if m else r[2]) > mi for r, m in zip(table, matches)]
    scores = []
    for i in range(n):
        if i == 0:
            scores.append(float('inf'))
            continue
        pair = (matches[i - 1], matches[i])
        x = {(0, 0): table[i][5], (1, 1): table[i - 1][5], (1, 0): table[i][6], (0, 1): 0}[pair]
        scores.append(int(table[i][4]) + int(x))
    dropped = []
    if decimate:
        for g in range(n // CYCLE):
            cyc = scores[CYCLE * g:CYCLE * g + CYCLE]
            dropped.append(CYCLE * g + min(range(CYCLE), key=lambda j: (cyc[j], j)))
    return matches, combed, scores, dropped


def weave(frames, H, W, fmt, first, i, match):
    """T9 without the fallback: one uint8 (framesize,) frame."""
    q = D.FIRST[first]
    planes = D.split(frames, H, W, fmt)
    out = []
    for p in planes:
        w = p[i].copy()
        if match:
            w[1 - q::2] = p[i - 1][1 - q::2]
        out.append(w[None])
    return D.join(out, fmt)[0]


def field_weave(frames, H, W, fmt, first, indices, matches, prev=None):
    """ops.field_weave restated: uint8 (k, framesize); frame -1 is `prev`."""
    frames = np.asarray(frames)
    both = frames if prev is None else np.concatenate([np.asarray(prev).reshape(1, -1), frames])
    off = 0 if prev is None else 1
    return np.stack([weave(both, H, W, fmt, first, i + off, m) for i, m in zip(indices, matches)])


def inverse_telecine(frames, H, W, fmt='420', first='top', decimate=True, nt=NT, ct=CT, mi=MI, info=None):
    """T1 - T9 on a whole clip: uint8 (n, framesize) -> uint8 (kept, framesize).  info: a dict that receives 'table', 'matches', 'combed',
    'scores' and 'dropped'."""
    frames = np.asarray(frames)
    n = frames.shape[0]
    table = field_match(frames, H, W, fmt, first, nt=nt, ct=ct)
    matches, combed, scores, dropped = decide(table, mi, decimate)
    out = []
    for i in range(n):
        if i in dropped:
            continue
        if combed[i]:
            out.append(D.deinterlace(frames[i:i + 1], H, W, fmt, first, 'frame', prev=frames[i - 1] if i else None,
                                     nxt=frames[i + 1] if i + 1 < n else None)[0])
        else:
            out.append(weave(frames, H, W, fmt, first, i, matches[i]))
    if info is not None:
        info.update(table=table, matches=matches, combed=combed, scores=scores, dropped=dropped)
    return np.stack(out) if out else np.zeros((0, frames.shape[1]), np.uint8)
