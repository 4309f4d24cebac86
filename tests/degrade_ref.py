"""NumPy restatement of the blur and noise degradations of DESIGN 4.17 (what ops.degrade and ops.philox_words compute): Philox4x32-10 in
uint64 arithmetic, the integer blur over the reflect-extended frame, and the noise twice - in float64, which the tests compare against,
and in float32 operation by operation as the kernel performs it, which measures how far float32 can move a sample (the tests' delta)."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
ONE = 1 << 20


def philox4x32_10(counter, key):
    """counter: four uint32 arrays of one shape (or ints), key: two ints -> the four uint32 words, as Random123 defines them."""
    c = [np.asarray(v, np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [v.astype(np.uint32) for v in c]


def philox_words(key, ctr_t, H, W):
    """(H, W, 4) uint32: the words at counter (x, y, ctr_t, 0) and the 64-bit key `key`, low word first."""
    y, x = np.mgrid[0:H, 0:W]
    return np.stack(philox4x32_10((x, y, ctr_t, 0), (key & MASK, (key >> 32) & MASK)), -1)


def reflect(i, n):
    """The reflection that does not repeat the edge sample, of indices -(n - 1) .. 2 (n - 1)."""
    i = np.abs(np.asarray(i))
    return np.where(i >= n, 2 * (n - 1) - i, i)


def blur_acc(img, kernel):
    """acc (H, W, 3) int64 = sum of Q20 weight x sample over the reflect-extended frame; kernel None: img << 20."""
    img = img.astype(np.int64)
    if kernel is None:
        return img << 20
    H, W, _ = img.shape
    k = kernel.shape[0]
    r = k // 2
    assert kernel.shape == (k, k) and k % 2 == 1 and min(H, W) > r
    ext = img[reflect(np.arange(-r, H + r), H)][:, reflect(np.arange(-r, W + r), W)]
    acc = np.zeros_like(img)
    for a in range(k):
        for b in range(k):
            acc += int(kernel[a, b]) * ext[a:a + H, b:b + W]
    return acc


def _uniform_parts(words):
    return [(w >> np.uint32(8)).astype(np.float64) for w in np.moveaxis(words, -1, 0)]


def normals64(words, gray=False):
    """(H, W, 3) float64 standard normals of (H, W, 4) Philox words: Box-Muller on (r0, r1) -> z_R, z_G and on (r2, r3) -> z_B."""
    n0, n1, n2, n3 = _uniform_parts(words)
    rho1, phi1 = np.sqrt(-2 * np.log((n0 + 0.5) * 2.0 ** -24)), 2 * np.pi * n1 * 2.0 ** -24
    rho2, phi2 = np.sqrt(-2 * np.log((n2 + 0.5) * 2.0 ** -24)), 2 * np.pi * n3 * 2.0 ** -24
    z = np.stack([rho1 * np.cos(phi1), rho1 * np.sin(phi1), rho2 * np.cos(phi2)], -1)
    return np.repeat(z[..., :1], 3, -1) if gray else z


def normals32(words, gray=False):
    """The same in float32, each operation rounded on its own (u by one fused multiply-add, as the kernel forms it)."""
    f = np.float32
    n0, n1, n2, n3 = _uniform_parts(words)

    def polar(a, b):
        u = (a * 2.0 ** -24 + 2.0 ** -25).astype(f)  # exact in float64, rounded once
        rho = np.sqrt(f(-2) * np.log(u))
        phi = f(6.283185307179586) * (b.astype(f) * f(2.0 ** -24))
        return rho, phi
    (rho1, phi1), (rho2, phi2) = polar(n0, n1), polar(n2, n3)
    z = np.stack([rho1 * np.cos(phi1), rho1 * np.sin(phi1), rho2 * np.cos(phi2)], -1)
    assert z.dtype == f
    return np.repeat(z[..., :1], 3, -1) if gray else z


def noisy_t(acc, read, shot, gray, key, ctr_t, dtype=np.float64):
    """t = v + s z before rounding, (H, W, 3) of `dtype` (float64, or float32 operation by operation); read, shot as float32 values."""
    H, W, _ = acc.shape
    words = philox_words(key, ctr_t, H, W)
    v32 = acc.astype(np.float32) * np.float32(2.0 ** -20)  # float32(acc): round to nearest even, then an exact scaling
    if dtype == np.float32:
        f = np.float32
        s = np.sqrt(f(shot) * v32 + f(read) * f(read))
        t = v32 + s * normals32(words, gray)
        assert t.dtype == f
        return t
    v = v32.astype(np.float64)
    read, shot = float(np.float32(read)), float(np.float32(shot))
    return v + np.sqrt(shot * v + read * read) * normals64(words, gray)


def round_levels(t):
    return np.clip(np.floor(t + t.dtype.type(0.5)), 0, 255).astype(np.uint8)


def degrade(img, kernel=None, noise=None, key=0, ctr_t=0):
    """One image (H, W, 3) uint8 -> uint8, the float64 definition; noise = (read_sigma, shot, gray) or None."""
    acc = blur_acc(img, kernel)
    if noise is None or (float(np.float32(noise[0])) == 0 and float(np.float32(noise[1])) == 0):
        return ((acc + (1 << 19)) >> 20).astype(np.uint8)
    return round_levels(noisy_t(acc, noise[0], noise[1], noise[2], key, ctr_t))
