"""Frames for the rmd_despike tests: the hand-made ones of tests/test_despike_host.py (noise-free, every outcome derivable by hand) and the random ones the
device is held to tests/despike_ref.py on.  No GPU, no library."""
import numpy as np

S2 = 1e-4  # the per-sample variance every hand-made pixel carries, so that V > 0


def sums_of(mean, n, s2=S2):
    """(S, Q) of pixels whose n samples have the (H, W) or (H, W, 3) mean `mean` and per-sample variance s2 (a number or an (H, W) array): S = n * mean,
    Q = S * S / n + (n - 1) * s2 — so that (Q - S * u) / (n - 1) comes back as s2 to rounding."""
    mean = np.asarray(mean, dtype=np.float64)
    if mean.ndim == 2:
        mean = np.repeat(mean[:, :, None], 3, axis=2)
    n = np.asarray(n, dtype=np.float64)
    if n.ndim == 2:
        n = n[:, :, None]
    s2 = np.asarray(s2, dtype=np.float64)
    if s2.ndim == 2:
        s2 = s2[:, :, None]
    S = mean * n
    Q = S * S / n + (n - 1.0) * s2
    return np.ascontiguousarray(S), np.array(np.broadcast_to(Q, S.shape))  # (a copy: the caller writes into both)


def flat(width, height, value=1.0, n=16):
    """A constant frame under one rect; the per-sample variance differs from pixel to pixel (Y does not read it), so every pixel's Q has bits of its own."""
    s2 = S2 * (1.0 + 1e-3 * np.arange(width * height, dtype=np.float64).reshape(height, width))
    S, Q = sums_of(np.full((height, width), value), n, s2)
    return S, Q, [(0, 0, width, height)], [n]


def plant(S, Q, x, y, value, n=16):
    """Pixel (x, y) becomes a noise-free pixel of mean `value`."""
    s, q = sums_of(np.full((1, 1), value), n)
    S[y, x], Q[y, x] = s[0, 0], q[0, 0]


def layout(width, height):
    """The rects and counts of a random frame: four rects at counts 2, 5, 16 and 16 (the quadrants of the covered part), a count-1 rect (a strip under them,
    from 3 rows on) and an uncovered strip on the right (from 3 columns on).  Rects without pixels stay in the list: they cover nothing."""
    strip = max(1, width // 8) if width >= 3 else 0
    low = max(1, height // 8) if height >= 3 else 0
    cw, ch = width - strip, height - low
    mx, my = cw // 2, ch // 2
    rects = [(0, 0, mx, my), (mx, 0, cw - mx, my), (0, my, mx, ch - my), (mx, my, cw - mx, ch - my), (0, ch, cw, low)]
    return rects, [2, 5, 16, 16, 1]


def random_frame(width, height, seed):
    """(S, Q, rects, counts): a smooth base with a little noise, exact-tie plateaus, planted spikes, pairs and one-pixel lines, a block of negative sums, and NaN
    and inf sums.  The largest planted luminance stays far below 1e6."""
    rng = np.random.default_rng(seed)
    rects, counts = layout(width, height)
    n = np.zeros((height, width))
    for (l, t, w, h), c in zip(rects, counts):
        n[t : t + h, l : l + w] = c
    n_safe = np.maximum(n, 1.0)
    yy, xx = np.mgrid[0:height, 0:width]
    base = 0.75 + 0.25 * np.sin(0.21 * xx) + 0.125 * np.cos(0.33 * yy)
    mean = base[:, :, None] * np.array([1.0, 0.75, 0.5]) * (1.0 + 0.02 * rng.standard_normal((height, width, 3)))
    for _ in range(max(1, width * height // 150)):  # plateaus: one exact value over a small block (exact ties inside one rect)
        x, y = int(rng.integers(0, width)), int(rng.integers(0, height))
        mean[y : y + int(rng.integers(1, 6)), x : x + int(rng.integers(1, 6))] = rng.integers(1, 9) / 8.0
    s2 = (0.05 + 0.05 * rng.random((height, width, 1))) ** 2
    S = mean * n_safe[:, :, None]
    Q = S * S / n_safe[:, :, None] + np.maximum(n_safe[:, :, None] - 1.0, 0.0) * s2

    def firefly(x, y):  # one sample of 50 times the pixel's mean, times its count, on top
        b = 50.0 * np.abs(mean[y, x]) * n_safe[y, x] + 1.0
        S[y, x] += b
        Q[y, x] += b * b

    for _ in range(max(1, width * height // 60)):
        x, y = int(rng.integers(0, width)), int(rng.integers(0, height))
        kind = int(rng.integers(0, 4))
        if kind <= 1:
            firefly(x, y)
        elif kind == 2:  # a pair
            firefly(x, y)
            firefly(min(x + 1, width - 1), y)
        else:  # a one-pixel-wide line, down
            for k in range(int(rng.integers(3, 9))):
                if y + k < height:
                    firefly(x, y + k)
    if width >= 8 and height >= 8:  # a block of negative sums, a brighter (less negative) pixel and a darker one inside
        x, y = width // 3, height // 3
        S[y : y + 5, x : x + 5] = -np.abs(S[y : y + 5, x : x + 5])
        S[y + 2, x + 2] *= 0.5
        S[y + 3, x + 1] *= 1.5
    flatS, flatQ = S.reshape(-1), Q.reshape(-1)
    for _ in range(max(1, width * height // 200)):
        flatS[int(rng.integers(0, flatS.size))] = np.nan
        flatQ[int(rng.integers(0, flatQ.size))] = np.inf
        flatS[int(rng.integers(0, flatS.size))] = -np.inf
    if width * height >= 4:
        flatQ[0] = np.float64(np.uint64(0x7FF8000000000ABC).view(np.float64))  # a NaN with a payload: a bit copy keeps it
    return np.ascontiguousarray(S), np.ascontiguousarray(Q), rects, counts
