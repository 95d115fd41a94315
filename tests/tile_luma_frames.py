"""The frames and rect lists tests/test_gpu_tile_luma.py sends to rmd_tile_luma_error; tests/test_tile_luma_host.py checks on the CPU that each class is
what it names.  Sums are made directly: S positive, Q = S^2 times a factor in [0.6, 1.5], which leaves a positive variance at every count >= 2."""
import numpy as np

W, H = 67, 45
FLOOR = 1e-3
NMAX = 2**32 - 1

# (rect, count): the smallest at which the lane striding, the combine and the addressing can go wrong
RECTS = [
    ((5, 7, 1, 1), 17),        # one pixel: lane 0 alone
    ((3, 2, 16, 16), 2),       # exactly 256: every lane one pixel
    ((20, 1, 17, 15), 3),      # 255: the last lane none
    ((1, 10, 32, 32), 17),     # the adaptive check's tile: four pixels a lane
    ((34, 3, 33, 31), NMAX),   # 1,023 pixels, ends at the frame's last column
    ((10, 20, 0, 5), 17),      # empty
    ((W, H, 0, 0), 3),         # empty, at the frame's far corner
    ((50, 30, 17, 15), 2),     # ends at the frame's last column and row
    ((8, 8, 20, 12), 3),       # two overlapping rects, at different counts
    ((18, 14, 20, 12), 17),
    ((40, 36, 9, 9), NMAX),    # one rect given twice
    ((40, 36, 9, 9), NMAX),
    ((0, 40, 6, 5), 1),        # a count of 1: every pixel invalid
    ((55, 0, 9, 7), 3),        # 63: one wave, its last lane none
    ((0, 30, 8, 8), 17),       # 64: exactly one wave, the other three add zeros
    ((60, 32, 5, 13), 2),      # 65: one lane of the second wave
]
BAD_PIXEL = (12, 20)  # (x, y) inside the 32 x 32 rect and no other rect of the list
BAD_RECT = 3

# the 300 x 300 frame: a row longer than a wave and a column longer than the workgroup
WIDE = 300
WIDE_RECTS = [((10, 5, 255, 1), 17), ((7, 3, 1, 257), 3), ((0, 0, 1, 1), 2)]


def rects_and_counts(pairs):
    return [r for r, _ in pairs], [c for _, c in pairs]


def random_positive(width=W, height=H, seed=1):
    rng = np.random.default_rng(seed)
    S = rng.uniform(0.05, 2.0, (height, width, 3)) * 16.0
    Q = S * S * rng.uniform(0.6, 1.5, (height, width, 3))
    return S, Q


def frames():
    """name -> (S, Q) on the W x H frame."""
    S, Q = random_positive()
    out = {"random": (S, Q)}
    out["tiny"] = (S * 2.0**-500, Q * 2.0**-1000)  # the radiance scaled by 2^-500: exact, the squares follow
    out["huge"] = (S * 2.0**500, Q * 2.0**1000)
    out["clamped"] = (S, S * S * 2.0**-40)  # Q < S^2 / n at every count up to 2^32 - 1: every variance clamps to 0
    out["negative"] = (-S, Q)
    nan_S = S.copy()
    nan_S[BAD_PIXEL[1], BAD_PIXEL[0], 1] = np.nan
    out["nan_in_S"] = (nan_S, Q)
    inf_Q = Q.copy()
    inf_Q[BAD_PIXEL[1], BAD_PIXEL[0], 2] = np.inf
    out["inf_in_Q"] = (S, inf_Q)
    return out


def permuted_tile(S, Q, rect, seed=5):
    """The frame with the pixels of `rect` permuted among themselves (S and Q together)."""
    l, t, w, h = rect
    order = np.random.default_rng(seed).permutation(w * h)
    S2, Q2 = S.copy(), Q.copy()
    S2[t : t + h, l : l + w] = S[t : t + h, l : l + w].reshape(-1, 3)[order].reshape(h, w, 3)
    Q2[t : t + h, l : l + w] = Q[t : t + h, l : l + w].reshape(-1, 3)[order].reshape(h, w, 3)
    return S2, Q2
