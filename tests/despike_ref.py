"""rmd_despike restated in numpy scalars (include/raymond_hip.h has the definition): plain loops over pixels and windows, the same brackets, bit copies
through view(np.uint64).  Also rmd_tile_error restated, for the tile the stage exists for.  No GPU, no library."""
import numpy as np

from tile_reduce_ref import A0, A1, A2, WB, WG, WR  # the luminance weights, and the binary64 product of each with itself


def count_image(width, height, rects, counts):
    """(n, rect index) per pixel: 0 and -1 where no rect lies."""
    n = np.zeros((height, width), dtype=np.uint32)
    idx = np.full((height, width), -1, dtype=np.int64)
    for j, ((l, t, w, h), c) in enumerate(zip(rects, counts)):
        n[t : t + h, l : l + w] = c
        idx[t : t + h, l : l + w] = j
    return n, idx


def luminance_planes(S, Q, n):
    """(valid, Y, V) per pixel; Y and V are NaN where the pixel is not valid."""
    H, W = n.shape
    valid = np.zeros((H, W), dtype=bool)
    Y = np.full((H, W), np.nan)
    V = np.full((H, W), np.nan)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                ni = int(n[y, x])
                if ni < 2 or not (np.isfinite(S[y, x]).all() and np.isfinite(Q[y, x]).all()):
                    continue
                nd = np.float64(ni)
                u, v = [], []
                for c in range(3):
                    s, q = np.float64(S[y, x, c]), np.float64(Q[y, x, c])
                    uc = s / nd
                    t = (q - s * uc) / (nd - np.float64(1.0))
                    if not t > 0.0:
                        t = np.float64(0.0)
                    u.append(uc), v.append(t / nd)
                valid[y, x] = True
                Y[y, x] = (WR * u[0] + WG * u[1]) + WB * u[2]
                V[y, x] = (A0 * v[0] + A1 * v[1]) + A2 * v[2]
    return valid, Y, V


def donor_of(valid, Y, x, y, radius, rank):
    """The donor's (x, y) for the valid pixel (x, y), or None with fewer than rank + 1 others: the others sorted by Y descending, ties by raster order of d."""
    H, W = Y.shape
    others = []
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            qx, qy = x + dx, y + dy
            if (dx or dy) and 0 <= qx < W and 0 <= qy < H and valid[qy, qx]:
                others.append((qx, qy))
    # a stable sort by -Y keeps the raster order among equal Y (and +0.0 == -0.0, as the comparison says)
    others.sort(key=lambda q: -float(Y[q[1], q[0]]))
    return others[rank] if len(others) > rank else None


class Plan:
    """What of a call does not depend on k, ratio and floor: the count and rect images, validity, Y, V and every valid pixel's donor."""

    def __init__(self, S, Q, rects, counts, radius, rank):
        self.S = np.ascontiguousarray(S, dtype=np.float64)
        self.Q = np.ascontiguousarray(Q, dtype=np.float64)
        self.rects = list(rects)
        H, W = self.S.shape[0], self.S.shape[1]
        self.n, self.idx = count_image(W, H, self.rects, counts)
        self.valid, self.Y, self.V = luminance_planes(self.S, self.Q, self.n)
        self.donor = {}
        for y in range(H):
            for x in range(W):
                if self.valid[y, x]:
                    d = donor_of(self.valid, self.Y, x, y, radius, rank)
                    if d is not None:
                        self.donor[(x, y)] = d

    def decide(self, k=6.0, ratio=2.0, floor=0.0):
        """(S', Q', replaced, spikes): the outputs, the per-rect counts (uint32) and the list of (x, y, donor x, donor y)."""
        S, Q, Y, V, n = self.S, self.Q, self.Y, self.V, self.n
        out_S, out_Q = S.copy(), Q.copy()
        oS, oQ, iS, iQ = (a.view(np.uint64) for a in (out_S, out_Q, S, Q))
        replaced = np.zeros(len(self.rects), dtype=np.uint32)
        spikes = []
        k, ratio, floor = np.float64(k), np.float64(ratio), np.float64(floor)
        k2 = k * k
        with np.errstate(all="ignore"):
            for (x, y), (qx, qy) in self.donor.items():
                e = (Y[y, x] - ratio * Y[qy, qx]) - floor
                if not (e > 0.0 and e * e > k2 * V[qy, qx]):
                    continue
                spikes.append((x, y, qx, qy))
                replaced[self.idx[y, x]] += 1
                n_p, n_q = int(n[y, x]), int(n[qy, qx])
                if n_p == n_q:
                    oS[y, x], oQ[y, x] = iS[qy, qx], iQ[qy, qx]
                else:
                    for c in range(3):
                        out_S[y, x, c] = (S[qy, qx, c] / np.float64(n_q)) * np.float64(n_p)
                        out_Q[y, x, c] = (Q[qy, qx, c] / np.float64(n_q)) * np.float64(n_p)
        return out_S, out_Q, replaced, spikes


def despike(S, Q, rects, counts, radius=2, rank=2, k=6.0, ratio=2.0, floor=0.0):
    """rmd_despike: (S', Q', replaced, spikes)."""
    return Plan(S, Q, rects, counts, radius, rank).decide(k, ratio, floor)


def tile_error(S, Q, sample_count, floor, rects):
    """rmd_tile_error restated: per rect the largest sqrt(v / n) / max(|m|, floor) over its pixels and channels, +inf with n < 2 or a non-finite sum."""
    out = np.zeros(len(rects))
    nd = np.float64(sample_count)
    with np.errstate(all="ignore"):
        for j, (l, t, w, h) in enumerate(rects):
            e = 0.0
            for y in range(t, t + h):
                for x in range(l, l + w):
                    if sample_count < 2 or not (np.isfinite(S[y, x]).all() and np.isfinite(Q[y, x]).all()):
                        e = np.inf
                        continue
                    for c in range(3):
                        m = S[y, x, c] / nd
                        v = (Q[y, x, c] - S[y, x, c] * m) / (nd - 1.0)
                        v = v if v > 0.0 else 0.0
                        e = max(e, float(np.sqrt(v / nd) / max(abs(m), floor)))
            out[j] = e
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
