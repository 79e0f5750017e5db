"""The numpy twin of the sharpen pass (extension; the definition is the text of include/mpcvr.h under mpcvr_sharpen_pass): every integer of
the text written out again, independently of csrc/vp_sharpen_core.h.  The blur is the 2-D sum of the text, tap by tap (the kernel sums
separably); everything in int64, with the bounds of the text asserted on the way."""
from math import comb

import numpy as np

from tests.deband_model import BGRA8, MAXCODE, RGB10A2, codes, hash32, pack, place  # noqa: F401  (re-exported for the tests)

RGB, LUMA = 0, 1
BRANCHES = ("cored", "sharpened", "at_lo", "at_hi")


def shifted(f, dx, dy):
    """f(..., y + dy, x + dx) with both coordinates clamped to the surface"""
    h, w = f.shape[-2:]
    yy = np.clip(np.arange(h) + dy, 0, h - 1)
    xx = np.clip(np.arange(w) + dx, 0, w - 1)
    return f[..., yy[:, None], xx[None, :]]


def apply(words, src_fmt, dst_fmt, radius, amount, threshold, overshoot, mode, dither, seed, counts=None):
    """the pass over (h, w) uint32 texels -> (h, w) uint32 texels.  `counts`: a dict that receives how many channels took each branch
    (BRANCHES: cored to zero, sharpened and unlimited, stopped by the limiter at lo, stopped at hi)"""
    h, w = words.shape
    maxin, maxout = MAXCODE[src_fmt], MAXCODE[dst_fmt]
    r = radius
    S = 16 ** r
    b = [comb(2 * r, j + r) for j in range(-r, r + 1)]
    assert sum(b) == 4 ** r
    c = codes(words, src_fmt)                                                  # (3, h, w)
    if mode == LUMA:
        f = ((54 * c[0] + 183 * c[1] + 19 * c[2] + 128) >> 8)[None]            # (1, h, w): one field for the texel
        assert f.min() >= 0 and f.max() <= maxin
    else:
        f = c
    blur = np.zeros_like(f)
    for j in range(-r, r + 1):
        for i in range(-r, r + 1):
            blur += b[j + r] * b[i + r] * shifted(f, i, j)
    assert blur.max() <= S * maxin
    d = S * f - blur
    assert np.abs(d).max() <= S * maxin <= 4190208
    T = threshold * (S // 4)
    e = d - np.clip(d, -T, T)                                                  # (1 | 3, h, w), broadcasts over the channels in mode 1
    assert np.abs(amount * e).max() <= 1072693248
    v = 64 * S * c + amount * e
    assert np.abs(v).max() < 2 ** 31
    mn, mx = c.copy(), c.copy()
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            n = shifted(c, i, j)
            mn, mx = np.minimum(mn, n), np.maximum(mx, n)
    lo, hi = np.maximum(mn - overshoot, 0), np.minimum(mx + overshoot, maxin)
    if counts is not None:
        cored = np.broadcast_to(e == 0, v.shape)
        counts.update(cored=int(cored.sum()), at_lo=int((v < 64 * S * lo).sum()), at_hi=int((v > 64 * S * hi).sum()))
        counts["sharpened"] = v.size - counts["cored"] - counts["at_lo"] - counts["at_hi"]
        assert not (cored & ((v < 64 * S * lo) | (v > 64 * S * hi))).any()      # a cored channel is its own code, inside lo .. hi
    v = np.minimum(np.maximum(v, 64 * S * lo), 64 * S * hi)
    assert v.min() >= 0
    q = (v + 8 * S) >> (4 * r + 4)
    assert q.min() >= 0 and q.max() <= 4 * maxin
    den = 4 * maxin
    y, x = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    dd = ((hash32(x, y, 0, seed) >> 8) * den) >> 24 if dither else den // 2
    out = (q * maxout + dd) // den
    assert out.max() <= maxout and out.min() >= 0
    return pack(out, dst_fmt)


def edge_row(n=48):
    """the test row of the header: 10-bit codes stepping 100 -> 900, blurred by the 9-tap binomial (C(8, j), sum 256, floor division)"""
    row = np.where(np.arange(n) >= n // 2, 900, 100).astype(np.int64)
    idx = np.arange(n)
    return sum(comb(8, j + 4) * row[np.clip(idx + j, 0, n - 1)] for j in range(-4, 5)) // 256


def width_10_90(row):
    """the count of texels strictly between 180 and 820"""
    return int(((row > 180) & (row < 820)).sum())
