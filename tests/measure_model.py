"""The numpy model of the measure extension (include/mpcvr.h: mpcvr_measure_pass, mpcvr_light_level_from_histogram,
mpcvr_histogram_percentile): the histogram of max(R, G, B) over a rectangle of 32-bit RGB texels, and what a host derives from it.  Integers
throughout, so the kernel and the host functions are held to it word for word; the nits are evaluated in np.longdouble, the tests'
expectation for the library's double."""
import numpy as np

BGRA8, RGB10A2 = 0, 1
BINS = 1024


def maxin(src_fmt):
    return 1023 if src_fmt == RGB10A2 else 255


def max_rgb(words, src_fmt):
    """max of the three code fields of uint32 texels; the A / X bits (the top byte, or the top two bits) are ignored"""
    t = np.asarray(words, dtype=np.uint32)
    if src_fmt == RGB10A2:
        fields = (t & 0x3ff, (t >> 10) & 0x3ff, (t >> 20) & 0x3ff)
    else:
        fields = (t & 0xff, (t >> 8) & 0xff, (t >> 16) & 0xff)
    return np.maximum(np.maximum(fields[0], fields[1]), fields[2])


def hist(surface_words, src_fmt, rect=None):
    """surface_words: (h, w) uint32; rect = (left, top, right, bottom) or None for the whole surface -> 1024 int64 counts"""
    s = np.asarray(surface_words, dtype=np.uint32)
    l, t, r, b = rect if rect is not None else (0, 0, s.shape[1], s.shape[0])
    return np.bincount(max_rgb(s[t:b, l:r], src_fmt).reshape(-1).astype(np.int64), minlength=BINS)


def pq_nits(codes, src_fmt, dtype=np.longdouble):
    """L(c) = 10000 * EOTF_ST2084(c / maxin), the constants of st2084.hlsl (all exact in binary)"""
    one = dtype(1)
    m1 = dtype(2610) / (dtype(4096) * dtype(4))
    m2 = dtype(2523) / dtype(4096) * dtype(128)
    c1 = dtype(3424) / dtype(4096)
    c2 = dtype(2413) / dtype(4096) * dtype(32)
    c3 = dtype(2392) / dtype(4096) * dtype(32)
    v = np.power(np.asarray(codes, dtype=dtype) / dtype(maxin(src_fmt)), one / m2)
    return dtype(10000) * np.power(np.maximum(v - c1, dtype(0)) / (c2 - c3 * v), one / m1)


def light_level(h, src_fmt, dtype=np.longdouble):
    """dict(pixels, min_code, max_code, max_nits, avg_nits) of a histogram; the sum ascends in c"""
    h = np.asarray(h).astype(np.int64)
    pixels = int(h.sum())
    if not pixels:
        return dict(pixels=0, min_code=-1, max_code=-1, max_nits=0.0, avg_nits=0.0)
    nz = np.nonzero(h)[0]
    L = pq_nits(np.arange(BINS), src_fmt, dtype) if src_fmt == RGB10A2 else np.concatenate([pq_nits(np.arange(256), src_fmt, dtype), np.zeros(BINS - 256, dtype)])
    total = dtype(0)
    for c in nz:
        total += dtype(int(h[c])) * L[c]
    return dict(pixels=pixels, min_code=int(nz[0]), max_code=int(nz[-1]), max_nits=L[nz[-1]], avg_nits=total / dtype(pixels))


def percentile(h, ppm):
    """the smallest code c with sum_{k <= c} h[k] >= ceil(ppm * pixels / 10^6), in Python integers; None for an empty histogram"""
    h = [int(v) for v in np.asarray(h)]
    pixels = sum(h)
    if not pixels:
        return None
    need = -(-(int(ppm) * pixels) // 1000000)
    run = 0
    for c, v in enumerate(h):
        run += v
        if run >= need:
            return c
    raise AssertionError("unreachable: the cumulative count ends at pixels >= need")
