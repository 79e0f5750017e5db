"""The numpy twin of the deband pass (extension; the definition is the text of include/mpcvr.h under mpcvr_deband_pass): every integer of
the text written out again, independently of csrc/vp_deband_core.h.  Hash and offsets in uint32 / int64, the channels in int64."""
import numpy as np

BGRA8, RGB10A2 = 0, 1
MAXCODE = {BGRA8: 255, RGB10A2: 1023}
M32 = 0xffffffff


def codes(words, fmt):
    """(3, h, w) int64: the R, G, B codes of (h, w) uint32 texels; the A / X bits are dropped"""
    w = words.astype(np.int64)
    if fmt == RGB10A2:
        return np.stack([w & 1023, (w >> 10) & 1023, (w >> 20) & 1023])
    return np.stack([(w >> 16) & 255, (w >> 8) & 255, w & 255])


def pack(c, fmt):
    """(h, w) uint32 texels of (3, h, w) codes, the A / X bits all ones"""
    r, g, b = (c[k].astype(np.int64) for k in range(3))
    if fmt == RGB10A2:
        return (r | g << 10 | b << 20 | 0xc0000000).astype(np.uint32)
    return (b | g << 8 | r << 16 | 0xff000000).astype(np.uint32)


def hash32(x, y, k, seed):
    """H(x, y, k, seed) of the header over int64 arrays x, y >= 0 -> int64 in 0 .. 2^32 - 1.  Computed in uint64 (a product of two 32-bit
    numbers fits) and cut to 32 bits after every operation."""
    m = np.uint64(M32)
    const = np.uint64((k * 0x85EBCA77 + (seed & M32) * 0xC2B2AE3D) & M32)
    h = (x.astype(np.uint64) + y.astype(np.uint64) * np.uint64(0x9E3779B1) + const) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7feb352d)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846ca68b)) & m
    h ^= h >> np.uint64(16)
    return h.astype(np.int64)


def apply(words, src_fmt, dst_fmt, rng, iterations, threshold, dither, seed):
    """the pass over (h, w) uint32 texels -> (h, w) uint32 texels"""
    h, w = words.shape
    maxin, maxout = MAXCODE[src_fmt], MAXCODE[dst_fmt]
    c = codes(words, src_fmt)
    y, x = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    cur = 4 * c
    for k in range(1, iterations + 1):
        r = rng * k
        hh = hash32(x, y, k, seed)
        dx = (((hh & 0xffff) * (2 * r + 1)) >> 16) - r
        dy = (((hh >> 16) * (2 * r + 1)) >> 16) - r
        s = np.zeros_like(cur)
        for ox, oy in ((dx, dy), (-dy, dx), (-dx, -dy), (dy, -dx)):
            s += c[:, np.clip(y + oy, 0, h - 1), np.clip(x + ox, 0, w - 1)]
        cur = np.where(np.abs(s - cur) * k <= threshold, s, cur)
    den = 4 * maxin
    d = ((hash32(x, y, 0, seed) >> 8) * den) >> 24 if dither else den // 2
    out = (cur * maxout + d) // den
    assert out.max() <= maxout and out.min() >= 0
    return pack(out, dst_fmt)


def place(buf, at, words, pitch):
    """write (h, w) uint32 texels into the uint8 buffer `buf` from byte `at` at `pitch` bytes per row; returns buf"""
    h, w = words.shape
    b = words.view(np.uint8).reshape(h, 4 * w)
    for i in range(h):
        buf[at + i * pitch: at + i * pitch + 4 * w] = b[i]
    return buf
