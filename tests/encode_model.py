"""The numpy model of the RGB -> NV12 / P010 pass (include/mpcvr.h: mpcvr_encode_pass), bit for bit: int64 throughout, the three chroma
sitings with edge replication, coefficients / offsets / shift as arguments (api.plan_encode returns them).  tests/test_encode.py closes it
through the oracle, tests/test_encode_gpu.py holds k_encode420 to it byte for byte."""
import numpy as np

CENTRE, LEFT, TOPLEFT = 0, 1, 2


def unpack_rgb(surface, src_fmt):
    """(h, w) uint32 texels -> (h, w, 3) int64 codes R, G, B.  src_fmt 0: B8G8R8A8 (B | G << 8 | R << 16 | A << 24); 1: R10G10B10A2
    (R | G << 10 | B << 20 | A << 30).  The A / X bits are dropped."""
    t = np.asarray(surface, dtype=np.uint32).astype(np.int64)
    if src_fmt == 0:
        return np.stack([(t >> 16) & 255, (t >> 8) & 255, t & 255], -1)
    return np.stack([t & 1023, (t >> 10) & 1023, (t >> 20) & 1023], -1)


def pack_rgb(rgb, src_fmt, alpha=0):
    rgb = np.asarray(rgb).astype(np.uint32)
    if src_fmt == 0:
        return (rgb[..., 2] | rgb[..., 1] << 8 | rgb[..., 0] << 16 | np.uint32(alpha & 255) << 24).astype(np.uint32)
    return (rgb[..., 0] | rgb[..., 1] << 10 | rgb[..., 2] << 20 | np.uint32(alpha & 3) << 30).astype(np.uint32)


def _taps(siting):
    """[(dy, dx, weight)] relative to texel (2j, 2i) of the block, and log2 of the weights' sum"""
    if siting == CENTRE:
        return [(0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 1)], 2
    h = [(-1, 1), (0, 2), (1, 1)]
    if siting == LEFT:
        return [(dy, dx, wx) for dy in (0, 1) for dx, wx in h], 3
    if siting == TOPLEFT:
        return [(dy, dx, wy * wx) for dy, wy in h for dx, wx in h], 4
    raise ValueError(siting)


def encode420(surface, src_fmt, out10, coef, off, shift, siting):
    """-> (Y (h, w), UV (h / 2, w)) as uint8 (out10 false: NV12) or uint16 holding code << 6 (P010)."""
    rgb = unpack_rgb(surface, src_fmt)
    h, w, _ = rgb.shape
    assert w >= 2 and h >= 2 and w % 2 == 0 and h % 2 == 0
    coef = np.asarray(coef, dtype=np.int64).reshape(3, 3)
    off = np.asarray(off, dtype=np.int64).reshape(3)
    S = int(shift)
    top = 1023 if out10 else 255
    y = np.clip((rgb @ coef[0] + off[0] + (1 << (S - 1))) >> S, 0, top)
    taps, logw = _taps(siting)
    W = 1 << logw
    ys, xs = np.arange(0, h, 2), np.arange(0, w, 2)
    sums = np.zeros((h // 2, w // 2, 3), dtype=np.int64)
    for dy, dx, wt in taps:
        rows = np.clip(ys + dy, 0, h - 1)
        cols = np.clip(xs + dx, 0, w - 1)
        sums += wt * rgb[rows[:, None], cols[None, :]]
    uv = np.empty((h // 2, w), dtype=np.int64)
    for k in (1, 2):
        uv[:, k - 1::2] = np.clip((sums @ coef[k] + W * off[k] + (W << (S - 1))) >> (S + logw), 0, top)
    if out10:
        return (y << 6).astype(np.uint16), (uv << 6).astype(np.uint16)
    return y.astype(np.uint8), uv.astype(np.uint8)


def accumulator_range(coef, off, shift, maxin, logw):
    """(most negative, largest) value an accumulator of the pass can hold: every channel's sum anywhere in [0, W * maxin], the rounding
    term included; over the luma row (W = 1) and the two chroma rows (W = 2^logw)."""
    coef = np.asarray(coef, dtype=np.int64).reshape(3, 3)
    off = np.asarray(off, dtype=np.int64).reshape(3)
    lo = hi = 0
    for k in range(3):
        W = 1 if k == 0 else 1 << logw
        base = W * int(off[k]) + (W << (shift - 1))
        pos = int(np.clip(coef[k], 0, None).sum()) * W * maxin
        neg = int(np.clip(coef[k], None, 0).sum()) * W * maxin
        lo, hi = min(lo, base + neg), max(hi, base + pos)
    return lo, hi
