"""The numpy twin of the 3D LUT pass (include/mpcvr.h: mpcvr_lut3d_pass; arithmetic: csrc/vp_lut3d_core.h).  Written from the header's
text, not from the C++: integers only, one vectorised evaluation per call.  Everything the tests compare is bits."""
import itertools

import numpy as np

BGRA8, RGB10A2 = 0, 1
MAXCODE = {BGRA8: 255, RGB10A2: 1023}
ACC_BOUND = 1023 * 65535                     # the header's bound on a weighted channel sum: 67,042,305
PERMS = list(itertools.permutations(range(3)))


def codes(texels, fmt):
    """(R, G, B) of 32-bit texels as int64 arrays; the A / X bits are ignored"""
    t = np.asarray(texels, dtype=np.uint32).astype(np.int64)
    if fmt == RGB10A2:
        return t & 1023, (t >> 10) & 1023, (t >> 20) & 1023
    return (t >> 16) & 255, (t >> 8) & 255, t & 255


def pack(r, g, b, fmt):
    """texels from codes, the A / X bits all ones"""
    if fmt == RGB10A2:
        return (r | g << 10 | b << 20 | 0xc0000000).astype(np.uint32)
    return (b | g << 8 | r << 16 | 0xff000000).astype(np.uint32)


def split(c, n, maxin):
    """(i, f) of a code: t = c (n - 1), i = min(t / maxin, n - 2), f = t - i maxin"""
    t = c * (n - 1)
    i = np.minimum(t // maxin, n - 2)
    return i, t - i * maxin


def entries_from_float(rgb):
    """mpcvr_plan_lut3d_entries: (n^3, 3) floats -> (n^3, 4) uint16, rint(clamp(x, 0, 1) * 65535) in double, NaN -> 0, pad 0"""
    x = np.asarray(rgb, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    x = np.where(np.isnan(x), 0.0, x)
    x = np.minimum(np.maximum(x, 0.0), 1.0)
    out = np.zeros((x.shape[0], 4), dtype=np.uint16)
    out[:, :3] = np.rint(x * 65535.0).astype(np.uint16)
    return out


def identity_axis(n):
    """the header's identity table along one axis: E[i] = (2 i 65535 + (n - 1)) / (2 (n - 1))"""
    i = np.arange(n, dtype=np.int64)
    return (2 * i * 65535 + (n - 1)) // (2 * (n - 1))


def identity_entries(n, pad=0):
    """the identity table: node (r, g, b) at index (b n + g) n + r holds {E[r], E[g], E[b], pad}"""
    e = identity_axis(n)
    b, g, r = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    out = np.empty((n ** 3, 4), dtype=np.uint16)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = e[r.ravel()], e[g.ravel()], e[b.ravel()], pad
    return out


def apply(texels, entries, n, src_fmt, dst_fmt, perm=None, check=True):
    """The pass over an array of texels.  perm = None orders the channels by their fractions (a stable sort: ties in channel order); a
    permutation of (0, 1, 2) = (R, G, B) forces that order for every texel — admissible only where f[perm[0]] >= f[perm[1]] >= f[perm[2]],
    which the caller guarantees.  Returns uint32 texels of dst_fmt."""
    shape = np.shape(texels)
    maxin, maxout = MAXCODE[src_fmt], MAXCODE[dst_fmt]
    e = np.asarray(entries, dtype=np.uint16).reshape(-1, 4).astype(np.int64)
    assert e.shape[0] == n ** 3 and 2 <= n <= 65
    c = [x.ravel() for x in codes(texels, src_fmt)]
    i, f = zip(*(split(x, n, maxin) for x in c))
    f = np.stack(f)                                        # (3, N)
    if perm is None:
        order = np.argsort(-f, axis=0, kind="stable")
    else:
        order = np.repeat(np.array(perm, dtype=np.int64)[:, None], f.shape[1], axis=1)
    fs = np.take_along_axis(f, order, axis=0)
    assert (fs[0] >= fs[1]).all() and (fs[1] >= fs[2]).all(), "an order that is not admissible for these texels"
    stride = np.array([1, n, n * n], dtype=np.int64)
    v0 = (i[2] * n + i[1]) * n + i[0]
    v1 = v0 + stride[order[0]]
    v2 = v1 + stride[order[1]]
    v3 = v2 + stride[order[2]]
    assert np.array_equal(v3, ((i[2] + 1) * n + i[1] + 1) * n + i[0] + 1)
    w = (maxin - fs[0], fs[0] - fs[1], fs[1] - fs[2], fs[2])
    assert (w[0] + w[1] + w[2] + w[3] == maxin).all() and all((x >= 0).all() for x in w)
    out = []
    for k in range(3):
        acc = w[0] * e[v0, k] + w[1] * e[v1, k] + w[2] * e[v2, k] + w[3] * e[v3, k]
        if check:
            assert acc.size == 0 or acc.max() <= ACC_BOUND
        v = (acc + (maxin >> 1)) // maxin
        out.append((v * maxout + 32767) // 65535)
    return pack(out[0], out[1], out[2], dst_fmt).reshape(shape)


def place(buf, at, words, pitch):
    """`words` ((h, w) uint32) written into the byte array `buf` from offset `at` with rows `pitch` bytes apart"""
    h, w = words.shape
    for y in range(h):
        buf[at + y * pitch:at + y * pitch + 4 * w] = np.ascontiguousarray(words[y]).view(np.uint8)
    return buf
