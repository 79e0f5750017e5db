"""Which BITS of a media sample are a pixel, and samples that set the others (host only, numpy only).

videorenderer_amd.synth draws legal-range codes with every other bit at one constant.  fields() restates, per format, where each component's
bits lie in a sample laid out by synth.make_frame (the reference's layouts: Helper.cpp:295-359 for the plane walk — tests/sample_layouts.py —
and the copy / sampling code named below), and sorts them into classes:

    code    bits the reference turns into a pixel
    low     the six bits under a 10-bit code of P010, P210 and Y210: the texture is R16_UNORM / R16G16B16A16_UNORM (Helper.cpp:305-308,
            319-320) and is sampled whole, so the reference READS them
    high    bits 10..15 of the LSB-aligned 10-bit formats (YUV420P10, YUV422P10, YUV444P10, GBRP10, Y10): CopyPlane10to16
            (Helper.cpp:789-803) stores src16[i] << 6 into a uint16_t, they fall off the top
    alpha   the A component of AYUV, Y410, Y416, ARGB32 (and XRGB32's X byte), BGRA64, b64a: sampled into .a and never used (Shaders.cpp:186-193 swizzle the three
            colour components; the convert shader writes alpha 1)
    pad     the two pad bits of r210's big-endian dword (CopyFrameR210, Helper.cpp:770-787 masks three 10-bit
            fields), bits 30..31 of every v210 dword and the v210 fields past the width in a row's last six-pixel group (CopyFrameV210,
            Helper.cpp:685-768 masks 0x3ff per field; the Y210 texture is width / 2 texels wide, clamp addressing never reaches the rest)

Bytes between a row's pixel bytes and the pitch are in no class (tests/sample_layouts.py::pixel_mask has them).
"""
from collections import namedtuple

import numpy as np

from tests.sample_layouts import frame_bytes, plane_walk
from videorenderer_amd import synth

CLASSES = ("code", "low", "high", "alpha", "pad")
IGNORED = ("high", "alpha", "pad")
SEEDS = (0x51A5, 0xB175)            # the two draws of with_ignored_bits every test uses
LSB10 = (20, 22, 24, 27, 38)        # raw 0..1023 in a 16-bit word
MSB10 = (2, 6, 8)                   # 10 bits in the word's MSBs
LSB10_EXTRA = (1024, 1025, 0xFC00, 0xFFFF)      # corner_frame: words that wrap under << 6 (1023 is the field's max already)

# comp: 'Y', 'U', 'V' (R, G, B stand in as synth has them), 'A', or 'X' for bits no component owns; idx: indices of the container words in
# the buffer viewed as `dtype` (little- or big-endian uint8/16/32), shape (rows, cols); shift: the field's lowest bit (scalar or per column)
Field = namedtuple("Field", "comp cls dtype idx shift bits")


def _grid(off, rows, pitch, col_bytes, wb):
    r = np.arange(rows, dtype=np.int64)[:, None]
    b = off + r * pitch + np.asarray(col_bytes, dtype=np.int64)[None, :]
    assert not (b % wb).any()
    return b // wb


def _word_fields(comp, cformat, dtype, idx):
    """a component stored one to a word: 8 / 16 bits whole, MSB-aligned 10 bits over `low`, LSB-aligned 10 bits under `high`"""
    if np.dtype(dtype).itemsize == 1:
        return [Field(comp, "code", dtype, idx, 0, 8)]
    if cformat in MSB10:
        return [Field(comp, "code", dtype, idx, 6, 10), Field(comp, "low", dtype, idx, 0, 6)]
    if cformat in LSB10:
        return [Field(comp, "code", dtype, idx, 0, 10), Field(comp, "high", dtype, idx, 10, 6)]
    return [Field(comp, "code", dtype, idx, 0, 16)]


# v210 (SMPTE): six pixels in four dwords of three 10-bit fields — (dword, shift) of Y0..Y5, Cb0..2, Cr0..2
V210_Y = ((0, 10), (1, 0), (1, 20), (2, 10), (3, 0), (3, 20))
V210_U = ((0, 0), (1, 10), (2, 20))
V210_V = ((0, 20), (2, 0), (3, 10))


def fields(cformat, w, h, pitch=None):
    """every bit of the pixel bytes of a sample at luma pitch `pitch` (default: synth's), as Fields"""
    pitch = synth.default_pitch(cformat, w) if pitch is None else pitch
    walk = plane_walk(cformat, w, h, pitch)
    out = []
    if cformat in synth.FORMATS:
        planes, nb, dw, dh, bits, msb, v_first = synth.FORMATS[cformat]
        dt = "<u1" if nb == 1 else "<u2"
        cw = w // dw
        off, rows, pp, _ = walk[0]
        out += _word_fields("Y", cformat, dt, _grid(off, rows, pp, np.arange(w) * nb, nb))
        if planes == 2:
            off, rows, pp, _ = walk[1]
            out += _word_fields("U", cformat, dt, _grid(off, rows, pp, np.arange(cw) * 2 * nb, nb))
            out += _word_fields("V", cformat, dt, _grid(off, rows, pp, (np.arange(cw) * 2 + 1) * nb, nb))
        else:
            for comp, (off, rows, pp, _) in zip("VU" if v_first else "UV", walk[1:]):
                out += _word_fields(comp, cformat, dt, _grid(off, rows, pp, np.arange(cw) * nb, nb))
        return out
    kind, nb = synth.PACKED[cformat][:2]
    off, rows, pp, _ = walk[0]
    x, j = np.arange(w), np.arange(w // 2)
    word = lambda comp, dt, col_bytes: _word_fields(comp, cformat, dt, _grid(off, rows, pp, col_bytes, np.dtype(dt).itemsize))
    whole = lambda comp, cls, dt, col_bytes: [Field(comp, cls, dt, _grid(off, rows, pp, col_bytes, np.dtype(dt).itemsize), 0, 8 * np.dtype(dt).itemsize)]
    if kind in ("yuy2", "uyvy", "y210"):
        dt = "<u1" if nb == 1 else "<u2"
        iy, iu, iv = (1, 0, 2) if kind == "uyvy" else (0, 1, 3)
        out += word("Y", dt, (2 * x + iy) * nb) + word("U", dt, (4 * j + iu) * nb) + word("V", dt, (4 * j + iv) * nb)
    elif kind == "v210":
        groups = (w + 5) // 6
        d = _grid(off, rows, pp, np.arange(groups * 4) * 4, 4)                     # every dword of the rows' groups
        out.append(Field("X", "pad", "<u4", d, 30, 2))
        for comp, table, n in (("Y", V210_Y, w), ("U", V210_U, w // 2), ("V", V210_V, w // 2)):
            k = np.arange(groups * len(table))
            dw_i = np.array([table[i % len(table)][0] for i in k]) + 4 * (k // len(table))
            sh = np.array([table[i % len(table)][1] for i in k])
            out.append(Field(comp, "code", "<u4", d[:, dw_i[:n]], sh[:n], 10))
            if n < k.size:
                out.append(Field("X", "pad", "<u4", d[:, dw_i[n:]], sh[n:], 10))
    elif kind == "ayuv":
        out += whole("V", "code", "<u1", 4 * x) + whole("U", "code", "<u1", 4 * x + 1) + whole("Y", "code", "<u1", 4 * x + 2) + whole("A", "alpha", "<u1", 4 * x + 3)
    elif kind == "y410":
        d = _grid(off, rows, pp, 4 * x, 4)
        out += [Field("U", "code", "<u4", d, 0, 10), Field("Y", "code", "<u4", d, 10, 10), Field("V", "code", "<u4", d, 20, 10), Field("A", "alpha", "<u4", d, 30, 2)]
    elif kind == "y416":
        out += whole("U", "code", "<u2", 8 * x) + whole("Y", "code", "<u2", 8 * x + 2) + whole("V", "code", "<u2", 8 * x + 4) + whole("A", "alpha", "<u2", 8 * x + 6)
    elif kind == "gbrp":
        dt = "<u1" if nb == 1 else "<u2"
        for comp, (off, rows, pp, _) in zip("YUV", walk):
            out += _word_fields(comp, cformat, dt, _grid(off, rows, pp, x * nb, nb))
    elif kind == "gray":
        dt = "<u1" if nb == 1 else "<u2"
        out += word("Y", dt, x * nb)
    elif kind == "rgb24":
        out += whole("V", "code", "<u1", 3 * x) + whole("U", "code", "<u1", 3 * x + 1) + whole("Y", "code", "<u1", 3 * x + 2)
    elif kind == "rgb32":
        out += whole("V", "code", "<u1", 4 * x) + whole("U", "code", "<u1", 4 * x + 1) + whole("Y", "code", "<u1", 4 * x + 2)
        out += whole("A", "alpha", "<u1", 4 * x + 3)        # (XRGB32's X byte as well: synth sets it like ARGB32's A)
    elif kind == "r210":        # big-endian dword: 2 pad bits, R, G, B
        d = _grid(off, rows, pp, 4 * x, 4)
        out += [Field("Y", "code", ">u4", d, 20, 10), Field("U", "code", ">u4", d, 10, 10), Field("V", "code", ">u4", d, 0, 10), Field("X", "pad", ">u4", d, 30, 2)]
    elif kind in ("rgb48", "bgr48"):
        a, c = ("Y", "V") if kind == "rgb48" else ("V", "Y")
        out += whole(a, "code", "<u2", 6 * x) + whole("U", "code", "<u2", 6 * x + 2) + whole(c, "code", "<u2", 6 * x + 4)
    elif kind == "bgra64":
        out += whole("V", "code", "<u2", 8 * x) + whole("U", "code", "<u2", 8 * x + 2) + whole("Y", "code", "<u2", 8 * x + 4) + whole("A", "alpha", "<u2", 8 * x + 6)
    elif kind == "b64a":        # big-endian words A, R, G, B
        out += whole("A", "alpha", ">u2", 8 * x) + whole("Y", "code", ">u2", 8 * x + 2) + whole("U", "code", ">u2", 8 * x + 4) + whole("V", "code", ">u2", 8 * x + 6)
    else:
        raise KeyError(kind)
    return out


def _bits_of(f):
    return (np.uint64((1 << f.bits) - 1) << np.asarray(f.shift, dtype=np.uint64)).astype(f.dtype)


def field_map(cformat, w, h, pitch=None):
    """{class: uint8 array of the sample's size, a bit set where the sample's bit belongs to the class}"""
    pitch = synth.default_pitch(cformat, w) if pitch is None else pitch
    out = {c: np.zeros(frame_bytes(cformat, w, h, pitch), dtype=np.uint8) for c in CLASSES}
    for f in fields(cformat, w, h, pitch):
        v = out[f.cls].view(f.dtype)
        np.bitwise_or.at(v, f.idx, np.broadcast_to(_bits_of(f), f.idx.shape))        # (v210: a field's columns share dwords)
    return out


def get_field(buf, f):
    v = np.ascontiguousarray(buf).view(np.uint8).ravel().view(f.dtype)
    return ((v[f.idx].astype(np.uint64) >> np.asarray(f.shift, dtype=np.uint64)) & np.uint64((1 << f.bits) - 1)).astype(np.uint32)


def put_field(buf, f, values):
    """in place: the field's bits of every container word <- values (rows x cols)"""
    v = buf.view(f.dtype)
    m = _bits_of(f)
    new = (np.asarray(values, dtype=np.uint64) << np.asarray(f.shift, dtype=np.uint64)).astype(f.dtype)
    np.bitwise_and.at(v, f.idx, np.broadcast_to(~m, f.idx.shape))                     # (v210: a field's columns share dwords)
    np.bitwise_or.at(v, f.idx, np.broadcast_to(new & m, f.idx.shape))


def random_bytes(n, seed):
    return synth.splitmix64((n + 7) // 8, synth.SEED_BASE ^ (seed * 0x9E37)).view(np.uint8)[:n].copy()


def _randomise(sample, cformat, w, h, classes, seed, pitch=None):
    sample = np.ascontiguousarray(sample).view(np.uint8).ravel()
    fm = field_map(cformat, w, h, pitch)
    mask = np.zeros_like(sample)
    for c in classes:
        mask |= fm[c]
    return (sample & ~mask) | (random_bytes(sample.size, seed) & mask)


def with_ignored_bits(sample, cformat, w, h, seed, pitch=None):
    """the same picture: every `high`, `alpha` and `pad` bit drawn from SplitMix64"""
    return _randomise(sample, cformat, w, h, IGNORED, seed, pitch)


def with_low_bits(sample, cformat, w, h, seed, pitch=None):
    """ANOTHER picture on P010 / P210 / Y210 (the reference reads the bits under the code); the same sample everywhere else"""
    return _randomise(sample, cformat, w, h, ("low",), seed, pitch)


def container_noise(cformat, w, h, seed):
    """(sample, pitch) at synth's pitch: every bit of every class random — the whole code space of the container (8 / 16-bit codes 0 .. max,
    10-bit fields 0 .. 1023, LSB-aligned 10-bit words 0 .. 65535), alpha and pad fields included; pitch padding zero"""
    pitch = synth.default_pitch(cformat, w)
    zero = np.zeros(frame_bytes(cformat, w, h, pitch), dtype=np.uint8)
    return _randomise(zero, cformat, w, h, CLASSES, seed), pitch


def is_rgb(cformat):
    return cformat in synth.PACKED and (synth.PACKED[cformat][0] == "gbrp" or synth.PACKED[cformat][0] in synth.RGB_FAMILIES)


def legal_range(cformat, comp):
    """(legal min, legal max, max) of a component's code field: 16 .. 235 / 240 scaled to the depth; RGB: the whole range"""
    bits = 8 if (cformat in synth.FORMATS and synth.FORMATS[cformat][1] == 1) else synth.FORMATS[cformat][4] if cformat in synth.FORMATS else synth.PACKED[cformat][2]
    top = (1 << bits) - 1
    return (0, top, top) if is_rgb(cformat) else (16 << (bits - 8), (235 if comp == "Y" else 240) << (bits - 8), top)


def corner_values(cformat, comp):
    """the cycle of one component: 0, 1, legal min - 1, legal min, legal max, legal max + 1, max - 1, max of its code field (RGB: the legal range
    is the whole one), and for the LSB-aligned 10-bit formats the WORDS 1024, 1025, 0xFC00, 0xFFFF behind them"""
    lo, hi, top = legal_range(cformat, comp)
    vals = []
    for v in (0, 1, lo - 1, lo, hi, hi + 1, top - 1, top):
        if 0 <= v <= top and v not in vals:
            vals.append(v)
    return vals + (list(LSB10_EXTRA) if cformat in LSB10 else [])


CYCLE = {"Y": 13, "U": 11, "V": 7}         # pairwise coprime: along a row every combination of the three components' values meets


def _corner_plane(cformat, comp, rows, cols):
    """value index (x % L + L * y) % n: period L along the row (every 64-column strip and its tail sees the cycle), the window of the value
    list moving on from row to row so that lists longer than L are walked through as well"""
    vals = np.array(corner_values(cformat, comp), dtype=np.uint32)
    y, x = np.mgrid[0:rows, 0:cols]
    return vals[(x % CYCLE[comp] + CYCLE[comp] * y) % vals.size]


def corner_frame(cformat, w, h):
    """(sample, pitch): a deterministic frame of corner_values; low / alpha / pad bits as synth leaves them"""
    buf, pitch = synth.make_frame(cformat, w, h, "noise", seed=1)
    buf = buf.copy()
    for f in fields(cformat, w, h, pitch):
        if f.comp not in CYCLE or f.cls == "low":
            continue
        words = _corner_plane(cformat, f.comp, *f.idx.shape)
        put_field(buf, f, (words & 0x3ff) if (f.cls == "code" and cformat in LSB10) else (words >> 10) if f.cls == "high" else words)
    return buf, pitch


def sparse_edges(sample, cformat, w, h, every=7):
    """legal noise with every `every`-th sample of each component (row-major) replaced by corner_frame's: for routes behind a PQ / HLG tail,
    where the suite's cap on channels beyond one code is a rate measured on noise"""
    out = np.ascontiguousarray(sample).view(np.uint8).ravel().copy()
    corner, pitch = corner_frame(cformat, w, h)
    for f in fields(cformat, w, h, pitch):
        if f.comp not in CYCLE or f.cls == "low":
            continue
        pick = (np.arange(f.idx.size).reshape(f.idx.shape) % every) == every - 1
        put_field(out, f, np.where(pick, get_field(corner, f), get_field(out, f)))
    return out


def first_difference(a, b, sample, cformat, src_w, src_h, pitch=None):
    """for a failure message: the first pixel where two frames differ and the source words around the source position it maps to"""
    ys, xs = np.nonzero((a != b).any(axis=-1))
    if not ys.size:
        return "equal"
    y, x = int(ys[0]), int(xs[0])
    sx, sy = min(x * src_w // a.shape[1], src_w - 1), min(y * src_h // a.shape[0], src_h - 1)
    words = []
    for f in fields(cformat, src_w, src_h, pitch):
        r, c = min(sy * f.idx.shape[0] // src_h, f.idx.shape[0] - 1), min(sx * f.idx.shape[1] // src_w, f.idx.shape[1] - 1)
        word = int(np.ascontiguousarray(sample).view(np.uint8).ravel().view(f.dtype)[f.idx[r, c]])
        words.append(f"{f.comp}/{f.cls}@({r},{c}) word {word:#x}")
    return f"first differing pixel (x, y) = ({x}, {y}): {a[y, x].tolist()} vs {b[y, x].tolist()}; source ({sx}, {sy}): " + ", ".join(words)
