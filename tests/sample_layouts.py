"""Media samples at a row pitch of the caller's choosing, with every byte that is not a pixel poisoned (host only, numpy only).

videorenderer_amd.synth lays a frame out at the reference's default pitch with zeroed padding; relayout() moves its pixel bytes to another
luma pitch along the library's plane walk (MemCopyToTexSrcVideo, DX11VideoProcessor.cpp:1213-1252 — CHipVideoProcessor::FillConvertParams):

    planar / bi-planar     luma rows at `pitch`; the interleaved UV plane at `pitch`; the two chroma planes of three-plane formats at
                           `pitch // div_w`, back to back behind pitch * height
    planar RGB (G, B, R)   three planes at `pitch`
    everything else        one plane (v210: whole 16-byte groups of six pixels are the row's pixel bytes)

The buffer is pitch * lines bytes (lines = height * PitchCoeff / 2, m_srcLines) — what mpcvr_get_frame_bytes reports; where `pitch // div_w`
floors (an odd pitch), the bytes behind the last chroma row belong to the padding as well.  Pixel VALUES are synth's: nothing here changes one.
"""
import numpy as np

from videorenderer_amd import synth

ALL_FORMATS = sorted(list(synth.FORMATS) + list(synth.PACKED))
RGB_FORMATS = sorted(cf for cf, v in synth.PACKED.items() if v[0] in synth.RGB_FAMILIES)
RGB_BPP = {"rgb24": 3, "rgb32": 4, "r210": 4, "rgb48": 6, "bgr48": 6, "bgra64": 8, "b64a": 8}


def sample_bytes(cformat):
    """bytes per stored component (what InitMediaType's alignment rules go by: 2 => an even pitch, 4 => a multiple of 4)"""
    if cformat in synth.FORMATS:
        return synth.FORMATS[cformat][1]
    kind, nbytes = synth.PACKED[cformat][:2]
    return 4 if kind in ("v210", "r210") else nbytes


def row_bytes(cformat, w):
    """pixel bytes of one luma (or only) row"""
    if cformat in synth.FORMATS:
        return w * synth.FORMATS[cformat][1]
    kind, nbytes = synth.PACKED[cformat][:2]
    if kind in ("yuy2", "uyvy", "y210"):
        return w * 2 * nbytes
    if kind == "v210":
        return (w + 5) // 6 * 16
    if kind in ("ayuv", "y410"):
        return w * 4
    if kind == "y416":
        return w * 8
    if kind in synth.RGB_FAMILIES:
        return w * RGB_BPP[kind]
    return w * nbytes           # gbrp, gray


def source_lines(cformat, h):
    """m_srcLines: height * PitchCoeff / 2 (Helper.cpp:295-359)"""
    if cformat in synth.FORMATS:
        planes, nbytes, dw, dh = synth.FORMATS[cformat][:4]
        coeff = 3 if (dw, dh) == (2, 2) else 4 if (dw, dh) == (2, 1) else 6
    else:
        coeff = 6 if synth.PACKED[cformat][0] == "gbrp" else 2
    return h * coeff // 2


def plane_walk(cformat, w, h, pitch):
    """[(first byte, rows, bytes from row to row, pixel bytes per row)] of every plane of a sample whose luma pitch is `pitch`"""
    rb = row_bytes(cformat, w)
    assert pitch >= rb, (cformat, w, pitch)
    if cformat in synth.PACKED:
        n = 3 if synth.PACKED[cformat][0] == "gbrp" else 1
        return [(i * pitch * h, h, pitch, rb) for i in range(n)]
    planes, nbytes, dw, dh = synth.FORMATS[cformat][:4]
    cw, ch = w // dw, h // dh
    walk = [(0, h, pitch, rb)]
    if planes == 2:
        walk.append((pitch * h, ch, pitch, 2 * cw * nbytes))
    else:
        cpitch = pitch // dw
        assert cpitch >= cw * nbytes, (cformat, w, pitch)
        walk.append((pitch * h, ch, cpitch, cw * nbytes))
        walk.append((pitch * h + cpitch * ch, ch, cpitch, cw * nbytes))
    return walk


def frame_bytes(cformat, w, h, pitch):
    return pitch * source_lines(cformat, h)


def poison_pattern(n, seed):
    """the issue's non-constant pattern over the byte index"""
    i = np.arange(n, dtype=np.int64)
    return ((131 * i + 17 * seed) & 0xff).astype(np.uint8)


def pixel_mask(cformat, w, h, pitch):
    """True at every byte of the pitch * lines buffer that belongs to a pixel"""
    m = np.zeros(frame_bytes(cformat, w, h, pitch), dtype=bool)
    for off, rows, pp, rb in plane_walk(cformat, w, h, pitch):
        m[off: off + rows * pp].reshape(rows, pp)[:, :rb] = True
    return m


def strip(buf, cformat, w, h, pitch):
    """the pixel bytes of a sample at `pitch`, plane after plane and row after row (the same for every pitch of the same picture)"""
    buf = np.ascontiguousarray(buf).view(np.uint8).ravel()
    assert buf.size == frame_bytes(cformat, w, h, pitch), (buf.size, cformat, w, h, pitch)
    return np.concatenate([buf[off: off + rows * pp].reshape(rows, pp)[:, :rb].ravel() for off, rows, pp, rb in plane_walk(cformat, w, h, pitch)])


def relayout(frame, cformat, w, h, pitch, poison):
    """A frame of synth.make_frame (default pitch, top-down) re-laid at luma pitch `pitch`: uint8, pitch * lines bytes.
    poison: None — padding bytes are zero, as synth leaves them; an int — padding bytes are poison_pattern(size, poison), moved on by one
    wherever a byte would equal the pixel byte in front of its run of padding or the one behind it (so no padding byte continues a pixel)."""
    frame = np.ascontiguousarray(frame).view(np.uint8).ravel()
    src_pitch = synth.default_pitch(cformat, w)
    assert frame.size == frame_bytes(cformat, w, h, src_pitch), (frame.size, cformat, w, h)
    total = frame_bytes(cformat, w, h, pitch)
    out = np.zeros(total, dtype=np.uint8) if poison is None else poison_pattern(total, poison)
    for (so, rows, sp, rb), (do, drows, dp, drb) in zip(plane_walk(cformat, w, h, src_pitch), plane_walk(cformat, w, h, pitch)):
        assert (rows, rb) == (drows, drb)
        out[do: do + rows * dp].reshape(rows, dp)[:, :rb] = frame[so: so + rows * sp].reshape(rows, sp)[:, :rb]
    if poison is not None:
        mask = pixel_mask(cformat, w, h, pitch)
        pad = np.flatnonzero(~mask)
        if pad.size:
            pix = np.flatnonzero(mask)
            # the pixel byte in front of / behind each padding byte's run (the buffer starts with a pixel; behind the last run: the last pixel again)
            at = np.searchsorted(pix, pad)
            left = out[pix[at - 1]]
            right = out[pix[np.minimum(at, pix.size - 1)]]
            v = out[pad]
            for _ in range(2):
                clash = (v == left) | (v == right)
                v[clash] += 1
            assert not ((v == left) | (v == right)).any()
            out[pad] = v
            assert out[pad].any()
    return out


def bottom_up(buf, h, pitch):
    """BI_RGB with biHeight > 0: rows stored last-first, handed over with a negative pitch (DX11VideoProcessor.cpp:1801-1803) — tests/golden/cases.py::case_frame"""
    return np.ascontiguousarray(buf.reshape(h, pitch)[::-1]).reshape(-1), -pitch


# ---- pitch classes ------------------------------------------------------------------------------------------------------------------
PITCH_CLASSES = ("wide", "mod16=8", "mod8=4", "mod4=2", "odd")


def pitch_of(cls, cformat, w):
    """The smallest luma pitch of a class above the tight row (row_bytes), or None where InitMediaType's rules leave the class empty
    for the format (16-bit samples: even; 32-bit texels and v210: a multiple of 4; `odd`: 1-byte samples only)."""
    t, b = row_bytes(cformat, w), sample_bytes(cformat)
    if cls == "tight":
        return synth.default_pitch(cformat, w)
    if cls == "wide":
        return (t // 256 + 1) * 256
    mod, res = {"mod16=8": (16, 8), "mod8=4": (8, 4), "mod4=2": (4, 2), "odd": (2, 1)}[cls]
    if (cls == "odd" and b != 1) or (cls == "mod4=2" and b == 4):
        return None
    p = t + 1
    while p % mod != res:
        p += 1
    return p


# ---- what the reference's RGB copy loops write (Helper.cpp, restated by orc_repack_rgb in oracle/mpcvr_oracle.c) ------------------------
def rgb_texels_written(kind, pitch, w):
    """How many texels of a `w`-texel texture row CopyFrame<kind> fills from a sample row of |pitch| bytes: line_pixels = |pitch| / bpp drives
    every loop, not the width.
      rgb32 (CopyPlaneAsIs, Helper.cpp:414-428), r210 (:770-787), bgra64 (:647-663), b64a (:665-683): line_pixels texels;
      rgb48 (CopyFrameRGB48, :541-565): whole groups of four only — line_pixels & ~3, no remainder branch;
      rgb24 (CopyFrameRGB24, :446-482): groups of four, then ONE texel if line_pixels is odd, two if it is even — a remainder of three loses two;
      bgr48 (CopyFrameBGR48, :600-645): groups of four and a remainder branch for one, two and three: line_pixels texels."""
    lp = abs(pitch) // RGB_BPP[kind]
    if kind == "rgb48":
        lp &= ~3
    elif kind == "rgb24" and lp % 4 == 3:
        lp -= 2
    return min(lp, w)
