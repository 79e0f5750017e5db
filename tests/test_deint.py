"""The deinterlacing pass on the CPU (include/mpcvr.h: mpcvr_plan_deint_planes, mpcvr_deint_plane_host, mpcvr_plan_batch_deint) against the
model (tests/deint_model.py) and against the layout rule of the header, written out here a second time.  mpcvr_deint_plane_host compiles
the per-component function the kernel compiles (csrc/vp_deint_core.h).  Everything is bits: no tolerance anywhere.  The kernel itself:
tests/test_deint_gpu.py."""
import itertools

import numpy as np
import pytest

from tests import deint_model as M

E_POINTER, E_INVALIDARG = -2147467261, -2147024809          # 0x80004003, 0x80070057

# name: (cformat, planes, bytes, div_w, div_h, depth) — the header's table, not the library's
FORMATS = {
    "NV12": (1, 2, 1, 2, 2, 8), "P010": (2, 2, 2, 2, 2, 16), "P016": (3, 2, 2, 2, 2, 16), "P210": (6, 2, 2, 2, 1, 16), "P216": (7, 2, 2, 2, 1, 16),
    "YV12": (14, 3, 1, 2, 2, 8), "YV16": (15, 3, 1, 2, 1, 8), "YV24": (16, 3, 1, 1, 1, 8),
    "YUV420P8": (17, 3, 1, 2, 2, 8), "YUV422P8": (18, 3, 1, 2, 1, 8), "YUV444P8": (19, 3, 1, 1, 1, 8),
    "YUV420P10": (20, 3, 2, 2, 2, 10), "YUV420P16": (21, 3, 2, 2, 2, 16), "YUV422P10": (22, 3, 2, 2, 1, 10), "YUV422P16": (23, 3, 2, 2, 1, 16),
    "YUV444P10": (24, 3, 2, 1, 1, 10), "YUV444P16": (25, 3, 2, 1, 1, 16),
    "GBRP8": (26, 3, 1, 1, 1, 8), "GBRP10": (27, 3, 2, 1, 1, 10), "GBRP16": (28, 3, 2, 1, 1, 16),
    "Y8": (37, 1, 1, 1, 1, 8), "Y10": (38, 1, 2, 1, 1, 10), "Y16": (39, 1, 2, 1, 1, 16),
}
PACKED = {"YUY2": 4, "UYVY": 5, "Y210": 8, "Y216": 9, "v210": 10, "AYUV": 11, "Y410": 12, "Y416": 13,
          "RGB24": 29, "XRGB32": 30, "ARGB32": 31, "r210": 32, "RGB48": 33, "BGR48": 34, "BGRA64": 35, "b64a": 36}
assert len(FORMATS) == 23


def header_planes(name, w, h, pitch):
    """The planes by the text of include/mpcvr.h"""
    _, planes, by, dw, dh, depth = FORMATS[name]
    mask = 0xff if by == 1 else 0x3ff if depth == 10 else 0xffff
    out = [dict(offset=0, pitch=pitch, comps=w, lines=h, bytes=by, cs=1, mask=mask)]
    if planes == 2:
        out.append(dict(offset=pitch * h, pitch=pitch, comps=w // 2 * 2, lines=h // dh, bytes=by, cs=2, mask=mask))
    if planes == 3:
        cp, ch = pitch // dw, h // dh
        out.append(dict(offset=pitch * h, pitch=cp, comps=w // dw, lines=ch, bytes=by, cs=1, mask=mask))
        out.append(dict(offset=pitch * h + cp * ch, pitch=cp, comps=w // dw, lines=ch, bytes=by, cs=1, mask=mask))
    return out


@pytest.mark.parametrize("name", sorted(FORMATS))
def test_plan_deint_planes_matches_the_layout_rule_of_the_header(name):
    from videorenderer_amd import api
    cf, _, by, _, _, _ = FORMATS[name]
    for w, h, pad in ((64, 48, 0), (66, 52, 12), (1920, 1080, 128), (2, 4, 4)):
        if h % 4 or w % 2:
            continue
        frame_bytes, default = api.plan_frame_layout(cf, w, h)
        pitch = default + pad
        assert api.plan_deint_planes(cf, w, h, pitch) == header_planes(name, w, h, pitch), (name, w, h, pitch)
        assert api.plan_deint_planes(cf, w, h, 0) == header_planes(name, w, h, default), (name, w, h, "default pitch")
        # the planes lie inside the sample the context would take
        vp_bytes = max(p["offset"] + (p["lines"] - 1) * p["pitch"] + p["comps"] * by for p in api.plan_deint_planes(cf, w, h, pitch))
        assert vp_bytes <= frame_bytes // default * pitch


def _plan_hr(cf, w, h, pitch):
    import ctypes as C
    from videorenderer_amd import api
    n, out = C.c_int32(), (api.DeintPlane * 3)()
    return api.load_library().mpcvr_plan_deint_planes(cf, w, h, pitch, C.byref(n), out)


def test_plan_deint_planes_refuses_packed_formats_short_planes_and_illegal_pitches():
    import ctypes as C
    from videorenderer_amd import api
    for name, cf in PACKED.items():
        assert _plan_hr(cf, 64, 48, 0) == E_INVALIDARG, name
    assert _plan_hr(0, 64, 48, 0) == E_INVALIDARG and _plan_hr(99, 64, 48, 0) == E_INVALIDARG
    for name, (cf, planes, by, dw, dh, depth) in FORMATS.items():
        assert _plan_hr(cf, 64, 48, 0) == 0, name
        assert _plan_hr(cf, 64, 1, 0) == E_INVALIDARG, name                       # one line (odd, too, for 4:2:0)
        assert _plan_hr(cf, 64, 2, 0) == (E_INVALIDARG if dh == 2 else 0), name    # 4:2:0: a chroma plane of one line
        assert _plan_hr(cf, 64, 4, 0) == 0, name
        assert _plan_hr(cf, 64, 48, 64 * by - by) == E_INVALIDARG, name            # shorter than a row
        assert _plan_hr(cf, 64, 48, -64 * by) == E_INVALIDARG, name                # bottom-up is defined for the RGB formats only
        assert _plan_hr(cf, 0, 48, 0) == E_INVALIDARG and _plan_hr(cf, 16386, 48, 0) == E_INVALIDARG, name
        if dw == 2:
            assert _plan_hr(cf, 63, 48, 0) == E_INVALIDARG, name
        if dh == 2:
            assert _plan_hr(cf, 64, 46 + 1, 0) == E_INVALIDARG, name
        if by == 2:
            assert _plan_hr(cf, 64, 48, 129) == E_INVALIDARG, name                 # 16-bit samples: an even pitch
            assert _plan_hr(cf, 64, 48, 130) == (E_INVALIDARG if planes == 3 and dw == 2 else 0), name      # ... and an even chroma pitch
            assert _plan_hr(cf, 64, 48, 132) == 0, name
        else:
            assert _plan_hr(cf, 64, 48, 67) == 0, name
    n = C.c_int32()
    assert api.load_library().mpcvr_plan_deint_planes(1, 64, 48, 0, None, (api.DeintPlane * 3)()) == E_POINTER
    assert api.load_library().mpcvr_plan_deint_planes(1, 64, 48, 0, C.byref(n), None) == E_POINTER


def test_plan_batch_deint_is_the_chunk_rule():
    from videorenderer_amd import api
    assert api.plan_batch_deint(64, 72, 8) == dict(frame_stride=64 * 72, frames_per_chunk=8, chunks=1)
    assert api.plan_batch_deint(66, 73, 8, 3 * 4864 + 5) == dict(frame_stride=4864, frames_per_chunk=3, chunks=3)      # 66 * 73 = 4818 -> 4864
    assert api.plan_batch_deint(66, 73, 8, 1) == dict(frame_stride=4864, frames_per_chunk=1, chunks=8)
    for bad in ((0, 72, 8), (64, 0, 8), (64, 72, 0)):
        with pytest.raises(api.MpcvrError):
            api.plan_batch_deint(*bad)


# ---- the host function against the model ----
SHAPES = ((2, 1), (2, 2), (3, 2), (4, 3), (5, 7), (6, 8), (9, 70))      # lines x comps
MAXV = {1: 255, 2: 65535}


noise = M.noise


def host_plane(f, nbytes, cs, mask, keep, first, mode, pad=0, poison=0x5a):
    """mpcvr_deint_plane_host over f[0], f[1], f[2] held in rows padded by `pad` poisoned bytes; the destination likewise, its padding checked"""
    from videorenderer_amd import api
    lines, comps = f.shape[1:]
    pitch = comps * nbytes + pad
    src = np.full((3, lines, pitch), poison, dtype=np.uint8)
    for i in range(3):
        src[i, :, :comps * nbytes] = np.ascontiguousarray(f[i]).view(np.uint8).reshape(lines, comps * nbytes)
    dst = np.full((lines, pitch), 0xc3, dtype=np.uint8)
    api.deint_plane_host(src[0], src[1], src[2], pitch, comps, lines, nbytes, cs, mask, keep, first, mode, dst, pitch)
    assert (dst[:, comps * nbytes:] == 0xc3).all(), "the pitch padding of the destination was written"
    return np.ascontiguousarray(dst[:, :comps * nbytes]).view(f.dtype)


COMBOS = list(itertools.product((1, 2), (1, 2), (0, 1), (0, 1), (0, 1)))      # bytes, cs, mode, keep, first


def test_host_plane_equals_the_model_on_noise_and_the_noise_takes_every_branch():
    info, cases = {}, 0
    for (lines, comps), (nbytes, cs, mode, keep, first) in itertools.product(SHAPES, COMBOS):
        if comps % cs:
            continue
        f = noise(lines, comps, nbytes, 1000 * lines + 10 * comps + nbytes)
        mask = MAXV[nbytes]
        got = host_plane(f, nbytes, cs, mask, keep, first, mode, pad=(0 if cases % 2 else 6))
        want = M.deint_plane(f[0], f[1], f[2], keep, first, mode, cs, mask, info)
        assert np.array_equal(got, want), (lines, comps, nbytes, cs, mode, keep, first, np.argwhere(got != want)[:4].tolist())
        cases += 1
    assert cases == 4 * 32 + 3 * 16        # comps 1, 3, 7 with cs = 1 only
    # the inputs leave the centre direction, both edges of the temporal band are taken, and the interlacing check matters
    assert all(info["dir"][j] > 0 for j in (-2, -1, 0, 1, 2)), info
    assert info["band_lo"] > 0 and info["band_hi"] > 0 and info["check_raised"] > 0, info


def test_a_moving_diagonal_edge_selects_the_far_directions():
    """an edge that moves two components per line: the line above matches the line below four components further on, which is direction -2
    for an edge leaning right (up[x - 2] against dn[x + 2]) and +2 for one leaning left"""
    for slope, want in ((2, -2), (-2, 2)):
        lines, comps = 9, 64
        frames = []
        for t in range(3):
            y, x = np.mgrid[0:lines, 0:comps]
            edge = 32 + slope * (y - 4) + 4 * (t - 1)
            frames.append(np.where(x < edge, 40, 200).astype(np.uint8))
        info = {}
        M.deint_plane(frames[0], frames[1], frames[2], 0, 1, 0, 1, 255, info)
        assert info["dir"][want] > 0 and info["dir"][-want] == 0, (slope, info)
        got = host_plane(np.stack(frames), 1, 1, 255, 0, 1, 0)
        assert np.array_equal(got, M.deint_plane(frames[0], frames[1], frames[2], 0, 1, 0, 1, 255))


@pytest.mark.parametrize("nbytes,cs", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_properties(nbytes, cs):
    f = noise(9, 70, nbytes, 77 + nbytes + cs)
    mx = MAXV[nbytes]
    for keep, first, mode in itertools.product((0, 1), (0, 1), (0, 1)):
        o = host_plane(f, nbytes, cs, mx, keep, first, mode)
        assert np.array_equal(o[keep::2], f[1][keep::2]), "kept lines are cur's"
        still = np.stack([f[1]] * 3)
        s = host_plane(still, nbytes, cs, mx, keep, first, 1)
        assert np.array_equal(s, f[1]), "prev == cur == next without the check returns cur"
    assert not np.array_equal(host_plane(np.stack([f[1]] * 3), nbytes, cs, mx, 0, 1, 0), f[1]), "... with the check it does not, on noise"


def test_ten_bit_mask_ignores_the_dirty_bits():
    rng = np.random.default_rng(5)
    clean = rng.integers(0, 1024, size=(3, 9, 70)).astype(np.uint16)
    dirty = clean | (rng.integers(0, 64, size=clean.shape).astype(np.uint16) << 10)
    for keep, first, mode in itertools.product((0, 1), (0, 1), (0, 1)):
        a = host_plane(clean, 2, 1, 0x3ff, keep, first, mode)
        b = host_plane(dirty, 2, 1, 0x3ff, keep, first, mode)
        assert np.array_equal(a, b) and int(b.max()) <= 1023
        assert np.array_equal(b, M.deint_plane(dirty[0], dirty[1], dirty[2], keep, first, mode, 1, 0x3ff))


def test_sixteen_bit_extremes_do_not_wrap():
    rng = np.random.default_rng(6)
    f = np.where(rng.random((3, 9, 70)) < 0.5, 0, 65535).astype(np.uint16)
    for cs, keep, first, mode in itertools.product((1, 2), (0, 1), (0, 1), (0, 1)):
        o = host_plane(f, 2, cs, 0xffff, keep, first, mode)
        want = M.deint_plane(f[0], f[1], f[2], keep, first, mode, cs, 0xffff)      # (int64: the model cannot wrap)
        assert 0 <= int(want.min()) and int(want.max()) <= 65535
        assert np.array_equal(o, want)
        assert np.array_equal(o[keep::2], f[1][keep::2])


def test_host_plane_refusals():
    import ctypes as C
    from videorenderer_amd import api
    L = api.load_library()
    a = np.zeros((4, 8), dtype=np.uint8)
    d = np.full((4, 8), 7, dtype=np.uint8)
    p = lambda x: C.c_void_p(x.ctypes.data)

    def call(prev=a, cur=a, nxt=a, sp=8, comps=8, lines=4, by=1, cs=1, mask=255, keep=0, first=1, mode=0, dst=d, dp=8):
        return L.mpcvr_deint_plane_host(p(prev) if prev is not None else None, p(cur), p(nxt), sp, comps, lines, by, cs, mask, keep, first, mode,
                                        p(dst) if dst is not None else None, dp)
    assert call() == 0
    assert call(prev=None) == E_POINTER and call(dst=None) == E_POINTER
    for kw in (dict(by=3), dict(cs=3), dict(cs=2, comps=7), dict(comps=0), dict(lines=1), dict(mask=256), dict(keep=2), dict(first=-1), dict(mode=2),
               dict(sp=7), dict(dp=7), dict(by=2, comps=4, sp=9), dict(mask=-1)):
        d[:] = 7
        assert call(**kw) == E_INVALIDARG, kw
        assert (d == 7).all(), kw
