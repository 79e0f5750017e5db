"""The sharpen pass on the CPU (extension; include/mpcvr.h: mpcvr_sharpen_params_default, mpcvr_sharpen_host, mpcvr_plan_sharpen,
mpcvr_plan_batch_sharpen, and every refusal of mpcvr_sharpen_pass that is answered before a launch), against the model
(tests/sharpen_model.py).  mpcvr_sharpen_host compiles csrc/vp_sharpen_core.h, the arithmetic of the kernel.  Everything is bits: no
tolerance anywhere; the inequalities (ranges, the edge figures) are the consequences the header states."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import sharpen_model as SM
from tests.test_deband import PAIR_IDS, PAIRS, noise, plan_chunks, smooth

BGRA8, RGB10A2 = SM.BGRA8, SM.RGB10A2
RGB, LUMA = SM.RGB, SM.LUMA
RADII, MODES = (1, 2, 3), (RGB, LUMA)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constants():
    """the constants csrc/vp_sharpen.h exports: the tile and the staged image"""
    text = open(os.path.join(ROOT, "videorenderer_amd", "csrc", "vp_sharpen.h")).read()
    v = {k: int(n) for k, n in re.findall(r"constexpr int (kSharpen\w+) = (\d+);", text)}
    assert re.search(r"kSharpenTileRows = kSharpenWaves \* kSharpenWaveRows;", text) and re.search(r"kSharpenImageCols = kSharpenTileCols \+ 2 \* kSharpenPad;", text)
    v["kSharpenTileRows"] = v["kSharpenWaves"] * v["kSharpenWaveRows"]
    v["kSharpenImageCols"] = v["kSharpenTileCols"] + 2 * v["kSharpenPad"]
    return v


K = header_constants()


def lds_rule(r, mode):
    """SharpenLdsBytes of csrc/vp_sharpen.h, written out a second time"""
    return (K["kSharpenTileRows"] + 2 * r) * (K["kSharpenImageCols"] + K["kSharpenTileCols"] * (1 if mode == LUMA else 2)) * 4


def params(radius, amount, threshold, overshoot, mode, dither):
    return dict(radius=radius, amount=amount, threshold=threshold, overshoot=overshoot, mode=mode, dither=dither)


def model(words, src_fmt, dst_fmt, P, seed, counts=None):
    return SM.apply(words, src_fmt, dst_fmt, P["radius"], P["amount"], P["threshold"], P["overshoot"], P["mode"], P["dither"], seed, counts)


def host(words, src_fmt, dst_fmt, P, seed):
    from videorenderer_amd import api
    return api.sharpen_host(words, src_fmt, P, seed, dst_fmt)


def extremes(fmt, h, w, seed):
    """(h, w) uint32: every channel 0 or maxin, independently (with amount 256 these reach the bounds of steps 2 and 4), random A / X bits"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 2, size=(3, h, w)) * SM.MAXCODE[fmt]
    return SM.pack(c, fmt) ^ (rng.integers(0, 4, size=(h, w)).astype(np.uint32) << np.uint32(30))


# ---- the surfaces and parameters of the GPU tests (tests/test_sharpen_gpu.py imports them), so that the CPU suite can say what they exercise --
GPU_EXTENT = (2 * K["kSharpenTileRows"] + 1, 2 * K["kSharpenTileCols"] + 1)
_gpu_src = {}


def gpu_surface(fmt):
    """(2 TH + 1, 2 TW + 1) uint32: smooth with a code or two of noise and random A / X bits; made once per format.  Smaller surfaces are
    its top-left corner."""
    if fmt not in _gpu_src:
        _gpu_src[fmt] = smooth(fmt, GPU_EXTENT[0], GPU_EXTENT[1], 40 + fmt)
    return _gpu_src[fmt]


def gpu_params(radius, mode, dither=1):
    """amount 200 / 64, coring at three quarters of a code, one code of overshoot: on the smooth surfaces every branch is taken"""
    return params(radius, 200, 3, 1, mode, dither)


# ---- the host function against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=["rgb", "luma"])
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("src_fmt,dst_fmt", PAIRS, ids=PAIR_IDS)
def test_host_function_equals_the_model(mpcvr, src_fmt, dst_fmt, radius, mode):
    """noise, frames of only 0 and maxin (the bounds of steps 2 and 4, asserted inside the model) and smooth-plus-noise, 45 x 37; a 2 x 2
    and a 3 x 5 frame where every tap clamps; dither 0 and 1; seeds 0 and 0xffffffff"""
    m = SM.MAXCODE[src_fmt]
    for kind, words in (("noise", noise(src_fmt, 37, 45, 10 + src_fmt)), ("extremes", extremes(src_fmt, 37, 45, 30 + src_fmt)),
                        ("smooth", smooth(src_fmt, 37, 45, 20 + src_fmt)), ("tiny", noise(src_fmt, 2, 2, 3)), ("small", noise(src_fmt, 5, 3, 4))):
        for a, t, o, di, seed in ((256, 0, 0, 0, 0), (256, 0, m, 1, 0xffffffff), (64, 4, 2, 1, 0), (200, 3, 1, 0, 0xffffffff), (32, 4 * m, 0, 1, 5), (0, 0, 0, 0, 1)):
            P = params(radius, a, t, o, mode, di)
            got, want = host(words, src_fmt, dst_fmt, P, seed), model(words, src_fmt, dst_fmt, P, seed)
            assert np.array_equal(got, want), (kind, P, seed, int((got != want).sum()))


def test_the_bounds_of_steps_2_and_4_are_reached():
    """a centre at maxin in a field of 0 and the reverse, amount 256, threshold 0: |d| = S maxin - its own weight, the largest the
    definition allows but for the centre tap (the model asserts |d| <= S maxin and |v| < 2^31 on the way)"""
    for fmt in (BGRA8, RGB10A2):
        m = SM.MAXCODE[fmt]
        for r in RADII:
            c = np.zeros((3, 9, 9), dtype=np.int64)
            c[:, 4, 4] = m
            for words in (SM.pack(c, fmt), SM.pack(m - c, fmt)):
                for mode in MODES:
                    SM.apply(words, fmt, fmt, r, 256, 0, m, mode, 0, 0)


def test_host_function_with_padded_rows_writes_only_pixels(mpcvr):
    from videorenderer_amd import api
    words = smooth(RGB10A2, 9, 13, 3)
    P = params(3, 200, 3, 1, LUMA, 1)
    for poison in (0x00, 0xa5):
        sp, dp = 4 * 13 + 12, 4 * 13 + 20
        src = SM.place(np.full(9 * sp, poison, dtype=np.uint8), 0, words, sp)
        dst = np.full(9 * dp, 0x5a, dtype=np.uint8)
        api.sharpen_host(src, RGB10A2, P, 7, BGRA8, src_pitch=sp, dst=dst, dst_pitch=dp, w=13)
        want = SM.place(np.full(9 * dp, 0x5a, dtype=np.uint8), 0, model(words, RGB10A2, BGRA8, P, 7), dp)
        assert np.array_equal(dst, want), poison


# ---- the consequences the header lists -------------------------------------------------------------------------------------------------------
def unchanged(c, mi, mo):
    return c if mi == mo else (2 * c * mo + mi) // (2 * mi)


@pytest.mark.parametrize("src_fmt,dst_fmt", PAIRS, ids=PAIR_IDS)
def test_amount_zero_and_full_threshold_return_the_code(mpcvr, src_fmt, dst_fmt):
    """header: a = 0, and t = 4 maxin, with dither 0: out == c at equal depths, (2 c maxout + maxin) / (2 maxin) across depths; every code"""
    mi, mo = SM.MAXCODE[src_fmt], SM.MAXCODE[dst_fmt]
    rs = np.random.default_rng(4)
    c = np.stack([rs.permutation(np.arange(32 * 32) % (mi + 1)).reshape(32, 32) for _ in range(3)])
    assert all(np.unique(c[k]).size == mi + 1 for k in range(3))
    words = SM.pack(c, src_fmt)
    for r in RADII:
        for mode in MODES:
            for a, t in ((0, 0), (256, 4 * mi)):
                got = SM.codes(host(words, src_fmt, dst_fmt, params(r, a, t, mi, mode, 0), 9), dst_fmt)
                assert np.array_equal(got, unchanged(c, mi, mo)), (r, mode, a, t)


@pytest.mark.parametrize("src_fmt", (BGRA8, RGB10A2), ids=["bgra8", "rgb10"])
def test_a_flat_surface_is_returned_unchanged_for_every_parameter_set(mpcvr, src_fmt):
    m = SM.MAXCODE[src_fmt]
    for level in ((0, 0, 0), (m, m, m), (1, m // 2, m - 1)):
        c = np.stack([np.full((11, 19), v, dtype=np.int64) for v in level])
        words = SM.pack(c, src_fmt)
        for r in RADII:
            for mode in MODES:
                for a, t, o in ((256, 0, 0), (256, 0, m), (64, 4, 2)):
                    assert np.array_equal(host(words, src_fmt, src_fmt, params(r, a, t, o, mode, 0), 3), words), (level, r, mode, a, t, o)
                    got = SM.codes(host(words, src_fmt, 1 - src_fmt, params(r, a, t, o, mode, 0), 3), 1 - src_fmt)
                    assert np.array_equal(got, unchanged(c, m, SM.MAXCODE[1 - src_fmt]))


@pytest.mark.parametrize("src_fmt", (BGRA8, RGB10A2), ids=["bgra8", "rgb10"])
def test_two_levels_are_returned_unchanged_without_overshoot_and_stay_within_it_with(mpcvr, src_fmt):
    """header: two levels A <= B per channel, every channel at its A on the same texels: unchanged at o = 0 for every a, r, mode; with
    overshoot o within A - o .. B + o (and it does overshoot, so the statement is not vacuous).  A straight, a diagonal and a staircase edge."""
    y, x = np.mgrid[0:24, 0:32]
    A, B = np.array([100, 60, 10])[:, None, None], np.array([140, 200, 10])[:, None, None]       # (B is flat: A == B)
    for side in (x >= 15, x + y >= 27, (x // 3 + y // 2) >= 9):
        c = np.where(side[None], B, A).astype(np.int64)
        words = SM.pack(c, src_fmt)
        for r in RADII:
            for mode in MODES:
                for a in (32, 256):
                    assert np.array_equal(host(words, src_fmt, src_fmt, params(r, a, 0, 0, mode, 0), 11), words), (r, mode, a)
                got = SM.codes(host(words, src_fmt, src_fmt, params(r, 256, 0, 7, mode, 0), 11), src_fmt)
                assert (got >= A - 7).all() and (got <= B + 7).all() and not np.array_equal(got, c), (r, mode)
                assert got[:2].min() < A[:2].min() and got[:2].max() > B[:2].max()


@pytest.mark.parametrize("src_fmt", (BGRA8, RGB10A2), ids=["bgra8", "rgb10"])
def test_an_affine_gray_surface_is_returned_unchanged_where_no_tap_clamps(mpcvr, src_fmt):
    y, x = np.mgrid[0:20, 0:30]
    g = 20 + 3 * x + 2 * y
    assert g.max() <= 255
    words = SM.pack(np.stack([g, g, g]), src_fmt)
    changed = False
    for r in RADII:
        for mode in MODES:
            got = host(words, src_fmt, src_fmt, params(r, 256, 0, SM.MAXCODE[src_fmt], mode, 0), 2)
            assert np.array_equal(got[r:-r, r:-r], words[r:-r, r:-r]), (r, mode)
            changed |= not np.array_equal(got, words)
    assert changed, "the clamped border should differ: the statement about the interior is not vacuous"


@pytest.mark.parametrize("src_fmt,dst_fmt", PAIRS, ids=PAIR_IDS)
def test_on_gray_the_two_modes_agree(mpcvr, src_fmt, dst_fmt):
    g = SM.codes(noise(src_fmt, 21, 33, 6), src_fmt)[0]
    words = SM.pack(np.stack([g, g, g]), src_fmt)
    for r in RADII:
        for di in (0, 1):
            a, b = (host(words, src_fmt, dst_fmt, params(r, 96, 3, 5, mode, di), 8) for mode in MODES)
            assert np.array_equal(a, b), (r, di)
    assert not np.array_equal(a, words)


@pytest.mark.parametrize("src_fmt", (BGRA8, RGB10A2), ids=["bgra8", "rgb10"])
def test_without_overshoot_every_channel_stays_within_its_3x3_neighbourhood(mpcvr, src_fmt):
    for words in (noise(src_fmt, 23, 31, 12), smooth(src_fmt, 23, 31, 13)):
        c = SM.codes(words, src_fmt)
        mn, mx = c.copy(), c.copy()
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                n = SM.shifted(c, i, j)
                mn, mx = np.minimum(mn, n), np.maximum(mx, n)
        for r in RADII:
            for mode in MODES:
                got = SM.codes(host(words, src_fmt, src_fmt, params(r, 256, 0, 0, mode, 0), 1), src_fmt)
                assert (got >= mn).all() and (got <= mx).all(), (r, mode)


def test_what_it_does_to_an_edge(mpcvr, capsys):
    """the header's figures: the blurred 100 -> 900 step has a 10 - 90 % width of 4 texels; radius 2, amount 64, threshold 0 leaves 2; with
    o = 0 nothing leaves 100 .. 900, with o = 16 the extremes are 91 and 908.  From the model, and the host function agrees."""
    row = SM.edge_row()
    assert SM.width_10_90(row) == 4 and row.min() == 100 and row.max() == 900
    words = SM.pack(np.stack([np.tile(row, (9, 1))] * 3), RGB10A2)
    for mode in MODES:
        for o, lo, hi in ((0, 100, 900), (16, 91, 908)):
            P = params(2, 64, 0, o, mode, 0)
            out = model(words, RGB10A2, RGB10A2, P, 0)
            assert np.array_equal(out, host(words, RGB10A2, RGB10A2, P, 0))
            got = SM.codes(out, RGB10A2)
            with capsys.disabled():
                print("\nsharpen on the blurred edge, mode %d overshoot %d: width %d -> %d, codes %d .. %d" % (mode, o, SM.width_10_90(row), SM.width_10_90(got[0, 4]), got.min(), got.max()))
            assert all(SM.width_10_90(got[k, j]) == 2 for k in range(3) for j in range(9))
            assert (got.min(), got.max()) == (lo, hi)


@pytest.mark.parametrize("fmt", (BGRA8, RGB10A2), ids=["bgra8", "rgb10"])
def test_the_gpu_tests_surfaces_take_every_branch(fmt):
    """every branch of the definition — cored to zero, sharpened and unlimited, stopped by the limiter at lo and at hi — is taken on the
    surfaces the GPU tests compare, at their parameters: the 70 x 40 corner, the tile-sized corner and the whole surface, every radius and
    mode.  (The shapes of a few texels — 1 x 1, 2 x 2, 3 x 5, a single row or column — cannot take all four; they are there for the clamps.)"""
    full = gpu_surface(fmt)
    TH, TW = K["kSharpenTileRows"], K["kSharpenTileCols"]
    for h, w in ((40, 70), (TH, TW), GPU_EXTENT):
        for r in RADII:
            for mode in MODES:
                counts = {}
                model(np.ascontiguousarray(full[:h, :w]), fmt, fmt, gpu_params(r, mode), 1, counts)
                assert sum(counts.values()) == 3 * h * w and all(counts[b] > 0 for b in SM.BRANCHES), (h, w, r, mode, counts)


# ---- defaults, the plan call, refusals ---------------------------------------------------------------------------------------------------------
def test_defaults(mpcvr):
    from videorenderer_amd import api
    for fmt, th, o in ((BGRA8, 4, 2), (RGB10A2, 16, 8)):
        p = api.sharpen_params_default(fmt)
        assert (p.radius, p.amount, p.threshold, p.overshoot, p.mode, p.dither) == (2, 32, th, o, 1, 1)
    assert (api.SHARPEN_RGB_EXT, api.SHARPEN_LUMA_EXT) == (0, 1)
    L = api.load_library()
    assert L.mpcvr_sharpen_params_default(0, None) == api.E_POINTER
    assert L.mpcvr_sharpen_params_default(2, C.byref(api.SharpenParams())) == api.E_INVALIDARG


def test_the_plan_call_agrees_with_the_header(mpcvr):
    from videorenderer_amd import api
    for r in RADII:
        for mode in MODES:
            for w, h in ((1, 1), (64, 64), (1920, 1080), (32768, 32768)):
                assert api.plan_sharpen(RGB10A2, params(r, 32, 16, 8, mode, 1), w, h) == (r, lds_rule(r, mode))
    assert 2 * lds_rule(3, RGB) <= 160 * 1024 and lds_rule(3, RGB) <= 64 * 1024
    assert K["kSharpenPad"] >= max(RADII) and K["kSharpenPad"] % 4 == 0


BAD_PARAMS = {
    "radius_0": dict(radius=0), "radius_4": dict(radius=4), "amount_negative": dict(amount=-1), "amount_257": dict(amount=257),
    "threshold_negative": dict(threshold=-1), "threshold_above_4_maxin": dict(threshold=4 * 255 + 1), "overshoot_negative": dict(overshoot=-1),
    "overshoot_above_maxin": dict(overshoot=256), "mode_2": dict(mode=2), "mode_negative": dict(mode=-1), "dither_2": dict(dither=2),
    "dither_negative": dict(dither=-1),
}
OK = params(2, 32, 4, 2, 1, 1)


def test_the_plan_call_refuses(mpcvr):
    from videorenderer_amd import api
    L = api.load_library()

    def hr(fmt=BGRA8, w=64, h=4, **kw):
        return L.mpcvr_plan_sharpen(fmt, C.byref(api.SharpenParams(**dict(OK, **kw))), w, h, None, None)

    assert hr() == 0                                   # any out pointer may be NULL
    assert hr(fmt=RGB10A2, threshold=4 * 1023, overshoot=1023) == 0
    assert hr(fmt=RGB10A2, threshold=4 * 1023 + 1) == api.E_INVALIDARG and hr(fmt=RGB10A2, overshoot=1024) == api.E_INVALIDARG
    assert hr(threshold=4 * 255, overshoot=255, amount=256, radius=3) == 0
    for label, kw in BAD_PARAMS.items():
        assert hr(**kw) == api.E_INVALIDARG, label
    for kw in (dict(fmt=2), dict(fmt=-1), dict(w=0), dict(h=0), dict(w=32769), dict(h=32769)):
        assert hr(**kw) == api.E_INVALIDARG, kw
    assert L.mpcvr_plan_sharpen(0, None, 64, 4, None, None) == api.E_POINTER


# ---- the refusals of the pass that need no GPU (nothing is launched: the addresses are never touched) -----------------------------------
A = 0x7f0000000000                                             # an address nobody dereferences


def sharpen_pass_hr(src=A, src_pitch=256, src_fmt=0, w=64, h=4, p="ok", seed=0, dst=A + (1 << 20), dst_pitch=256, dst_fmt=0, **kw):
    from videorenderer_amd import api
    pp = None if p is None else C.byref(api.SharpenParams(**dict(OK, **kw)))
    return api.load_library().mpcvr_sharpen_pass(C.c_void_p(src), src_pitch, src_fmt, w, h, pp, seed, C.c_void_p(dst), dst_pitch, dst_fmt, None)


REFUSALS = {
    "null_src": (dict(src=0), "E_POINTER"),
    "null_params": (dict(p=None), "E_POINTER"),
    "null_dst": (dict(dst=0), "E_POINTER"),
    "src_fmt": (dict(src_fmt=2), "E_INVALIDARG"),
    "dst_fmt": (dict(dst_fmt=-1), "E_INVALIDARG"),
    "w_0": (dict(w=0), "E_INVALIDARG"),
    "w_big": (dict(w=32769, src_pitch=4 * 32769 + 4, dst_pitch=4 * 32769 + 4), "E_INVALIDARG"),
    "h_0": (dict(h=0), "E_INVALIDARG"),
    "h_big": (dict(h=32769), "E_INVALIDARG"),
    "src_pitch_short": (dict(src_pitch=252), "E_INVALIDARG"),
    "dst_pitch_short": (dict(dst_pitch=252), "E_INVALIDARG"),
    "src_odd": (dict(src=A + 2), "E_INVALIDARG"),
    "dst_odd": (dict(dst=A + (1 << 20) + 1), "E_INVALIDARG"),
    "src_pitch_odd": (dict(src_pitch=258), "E_INVALIDARG"),
    "dst_pitch_odd": (dict(dst_pitch=257), "E_INVALIDARG"),
    "in_place": (dict(dst=A), "E_INVALIDARG"),
    "dst_one_texel_into_src": (dict(dst=A + 4), "E_INVALIDARG"),
    "dst_one_row_into_src": (dict(dst=A + 256), "E_INVALIDARG"),
    "dst_last_texel_of_src": (dict(dst=A + 3 * 256 + 252), "E_INVALIDARG"),
    "dst_ends_inside_src": (dict(dst=A - 3 * 256 - 252), "E_INVALIDARG"),
    "dst_interleaved_with_src": (dict(src_pitch=512, dst_pitch=512, dst=A + 256), "E_INVALIDARG"),
}
REFUSALS.update({k: (v, "E_INVALIDARG") for k, v in BAD_PARAMS.items()})


@pytest.mark.parametrize("label", list(REFUSALS))
def test_sharpen_pass_refuses_before_any_launch(mpcvr, label):
    from videorenderer_amd import api
    kw, want = REFUSALS[label]
    assert sharpen_pass_hr(**kw) == getattr(api, want), label


def test_the_host_function_refuses_what_the_pass_refuses_and_writes_nothing(mpcvr):
    from videorenderer_amd import api
    L = api.load_library()
    buf = np.full(1 << 16, 0x5a, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data % 16)
    s0, d0 = base + 1024, base + 32768

    def hr(src=s0, sp=256, sf=0, w=64, h=4, p="ok", dst=d0, dp=256, df=0, **kw):
        pp = None if p is None else C.byref(api.SharpenParams(**dict(OK, **kw)))
        return L.mpcvr_sharpen_host(C.c_void_p(src), sp, sf, w, h, pp, 0, C.c_void_p(dst), dp, df)

    E = api.E_INVALIDARG
    for kw, want in ((dict(src=0), api.E_POINTER), (dict(p=None), api.E_POINTER), (dict(dst=0), api.E_POINTER), (dict(sf=2), E), (dict(df=2), E),
                     (dict(w=0), E), (dict(h=0), E), (dict(w=32769), E), (dict(h=32769), E), (dict(sp=252), E), (dict(dp=252), E), (dict(sp=258), E),
                     (dict(dp=258), E), (dict(src=s0 + 2), E), (dict(dst=d0 + 1), E), (dict(dst=s0), E), (dict(dst=s0 + 4), E),
                     (dict(dst=s0 + 3 * 256 + 252), E), (dict(dst=s0 - 3 * 256 - 252), E), (dict(sp=512, dp=512, dst=s0 + 256), E)):
        assert hr(**kw) == want, kw
    for label, kw in BAD_PARAMS.items():
        assert hr(**kw) == E, label
    assert bool((buf == 0x5a).all()), "a refused call wrote"
    # ... and the arguments they were derived from are accepted, touching surfaces included
    assert hr() == 0 and hr(dst=s0 + 3 * 256 + 256) == 0 and hr(dst=s0 - 3 * 256 - 256) == 0


@pytest.mark.parametrize("w,h,n,budget", [(1, 1, 1, 0), (5, 3, 7, 0), (64, 32, 7, 3 * 8192), (64, 32, 7, 1), (7680, 4320, 40, 0), (32768, 32768, 3, 0)])
def test_plan_batch_sharpen_is_plan_chunks_arithmetic(mpcvr, w, h, n, budget):
    from videorenderer_amd import api
    got = api.plan_batch_sharpen(w, h, n, budget)
    pitch = (4 * w + 15) // 16 * 16
    stride, fpc, chunks = plan_chunks(pitch * h, n, budget)
    assert got == dict(surface_pitch=pitch, frame_stride=stride, frames_per_chunk=fpc, chunks=chunks)
    assert got == api.plan_batch_tensor(w, h, n, budget)
    L = api.load_library()
    for bw, bh, bn in ((0, 4, 1), (4, 0, 1), (32769, 4, 1), (4, 32769, 1), (4, 4, 0)):
        assert L.mpcvr_plan_batch_sharpen(bw, bh, bn, 0, None, None, None, None) == api.E_INVALIDARG
