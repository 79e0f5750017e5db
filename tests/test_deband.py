"""The deband pass on the CPU (extension; include/mpcvr.h: mpcvr_deband_params_default, mpcvr_deband_host, mpcvr_plan_deband,
mpcvr_plan_batch_deband, and every refusal of mpcvr_deband_pass that is answered before a launch), against the model
(tests/deband_model.py).  mpcvr_deband_host compiles csrc/vp_deband_core.h, the arithmetic of the kernel.  Everything is bits: no
tolerance anywhere; the one inequality (the pass does deband a quantised ramp) is a condition on the definition."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import deband_model as DM

BGRA8, RGB10A2 = DM.BGRA8, DM.RGB10A2
PAIRS = [(s, d) for s in (BGRA8, RGB10A2) for d in (BGRA8, RGB10A2)]
PAIR_IDS = ["%s-to-%s" % ("rgb10" if s else "bgra8", "rgb10" if d else "bgra8") for s, d in PAIRS]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constants():
    """the constants csrc/vp_deband.h exports: the tile, the LDS limit and the dispatcher's rule"""
    text = open(os.path.join(ROOT, "videorenderer_amd", "csrc", "vp_deband.h")).read()
    v = {k: int(n) for k, n in re.findall(r"constexpr int (kDeband\w+) = (\d+);", text)}
    assert re.search(r"kDebandTileRows = kDebandWaves \* kDebandWaveRows;", text)
    v["kDebandTileRows"] = v["kDebandWaves"] * v["kDebandWaveRows"]
    # the rule itself, as the header writes it
    assert re.search(r"constexpr int DebandPlacement\(int R, int /\*w\*/, int /\*h\*/\) \{ return R <= kDebandLdsMaxR \? DB_LDS : DB_GLOBAL; \}", text), "the rule changed: rewrite rule()"
    return v


K = header_constants()


def rule(R, w, h):
    """DebandPlacement of csrc/vp_deband.h, written out a second time"""
    return "lds" if R <= K["kDebandLdsMaxR"] else "global"


def noise(fmt, h, w, seed):
    """(h, w) uint32 of noise in all 32 bits (the A / X bits are random)"""
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=(h, w), dtype=np.uint64).astype(np.uint32)


def smooth(fmt, h, w, seed):
    """(h, w) uint32: a slow two-axis ramp plus noise of a code or two per channel, so that thresholds in between accept some taps and refuse others"""
    rng = np.random.default_rng(seed)
    m = DM.MAXCODE[fmt]
    y, x = np.mgrid[0:h, 0:w]
    c = np.stack([np.clip(m // 3 + (x * (k + 1) + y * (3 - k)) // 7 + rng.integers(-2, 3, size=(h, w)), 0, m) for k in range(3)])
    return DM.pack(c, fmt) ^ (rng.integers(0, 4, size=(h, w)).astype(np.uint32) << np.uint32(30))      # (random A / X bits)


def params(rng, it, th, di):
    return dict(range=rng, iterations=it, threshold=th, dither=di)


def host(words, src_fmt, dst_fmt, rng, it, th, di, seed):
    from videorenderer_amd import api
    return api.deband_host(words, src_fmt, params(rng, it, th, di), seed, dst_fmt)


# (range, iterations) at every bound: range 1 and 64, iterations 1 and 4, R = 64 three ways, and the defaults
SHAPES = [(1, 1), (1, 4), (64, 1), (16, 4), (32, 2), (16, 2), (7, 3)]


@pytest.mark.parametrize("rng,it", SHAPES)
@pytest.mark.parametrize("src_fmt,dst_fmt", PAIRS, ids=PAIR_IDS)
def test_host_function_equals_the_model(mpcvr, src_fmt, dst_fmt, rng, it):
    """noise (most taps refused at small thresholds, all accepted at 4 maxin) and a smooth surface (a mix), 45 x 37: smaller than R = 64
    in both directions, so every tap direction clamps; thresholds 0, in between and 4 maxin; dither 0 / 1; seeds 0 and 0xffffffff"""
    m = DM.MAXCODE[src_fmt]
    for kind, words in (("noise", noise(src_fmt, 37, 45, 10 + src_fmt)), ("smooth", smooth(src_fmt, 37, 45, 20 + src_fmt))):
        for th, di, seed in ((0, 0, 0), (0, 1, 0xffffffff), (4 * m, 1, 0), (4 * m, 0, 0xffffffff), (12 if src_fmt else 6, 1, 5), (40, 0, 0)):
            got = host(words, src_fmt, dst_fmt, rng, it, th, di, seed)
            want = DM.apply(words, src_fmt, dst_fmt, rng, it, th, di, seed)
            assert np.array_equal(got, want), (kind, rng, it, th, di, seed, int((got != want).sum()))


def test_host_function_with_padded_rows_writes_only_pixels(mpcvr):
    from videorenderer_amd import api
    words = smooth(RGB10A2, 9, 13, 3)
    for poison in (0x00, 0xa5):
        sp, dp = 4 * 13 + 12, 4 * 13 + 20
        src = DM.place(np.full(9 * sp, poison, dtype=np.uint8), 0, words, sp)
        dst = np.full(9 * dp, 0x5a, dtype=np.uint8)
        api.deband_host(src, RGB10A2, params(4, 2, 16, 1), 7, BGRA8, src_pitch=sp, dst=dst, dst_pitch=dp, w=13)
        want = DM.place(np.full(9 * dp, 0x5a, dtype=np.uint8), 0, DM.apply(words, RGB10A2, BGRA8, 4, 2, 16, 1, 7), dp)
        assert np.array_equal(dst, want), poison


@pytest.mark.parametrize("src_fmt,dst_fmt", PAIRS, ids=PAIR_IDS)
def test_threshold_zero_returns_the_code(mpcvr, src_fmt, dst_fmt):
    """header: threshold == 0, dither 0: out == c at equal depths, (2 c maxout + maxin) / (2 maxin) across depths — every code"""
    mi, mo = DM.MAXCODE[src_fmt], DM.MAXCODE[dst_fmt]
    rs = np.random.default_rng(4)
    c = np.stack([rs.permutation(np.arange(32 * 32) % (mi + 1)).reshape(32, 32) for _ in range(3)])
    assert all(np.unique(c[k]).size == mi + 1 for k in range(3))
    for rng, it in ((16, 4), (1, 1), (64, 1)):
        got = DM.codes(host(DM.pack(c, src_fmt), src_fmt, dst_fmt, rng, it, 0, 0, 9), dst_fmt)
        want = c if mi == mo else (2 * c * mo + mi) // (2 * mi)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("src_fmt", (BGRA8, RGB10A2), ids=["bgra8", "rgb10"])
def test_a_flat_surface_is_returned_unchanged_for_every_threshold(mpcvr, src_fmt):
    m = DM.MAXCODE[src_fmt]
    for level in ((0, 0, 0), (m, m, m), (1, m // 2, m - 1)):
        c = np.stack([np.full((20, 33), v, dtype=np.int64) for v in level])
        words = DM.pack(c, src_fmt)
        for th in (0, 1, 16, 4 * m):
            for di in (0, 1):
                assert np.array_equal(host(words, src_fmt, src_fmt, 16, 4, th, di, 3), words), (level, th, di)


@pytest.mark.parametrize("src_fmt", (BGRA8, RGB10A2), ids=["bgra8", "rgb10"])
def test_two_levels_farther_apart_than_the_threshold_are_returned_unchanged(mpcvr, src_fmt):
    """header: |A - B| > threshold per channel -> unchanged at equal depths with dither 0.  A vertical and a diagonal edge; the G edge
    runs the other way (high to low), B steps by exactly threshold + 1.  And the converse, so that the test is not vacuous: with
    |A - B| == threshold texels beside the edge do change."""
    th = 24
    y, x = np.mgrid[0:48, 0:64]
    for side in (x >= 31, x + y >= 50):
        c = np.stack([np.where(side, 140, 100), np.where(side, 60, 200), np.where(side, 10 + th + 1, 10)]).astype(np.int64)
        words = DM.pack(c, src_fmt)
        for rng, it in ((16, 4), (3, 2), (64, 1)):
            assert np.array_equal(host(words, src_fmt, src_fmt, rng, it, th, 0, 11), words), (rng, it)
        c[2] = np.where(side, 10 + th, 10)
        words = DM.pack(c, src_fmt)
        got = host(words, src_fmt, src_fmt, 3, 1, th, 0, 11)
        assert not np.array_equal(got, words) and np.array_equal(DM.codes(got, src_fmt)[:2], c[:2])


def test_it_does_deband_a_quantised_ramp(mpcvr, capsys):
    """a 64 x 512 RGB10A2 ramp of slope 0.25 code per pixel quantised to multiples of 4: the output's mean absolute distance to the
    unquantised ramp must be below the input's (range 16, iterations 4, threshold 24, dither 0, seed 1).  A condition on the definition."""
    h, w = 64, 512
    ideal = 300.0 + 0.25 * np.arange(w, dtype=np.float64)[None, :].repeat(h, 0)
    q = (np.floor(ideal / 4.0 + 0.5) * 4.0).astype(np.int64)          # the nearest multiple of 4: plateaus 16 pixels wide, 4 codes high
    words = DM.pack(np.stack([q, q, q]), RGB10A2)
    got = DM.codes(host(words, RGB10A2, RGB10A2, 16, 4, 24, 0, 1), RGB10A2)
    assert np.array_equal(DM.pack(got, RGB10A2), DM.apply(words, RGB10A2, RGB10A2, 16, 4, 24, 0, 1))
    err_in, err_out = float(np.abs(q - ideal).mean()), float(np.abs(got[0] - ideal).mean())
    with capsys.disabled():
        print("\ndeband on a quantised ramp: mean |error| %.3f -> %.3f codes, ratio %.3f" % (err_in, err_out, err_out / err_in))
    assert err_out < err_in


def test_defaults(mpcvr):
    from videorenderer_amd import api
    for fmt, th in ((BGRA8, 4), (RGB10A2, 16)):
        p = api.deband_params_default(fmt)
        assert (p.range, p.iterations, p.threshold, p.dither) == (16, 2, th, 1)
    L = api.load_library()
    assert L.mpcvr_deband_params_default(0, None) == api.E_POINTER
    assert L.mpcvr_deband_params_default(2, C.byref(api.DebandParams())) == api.E_INVALIDARG


def test_the_plan_call_agrees_with_the_header(mpcvr, monkeypatch):
    from videorenderer_amd import api
    monkeypatch.delenv("MPCVR_DEBAND_TAPS", raising=False)
    fit = K["kDebandLdsFitR"]
    assert K["kDebandLdsMaxR"] <= fit and (K["kDebandTileCols"] + 2 * fit) * (K["kDebandTileRows"] + 2 * fit) * 4 * 2 <= 160 * 1024
    seen = set()
    for rng in (1, 2, 3, 8, 11, 16, 17, 32, 33, 64):
        for it in (1, 2, 3, 4):
            if rng * it > 64:
                continue
            for w, h in ((1, 1), (64, 64), (1920, 1080), (32768, 32768)):
                R, place = api.plan_deband(RGB10A2, params(rng, it, 16, 1), w, h)
                assert R == rng * it and place == rule(R, w, h), (rng, it, w, h, place)
                seen.add(place)
    assert seen == {"lds", "global"}, "the rule never selects %s: that placement should not be in the build" % ({"lds", "global"} - seen)
    # the override, where the placement is possible
    monkeypatch.setenv("MPCVR_DEBAND_TAPS", "global")
    assert api.plan_deband(BGRA8, params(1, 1, 0, 0), 70, 40) == (1, "global")
    monkeypatch.setenv("MPCVR_DEBAND_TAPS", "lds")
    assert api.plan_deband(BGRA8, params(fit, 1, 0, 0), 70, 40) == (fit, "lds")
    assert api.plan_deband(BGRA8, params(fit + 1, 1, 0, 0), 70, 40) == (fit + 1, "global")
    monkeypatch.setenv("MPCVR_DEBAND_TAPS", "else")
    assert api.plan_deband(BGRA8, params(1, 1, 0, 0), 70, 40) == (1, rule(1, 70, 40))


BAD_PARAMS = {
    "range_0": dict(range=0), "range_65": dict(range=65), "iterations_0": dict(iterations=0), "iterations_5": dict(iterations=5),
    "halo_66": dict(range=33, iterations=2), "halo_68": dict(range=17, iterations=4), "threshold_negative": dict(threshold=-1),
    "threshold_above_4_maxin": dict(threshold=4 * 255 + 1), "dither_2": dict(dither=2), "dither_negative": dict(dither=-1),
}


def test_the_plan_call_refuses(mpcvr):
    from videorenderer_amd import api
    L = api.load_library()
    ok = params(16, 2, 4, 1)

    def hr(fmt=BGRA8, w=64, h=4, **kw):
        return L.mpcvr_plan_deband(fmt, C.byref(api.DebandParams(**dict(ok, **kw))), w, h, None, None)

    assert hr() == 0                                   # any out pointer may be NULL
    assert hr(fmt=RGB10A2, threshold=4 * 1023) == 0 and hr(fmt=RGB10A2, threshold=4 * 1023 + 1) == api.E_INVALIDARG
    for label, kw in BAD_PARAMS.items():
        assert hr(**kw) == api.E_INVALIDARG, label
    for kw in (dict(fmt=2), dict(fmt=-1), dict(w=0), dict(h=0), dict(w=32769), dict(h=32769)):
        assert hr(**kw) == api.E_INVALIDARG, kw
    assert L.mpcvr_plan_deband(0, None, 64, 4, None, None) == api.E_POINTER


# ---- the refusals of the pass that need no GPU (nothing is launched: the addresses are never touched) -----------------------------------
A = 0x7f0000000000                                             # an address nobody dereferences


def deband_pass_hr(src=A, src_pitch=256, src_fmt=0, w=64, h=4, p="ok", seed=0, dst=A + (1 << 20), dst_pitch=256, dst_fmt=0, **kw):
    from videorenderer_amd import api
    pp = None if p is None else C.byref(api.DebandParams(**dict(params(16, 2, 4, 1), **kw)))
    return api.load_library().mpcvr_deband_pass(C.c_void_p(src), src_pitch, src_fmt, w, h, pp, seed, C.c_void_p(dst), dst_pitch, dst_fmt, None)


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
def test_deband_pass_refuses_before_any_launch(mpcvr, label):
    from videorenderer_amd import api
    kw, want = REFUSALS[label]
    assert deband_pass_hr(**kw) == getattr(api, want), label


def test_the_host_function_refuses_what_the_pass_refuses_and_writes_nothing(mpcvr):
    from videorenderer_amd import api
    L = api.load_library()
    buf = np.full(1 << 16, 0x5a, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data % 16)
    s0, d0 = base + 1024, base + 32768

    def hr(src=s0, sp=256, sf=0, w=64, h=4, p="ok", dst=d0, dp=256, df=0, **kw):
        pp = None if p is None else C.byref(api.DebandParams(**dict(params(16, 2, 4, 1), **kw)))
        return L.mpcvr_deband_host(C.c_void_p(src), sp, sf, w, h, pp, 0, C.c_void_p(dst), dp, df)

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


def plan_chunks(frame_bytes, n, budget):
    """PlanChunks of csrc/vp_plan.h, by hand"""
    stride = (frame_bytes + 255) // 256 * 256
    fit = (budget or (4 << 30)) // stride
    fpc = max(1, min(n, fit))
    return stride, fpc, (n + fpc - 1) // fpc


@pytest.mark.parametrize("w,h,n,budget", [(1, 1, 1, 0), (5, 3, 7, 0), (64, 32, 7, 3 * 8192), (64, 32, 7, 1), (7680, 4320, 40, 0), (32768, 32768, 3, 0)])
def test_plan_batch_deband_is_plan_chunks_arithmetic(mpcvr, w, h, n, budget):
    from videorenderer_amd import api
    got = api.plan_batch_deband(w, h, n, budget)
    pitch = (4 * w + 15) // 16 * 16
    stride, fpc, chunks = plan_chunks(pitch * h, n, budget)
    assert got == dict(surface_pitch=pitch, frame_stride=stride, frames_per_chunk=fpc, chunks=chunks)
    assert got == api.plan_batch_tensor(w, h, n, budget)
    L = api.load_library()
    for bw, bh, bn in ((0, 4, 1), (4, 0, 1), (32769, 4, 1), (4, 32769, 1), (4, 4, 0)):
        assert L.mpcvr_plan_batch_deband(bw, bh, bn, 0, None, None, None, None) == api.E_INVALIDARG
