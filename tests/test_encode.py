"""The RGB -> NV12 / P010 pass (extension; include/mpcvr.h: mpcvr_plan_encode / mpcvr_encode_pass) on the CPU: the planner's integers, the
range of the 32-bit arithmetic, and the definition closed through the oracle — a frame encoded by the model (tests/encode_model.py) and
handed to the oracle as an NV12 / P010 sample comes back as the frame.  The kernel itself: tests/test_encode_gpu.py."""
import itertools

import numpy as np
import pytest

from tests import encode_model as EM
from tests.golden.cases import FULL, M240, M601, M709, M2020, MPEG1, MPEG2, COSITED, MYCGCO, TV, ext

NV12, P010 = 1, 2
BGRA8, RGB10A2 = 0, 1
MATRICES = {"601": M601, "709": M709, "240M": M240, "2020nc": M2020, "YCgCo": MYCGCO}
RANGES = {"limited": TV, "full": FULL}
PAIRS = [(o, s, m, r) for o in (NV12, P010) for s in (BGRA8, RGB10A2) for m in MATRICES for r in RANGES]
PAIR_IDS = ["%s-from-%s-%s-%s" % ("P010" if o == P010 else "NV12", "rgb10" if s else "bgra8", m, r) for o, s, m, r in PAIRS]


def scales(out_cformat, src_fmt):
    return (65535.0 / 64.0 if out_cformat == P010 else 255.0), (1023.0 if src_fmt == RGB10A2 else 255.0)


@pytest.mark.parametrize("out_cformat,src_fmt,matrix,rng", PAIRS, ids=PAIR_IDS)
def test_planned_integers_are_the_scaled_inverse_of_the_colour_matrix(mpcvr, out_cformat, src_fmt, matrix, rng):
    """coef = rint(inverse(M) T / maxin 2^S), off = rint(-(inverse(M) c) T 2^S) with (M, c) from mpcvr_plan_color_matrix: against numpy's
    inverse, to one unit of 2^-S per coefficient (two correct double inversions differ on an rint tie at most: 1.5e-5 of a coefficient,
    under 0.02 code at 10 bits) and, for the offsets, to what one unit in each coefficient of the row implies: an error e in N[i][j] moves
    off[i] by e |c[j]| T 2^S, and a unit of coef is e = maxin / (T 2^S) — sum_j |c[j]| maxin units, plus one for the rint."""
    from videorenderer_amd import api
    e = ext(MPEG2, RANGES[rng], MATRICES[matrix])
    plan = api.plan_encode(out_cformat, src_fmt, e)
    cm, ex = api.plan_color_matrix(out_cformat, 64, 32, e)
    assert plan["extfmt"] == ex and plan["shift"] == 16
    M = np.array(cm[:9], dtype=np.float64).reshape(3, 3)
    c = np.array(cm[9:], dtype=np.float64)
    T, maxin = scales(out_cformat, src_fmt)
    one = float(1 << plan["shift"])
    N = np.linalg.inv(M)
    want_coef = np.rint(N * T / maxin * one)
    want_off = np.rint(-(N @ c) * T * one)
    d = np.abs(plan["coef"].astype(np.int64) - want_coef.astype(np.int64))
    print("coef differ by at most", d.max(), "off by", np.abs(plan["off"] - want_off).max())
    assert d.max() <= 1, (plan["coef"], want_coef)
    bound = np.abs(c).sum() * maxin + 1
    assert np.abs(plan["off"].astype(np.int64) - want_off.astype(np.int64)).max() <= bound, (plan["off"], want_off, bound)


def test_every_accumulator_fits_32_bits(mpcvr):
    """The device arithmetic is 32-bit: the largest and the most negative accumulator over every accepted matrix x range x format pair and
    every siting (every channel's weighted sum anywhere in [0, W maxin]) must fit int32, from the planned integers."""
    from videorenderer_amd import api
    worst_hi, worst_lo, where = 0, 0, None
    for out_cformat, src_fmt, matrix, rng in PAIRS:
        plan = api.plan_encode(out_cformat, src_fmt, ext(MPEG2, RANGES[rng], MATRICES[matrix]))
        maxin = 1023 if src_fmt == RGB10A2 else 255
        for logw in (2, 3, 4):
            lo, hi = EM.accumulator_range(plan["coef"], plan["off"], plan["shift"], maxin, logw)
            assert -2 ** 31 <= lo and hi <= 2 ** 31 - 1, (out_cformat, src_fmt, matrix, rng, logw, lo, hi)
            if hi > worst_hi:
                worst_hi, where = hi, (out_cformat, src_fmt, matrix, rng, logw)
            worst_lo = min(worst_lo, lo)
    print("largest accumulator %.4g at %s; most negative %.4g" % (worst_hi, where, worst_lo))
    # include/mpcvr.h quotes the largest, 1.07e9: P010 out, top-left siting, full range (8- and 10-bit sources differ in the rounding only)
    assert where[0] == P010 and where[3] == "full" and where[4] == 4 and 1.0e9 < worst_hi < 1.1e9


def test_siting_and_defaults_follow_the_description(mpcvr):
    """The chroma field maps as the convert path reads it for 4:2:0 input (7 top-left, 1 centre, else left); a description without a matrix
    plans as mpcvr_set_input would for a small frame (BT.601, limited range)."""
    from videorenderer_amd import api
    assert api.plan_encode(NV12, BGRA8, ext(COSITED, TV, M709))["siting"] == EM.TOPLEFT
    assert api.plan_encode(NV12, BGRA8, ext(MPEG1, TV, M709))["siting"] == EM.CENTRE
    assert api.plan_encode(NV12, BGRA8, ext(MPEG2, TV, M709))["siting"] == EM.LEFT
    assert api.plan_encode(P010, RGB10A2, ext(0, TV, M709))["siting"] == EM.LEFT
    a, b = api.plan_encode(NV12, BGRA8, 0), api.plan_encode(NV12, BGRA8, ext(MPEG2, TV, M601))
    assert np.array_equal(a["coef"], b["coef"]) and np.array_equal(a["off"], b["off"])
    # BT.709 limited range, 8 bits: the familiar integers (0.2126 * 219 / 255 * 65536 = 11966, 16 * 65536 ...)
    p = api.plan_encode(NV12, BGRA8, ext(MPEG2, TV, M709))
    assert abs(int(p["coef"][0, 0]) - 11966) <= 2 and abs(int(p["off"][0]) - (16 << 16)) <= 600 and abs(int(p["off"][1]) - (128 << 16)) <= 600


def test_refusals(mpcvr):
    """Other output formats — RGB (a description that plans as RGB has nothing to invert towards), gray, YUV layouts that are not NV12 /
    P010, an unknown number — and another source format: MPCVR_E_INVALIDARG.  mpcvr_encode_pass answers its argument checks without a device."""
    from videorenderer_amd import api
    for bad in (30, 26, 37, 38, 14, 3, 0, 99, -1):       # XRGB32, GBRP8, Y8, Y10, YV12, P016, none, unknown
        with pytest.raises(api.MpcvrError) as e:
            api.plan_encode(bad, BGRA8, ext(MPEG2, TV, M709))
        assert e.value.hr == api.E_INVALIDARG, bad
    for bad_src in (2, -1, 8):
        with pytest.raises(api.MpcvrError) as e:
            api.plan_encode(NV12, bad_src, 0)
        assert e.value.hr == api.E_INVALIDARG
    L = api.load_library()
    args = lambda **kw: [kw.get(k, v) for k, v in (("src", 4096), ("sp", 64), ("fmt", 0), ("w", 16), ("h", 4), ("cf", NV12), ("ex", 0),
                                                      ("y", 8192), ("yp", 16), ("uv", 12288), ("uvp", 16), ("stream", None))]
    for kw, hr in ((dict(w=15), api.E_INVALIDARG), (dict(h=3), api.E_INVALIDARG), (dict(w=0), api.E_INVALIDARG), (dict(cf=30), api.E_INVALIDARG),
                   (dict(cf=37), api.E_INVALIDARG), (dict(fmt=2), api.E_INVALIDARG), (dict(y=8194), api.E_INVALIDARG), (dict(yp=18), api.E_INVALIDARG),
                   (dict(uvp=12), api.E_INVALIDARG), (dict(sp=60), api.E_INVALIDARG), (dict(uv=8192 + 48), api.E_INVALIDARG),
                   (dict(y=4096 + 128), api.E_INVALIDARG), (dict(y=None), api.E_POINTER), (dict(uv=None), api.E_POINTER), (dict(src=None), api.E_POINTER)):
        assert L.mpcvr_encode_pass(*args(**kw)) == hr, kw


# ---- closure through the oracle ------------------------------------------------------------------------------------------------------
def block_constant_frame(maxin, seed, blocks_w=16, blocks_h=8):
    """(2 bh, 2 bw, 3) codes, constant over 2x2 blocks: the 8 cube corners, then random codes"""
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, maxin + 1, size=(blocks_h * blocks_w, 3), dtype=np.int64)
    cols[:8] = np.array(list(itertools.product((0, maxin), repeat=3)), dtype=np.int64)
    blocks = cols.reshape(blocks_h, blocks_w, 3)
    return np.repeat(np.repeat(blocks, 2, axis=0), 2, axis=1)


# (label, out_cformat, src_fmt, description, oracle output_format, bound in codes of the target)
# The bound is what this test measures (pytest -s prints it), not a free tolerance.  The decoder sees Y, U and V each rounded to a code of
# a LIMITED-range scale (219 / 224 steps where RGB has 255, 876 / 896 where it has 1023), so each is off by up to half a code and the three
# add up through the matrix row: half a Y code is 0.58 RGB codes, half a Cb code 1.06 (BT.709) / 1.07 (BT.2020nc) codes of blue — 1.65
# codes of blue in the worst case, 1.5 (BT.709) / 1.4 (BT.2020nc) of red, 1.0 of green, whatever the depth, since both sides scale alike.  Rounded to a code:
#   NV12, BT.709 limited, 8 bits -> 8 bits:        measured maximum 2 codes (per channel R 1, G 1, B 2; mean 0.40)
#   P010, BT.2020nc limited, 10 bits -> 10 bits:   measured maximum 2 codes (per channel R 1, G 1, B 2; mean 0.36) — not the <= 1 one might
#     hope for from two more bits: the target's codes are as fine as the sample's, so the ratio is the 8-bit one.
# The test also holds every channel to its own worst case, computed from the matrix (floor(sum_j |M[i][j]| / 2 in target codes + 1 / 2)).
# A wrong matrix, swapped U / V or a wrong offset misses by tens of codes.
CLOSURE = [
    ("nv12_709_limited", NV12, BGRA8, ext(MPEG1, TV, M709), 0, 2),
    ("p010_2020nc_limited", P010, RGB10A2, ext(MPEG1, TV, M2020), 1, 2),
]


@pytest.mark.parametrize("label,out_cformat,src_fmt,exfmt,target,bound", CLOSURE, ids=[c[0] for c in CLOSURE])
def test_model_output_decodes_back_to_the_frame_through_the_oracle(mpcvr, oracle, label, out_cformat, src_fmt, exfmt, target, bound):
    from videorenderer_amd import api
    ten_in = src_fmt == RGB10A2
    maxin = 1023 if ten_in else 255
    rgb = block_constant_frame(maxin, seed=5 + out_cformat)
    h, w, _ = rgb.shape
    plan = api.plan_encode(out_cformat, src_fmt, exfmt)
    assert plan["siting"] == EM.CENTRE
    y, uv = EM.encode420(EM.pack_rgb(rgb, src_fmt, alpha=255), src_fmt, out_cformat == P010, plan["coef"], plan["off"], plan["shift"], plan["siting"])
    frame = np.concatenate([y.reshape(-1).view(np.uint8), uv.reshape(-1).view(np.uint8)])
    nbytes, pitch = oracle.frame_bytes(out_cformat, w, h)
    assert nbytes == frame.size and pitch == w * (2 if out_cformat == P010 else 1)
    p = oracle.default_params(cformat=out_cformat, width=w, height=h, exfmt=exfmt, window_w=w, window_h=h, video_rect=(0, 0, w, h),
                              iChromaScaling=0, bUseDither=0, output_format=target)
    out = oracle.process(p, frame, pitch)
    back = EM.unpack_rgb(out.view(np.uint32)[..., 0], target)
    diff = np.abs(back - rgb)
    print(label, "closure: max |difference| =", diff.max(), "codes; per channel", diff.reshape(-1, 3).max(0), "; mean", diff.mean())
    assert diff.max() <= bound, (label, diff.max())
    cm, _ = api.plan_color_matrix(out_cformat, w, h, exfmt)
    T, _ = scales(out_cformat, src_fmt)
    maxt = 1023 if target else 255
    # (+ 0.03: the 2^-16 rounding of the coefficients, under 0.02 code, and the oracle's fp32)
    per_channel = np.floor(np.abs(np.array(cm[:9], dtype=np.float64).reshape(3, 3)).sum(1) * 0.5 / T * maxt + 0.5 + 0.03)
    print(label, "worst case per channel", per_channel)
    assert (diff.reshape(-1, 3).max(0) <= per_channel).all() and per_channel.max() <= bound, (diff.reshape(-1, 3).max(0), per_channel)
