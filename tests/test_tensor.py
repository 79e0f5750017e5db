"""The tensor extension on the CPU (include/mpcvr.h: mpcvr_plan_tensor_value, mpcvr_plan_batch_tensor, and every refusal of
mpcvr_tensor_pass that is answered before a launch), against the model (tests/tensor_model.py).  Everything is bits: no tolerance
anywhere.  The kernel itself: tests/test_tensor_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests import tensor_model as TM

BGRA8, RGB10A2 = TM.BGRA8, TM.RGB10A2
F32 = np.float32
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (scale, bias) rows; every row runs over all 256 and all 1024 codes and the three dtypes.  What each is there for is checked by name below.
FACTORS = {
    "unit_interval": (1 / 255, 0.0),
    "imagenet_r": (1 / (255 * IMAGENET_STD[0]), -IMAGENET_MEAN[0] / IMAGENET_STD[0]),
    "imagenet_g": (1 / (255 * IMAGENET_STD[1]), -IMAGENET_MEAN[1] / IMAGENET_STD[1]),
    "imagenet_b": (1 / (255 * IMAGENET_STD[2]), -IMAGENET_MEAN[2] / IMAGENET_STD[2]),
    "codes_as_they_are": (1.0, 0.0),                  # 10-bit codes: bf16 ties (257 -> 256, 259 -> 260)
    "times_3": (3.0, 0.0),                            # fp16 ties: 683 * 3 = 2049 -> 2048, 685 * 3 = 2055 -> 2056
    "times_100": (100.0, 0.0),                        # fp16 overflow: 655 * 100 -> 65504, 656 * 100 -> inf
    "two_to_minus_20": (2.0 ** -20, 0.0),             # fp16 subnormals, exact: codes below 64
    "two_to_minus_26": (2.0 ** -26, 0.0),             # fp16 subnormals with ties: 2 -> 0, 6 -> 2 units of 2^-24
    "negative": (-1 / 255, 1.0),
    "negative_times_3": (-3.0, 0.0),
    "negative_times_100": (-100.0, 0.0),
    "cancelling_exactly": (0.5, -64.0),               # code 128 -> +0
    "cancelling_a_rounded_product": (1 / 255, -float(F32(100) * F32(1 / 255))),     # code 100 -> +0, its neighbours a few ulps of the product
    "zero_scale": (0.0, 0.5),
    "smallest_factors": (2.0 ** -100, -(2.0 ** -100)),
    "largest_factors": (2.0 ** 100, 2.0 ** 100),
}


def _all_bits(dtype, fmt, scale, bias):
    from videorenderer_amd import api
    n = 1024 if fmt == RGB10A2 else 256
    return np.array([api.plan_tensor_value(dtype, fmt, c, scale, bias) for c in range(n)], dtype=np.uint32)


@pytest.mark.parametrize("label", list(FACTORS))
@pytest.mark.parametrize("dtype", [TM.F32, TM.F16, TM.BF16])
@pytest.mark.parametrize("fmt", [BGRA8, RGB10A2])
def test_plan_tensor_value_equals_the_model_on_every_code(mpcvr, fmt, dtype, label):
    scale, bias = FACTORS[label]
    got = _all_bits(dtype, fmt, scale, bias)
    want = TM.element_bits(np.arange(got.size), scale, bias, dtype).astype(np.uint32)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{label}: {bad.size} codes differ, first {bad[0]}: got {got[bad[0]]:#x}, model {want[bad[0]]:#x}"


def _f16(x):
    return int(np.float16(x).view(np.uint16))


def test_the_rounding_rows_hold_what_they_are_there_for(mpcvr):
    """the ties, the overflow and the subnormals named in FACTORS, as literal bits (the model agrees by the test above)"""
    from videorenderer_amd import api
    v = api.plan_tensor_value
    # bf16 keeps 8 significant bits: 257 = 0x101 and 259 = 0x103 are ties at 9 bits
    assert v(TM.BF16, RGB10A2, 257, 1.0, 0.0) == F32(256).view(np.uint32) >> 16
    assert v(TM.BF16, RGB10A2, 259, 1.0, 0.0) == F32(260).view(np.uint32) >> 16
    assert v(TM.BF16, RGB10A2, 258, 1.0, 0.0) == F32(258).view(np.uint32) >> 16
    # fp16 keeps 11: 2049 and 2055 are ties at 12
    assert v(TM.F16, RGB10A2, 683, 3.0, 0.0) == _f16(2048) and v(TM.F16, RGB10A2, 685, 3.0, 0.0) == _f16(2056)
    assert v(TM.F16, RGB10A2, 655, 100.0, 0.0) == 0x7bff and v(TM.F16, RGB10A2, 656, 100.0, 0.0) == 0x7c00
    assert v(TM.F16, RGB10A2, 656, -100.0, 0.0) == 0xfc00
    assert v(TM.F32, RGB10A2, 656, 100.0, 0.0) == F32(65600).view(np.uint32)
    # subnormals: c * 2^-20 = 16 c units of 2^-24; c * 2^-26 = c / 4 units, ties to even
    assert [v(TM.F16, BGRA8, c, 2.0 ** -20, 0.0) for c in (1, 63, 64)] == [16, 1008, 0x0400]
    assert [v(TM.F16, BGRA8, c, 2.0 ** -26, 0.0) for c in (1, 2, 3, 5, 6, 7, 10)] == [0, 0, 1, 1, 2, 2, 2]
    # two roundings, not one: 1 / 255 rounded to fp32 times 255 is exactly 1, and code 100 cancels to +0
    assert v(TM.F32, BGRA8, 255, 1 / 255, 0.0) == F32(1).view(np.uint32)
    assert v(TM.F32, BGRA8, 100, *FACTORS["cancelling_a_rounded_product"]) == 0
    assert v(TM.F32, BGRA8, 128, 0.5, -64.0) == 0


def test_two_roundings_differ_from_a_fused_multiply_add_somewhere():
    """the table would not notice a contracted multiply-add if no row's product needed rounding before the add: at least one code of the
    ImageNet rows gives other bits when the product is kept exact (the model in float64, rounded once)"""
    differ = 0
    for label in ("imagenet_r", "imagenet_g", "imagenet_b", "cancelling_a_rounded_product"):
        scale, bias = FACTORS[label]
        c = np.arange(1024)
        two = TM.element_bits(c, scale, bias, TM.F32)
        fused = (c.astype(np.float64) * np.float64(F32(scale)) + np.float64(F32(bias))).astype(np.float32).view(np.uint32)     # exact product (34 bits), one rounding
        differ += int((two != fused).sum())
    assert differ > 0


BAD_FACTORS = [float("inf"), float("-inf"), float("nan"), 2.0 ** 101, -(2.0 ** 101), 2.0 ** -101, -(2.0 ** -101), 2.0 ** -140, float(np.nextafter(F32(2.0 ** 100), F32(np.inf))),
               float(np.nextafter(F32(2.0 ** -100), F32(0)))]


@pytest.mark.parametrize("bad", BAD_FACTORS)
def test_plan_tensor_value_refuses_factors_outside_the_set(mpcvr, bad):
    from videorenderer_amd import api
    L = api.load_library()
    bits = C.c_uint32(0xdeadbeef)
    assert L.mpcvr_plan_tensor_value(TM.F32, BGRA8, 1, bad, 0.0, C.byref(bits)) == api.E_INVALIDARG
    assert L.mpcvr_plan_tensor_value(TM.F32, BGRA8, 1, 1.0, bad, C.byref(bits)) == api.E_INVALIDARG
    assert bits.value == 0xdeadbeef


def test_plan_tensor_value_accepts_the_ends_of_the_set_and_refuses_the_rest(mpcvr):
    from videorenderer_amd import api
    L = api.load_library()
    bits = C.c_uint32()
    for ok in (2.0 ** 100, -(2.0 ** 100), 2.0 ** -100, -(2.0 ** -100), 0.0, -0.0):
        assert L.mpcvr_plan_tensor_value(TM.F32, BGRA8, 1, ok, ok, C.byref(bits)) == 0
    assert L.mpcvr_plan_tensor_value(TM.F32, BGRA8, 1, 1.0, 0.0, None) == api.E_POINTER
    for dtype, fmt, code in ((3, BGRA8, 0), (-1, BGRA8, 0), (TM.F32, 2, 0), (TM.F32, -1, 0), (TM.F32, BGRA8, 256), (TM.F32, RGB10A2, 1024)):
        assert L.mpcvr_plan_tensor_value(dtype, fmt, code, 1.0, 0.0, C.byref(bits)) == api.E_INVALIDARG
    assert L.mpcvr_plan_tensor_value(TM.F32, RGB10A2, 1023, 1.0, 0.0, C.byref(bits)) == 0 and bits.value == F32(1023).view(np.uint32)


def _formulas(w, h, n, budget):
    budget = budget or (4 << 30)
    pitch = (4 * w + 15) & ~15
    stride = (pitch * h + 255) & ~255
    fpc = min(max(budget // stride, 1), n)
    return dict(surface_pitch=pitch, frame_stride=stride, frames_per_chunk=fpc, chunks=-(-n // fpc))


@pytest.mark.parametrize("w,h,n,budget", [(1, 1, 1, 0), (3, 5, 7, 0), (1919, 1079, 32, 0), (1920, 1080, 32, 0), (7680, 4320, 32, 1 << 30), (7681, 4321, 33, 1 << 30),
                                          (32768, 32768, 3, 0), (32767, 1, 5, 1), (641, 361, 8, 3 * ((641 * 4 + 15 & ~15) * 361 + 255 & ~255))])
def test_plan_batch_tensor_is_the_three_formulas_for_any_parity(mpcvr, w, h, n, budget):
    from videorenderer_amd import api
    got = api.plan_batch_tensor(w, h, n, budget)
    assert got == _formulas(w, h, n, budget)
    if not (w | h) & 1:
        assert got == api.plan_batch_yuv(w, h, n, budget)


def test_plan_batch_tensor_refusals_and_plan_batch_yuv_as_it_was(mpcvr):
    from videorenderer_amd import api
    L = api.load_library()
    for w, h, n in ((0, 4, 1), (4, 0, 1), (32769, 4, 1), (4, 32769, 1), (4, 4, 0), (4, 4, -1), (-2, 4, 1)):
        assert L.mpcvr_plan_batch_tensor(w, h, n, 0, None, None, None, None) == api.E_INVALIDARG
    assert L.mpcvr_plan_batch_tensor(5, 3, 2, 0, None, None, None, None) == 0      # any out pointer may be NULL
    for w, h in ((5, 4), (4, 5), (1, 1)):                  # the evenness condition stays where it was
        assert L.mpcvr_plan_batch_yuv(w, h, 1, 0, None, None, None, None) == api.E_INVALIDARG


# ---- the refusals of mpcvr_tensor_pass that are answered before anything is launched: no GPU needed, the pointers are never followed ----
SRC, DST = 0x10000000, 0x20000000
W, H = 64, 32


def _desc(dtype=TM.F32, layout=TM.PLANAR, order=TM.RGB, row_pitch=None, plane_pitch=None, scale=(1 / 255,) * 3, bias=(0.0,) * 3, reserved=0):
    from videorenderer_amd import api
    es = TM.ELEMENT_SIZE.get(dtype, 4)
    if row_pitch is None:
        row_pitch = W * es * (1 if layout == TM.PLANAR else 3)
    if plane_pitch is None:
        plane_pitch = row_pitch * H
    d = api.tensor_desc(dtype, layout, row_pitch, plane_pitch, scale, bias, order)
    d.reserved = reserved
    return d


def _pass(desc, src=SRC, src_pitch=4 * W, fmt=BGRA8, w=W, h=H, dst=DST):
    from videorenderer_amd import api
    return api.load_library().mpcvr_tensor_pass(C.c_void_p(src), src_pitch, fmt, w, h, C.byref(desc) if desc is not None else None, C.c_void_p(dst), None)


def test_tensor_pass_null_pointers(mpcvr):
    from videorenderer_amd import api
    assert _pass(_desc(), src=0) == api.E_POINTER
    assert _pass(_desc(), dst=0) == api.E_POINTER
    assert _pass(None) == api.E_POINTER
    L = api.load_library()
    assert L.mpcvr_render_tensor(None, 0, C.byref(_desc()), C.c_void_p(DST)) == api.E_POINTER
    assert L.mpcvr_process_batch_tensor(None, 1, None, C.byref(_desc()), None) == api.E_POINTER


REFUSED = {
    "another_source_format": dict(fmt=2),
    "width_0": dict(w=0),
    "height_0": dict(h=0),
    "width_32769": dict(w=32769, src_pitch=4 * 32769 + 12),
    "height_32769": dict(h=32769),
    "source_pitch_below_a_row": dict(src_pitch=4 * W - 4),
    "source_off_4": dict(src=SRC + 2),
    "source_pitch_off_4": dict(src_pitch=4 * W + 2),
    "dtype_3": dict(desc=dict(dtype=3)),
    "dtype_negative": dict(desc=dict(dtype=-1)),
    "layout_2": dict(desc=dict(layout=2)),
    "channel_order_2": dict(desc=dict(order=2)),
    "reserved_set": dict(desc=dict(reserved=1)),
    "scale_inf": dict(desc=dict(scale=(1.0, float("inf"), 1.0))),
    "scale_nan": dict(desc=dict(scale=(float("nan"), 1.0, 1.0))),
    "scale_2_101": dict(desc=dict(scale=(1.0, 1.0, 2.0 ** 101))),
    "scale_2_minus_101": dict(desc=dict(scale=(2.0 ** -101, 1.0, 1.0))),
    "bias_inf": dict(desc=dict(bias=(0.0, 0.0, float("-inf")))),
    "bias_nan": dict(desc=dict(bias=(0.0, float("nan"), 0.0))),
    "bias_2_101": dict(desc=dict(bias=(-(2.0 ** 101), 0.0, 0.0))),
    "bias_2_minus_101": dict(desc=dict(bias=(0.0, 2.0 ** -101, 0.0))),
    "planar_row_pitch_below_a_row": dict(desc=dict(row_pitch=4 * W - 4)),
    "interleaved_row_pitch_below_a_row": dict(desc=dict(layout=TM.INTERLEAVED, row_pitch=12 * W - 4)),
    "interleaved_fp16_row_pitch_of_a_planar_row": dict(desc=dict(dtype=TM.F16, layout=TM.INTERLEAVED, row_pitch=2 * W)),
    "row_pitch_0": dict(desc=dict(row_pitch=0)),
    "row_pitch_negative": dict(desc=dict(row_pitch=-4 * W)),
    "row_pitch_beyond_2_47": dict(desc=dict(row_pitch=(1 << 47) + 4)),
    "plane_pitch_0": dict(desc=dict(plane_pitch=0)),
    "plane_pitch_negative": dict(desc=dict(plane_pitch=-4 * W * H)),
    "plane_pitch_beyond_2_47": dict(desc=dict(plane_pitch=(1 << 47) + 4)),
    "fp32_tensor_off_4": dict(dst=DST + 2),
    "fp16_tensor_off_2": dict(dst=DST + 1, desc=dict(dtype=TM.F16)),
    "fp32_row_pitch_off_4": dict(desc=dict(row_pitch=4 * W + 2)),
    "bf16_row_pitch_off_2": dict(desc=dict(dtype=TM.BF16, row_pitch=2 * W + 1)),
    "fp32_plane_pitch_off_4": dict(desc=dict(plane_pitch=4 * W * H + 2)),
    "planes_overlap_by_one_element": dict(desc=dict(plane_pitch=4 * W * H - 4)),
    "planes_interleave_row_by_row": dict(desc=dict(row_pitch=12 * W, plane_pitch=4 * W)),
    "first_plane_ends_inside_the_source": dict(dst=SRC - 4 * W * H + 4),
    "third_plane_on_the_source": dict(dst=SRC - 2 * 4 * W * H),
    "interleaved_tensor_over_the_source": dict(dst=SRC + 4, desc=dict(layout=TM.INTERLEAVED)),
}


@pytest.mark.parametrize("label", list(REFUSED))
def test_tensor_pass_refuses_before_any_launch(mpcvr, label):
    from videorenderer_amd import api
    kw = dict(REFUSED[label])
    desc = _desc(**kw.pop("desc", {}))
    assert _pass(desc, **kw) == api.E_INVALIDARG
