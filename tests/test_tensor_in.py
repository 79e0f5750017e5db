"""The sample pass on the CPU (include/mpcvr.h: mpcvr_plan_sample_code, mpcvr_plan_batch_from_tensors, and every refusal of
mpcvr_sample_pass that is answered before a launch), against the model (tests/tensor_in_model.py).  Everything is bits: no tolerance
anywhere.  The kernel itself: tests/test_tensor_in_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests import tensor_in_cases as K
from tests import tensor_in_model as M

E_POINTER, E_INVALIDARG = -2147467261, -2147024809          # 0x80004003, 0x80070057


def _host_codes(dtype, cformat, element_bits, scale, bias):
    """mpcvr_plan_sample_code over an array of element bits"""
    from videorenderer_amd import api
    f, out = api.load_library().mpcvr_plan_sample_code, C.c_uint32()
    ref, s, b = C.byref(out), float(scale), float(bias)
    got = np.empty(len(element_bits), dtype=np.uint32)
    for i, e in enumerate(np.asarray(element_bits).tolist()):
        hr = f(dtype, cformat, e, s, b, ref)
        assert hr == 0, (hr, e)
        got[i] = out.value
    return got


def _factor_pairs(cformat):
    """(label, scale, bias): the identity factors and the three pairs of the ImageNet triple"""
    (s0, _, _), (b0, _, _) = K.identity_factors(cformat)
    s, b = K.imagenet_factors(cformat)
    return [("identity", s0, b0)] + [("imagenet_" + "rgb"[k], s[k], b[k]) for k in range(3)]


def _compare(dtype, cformat, element_bits, scale, bias, what):
    got = _host_codes(dtype, cformat, element_bits, scale, bias)
    want = M.code(element_bits, dtype, cformat, scale, bias)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first bits {int(element_bits[bad[0]]):#x}: got {got[bad[0]]}, model {want[bad[0]]}"
    assert int(got.max()) <= M.MAXCODE[cformat]


@pytest.mark.parametrize("cformat", K.FORMATS)
@pytest.mark.parametrize("dtype", [M.F16, M.BF16])
def test_plan_sample_code_equals_the_model_on_every_16_bit_pattern(mpcvr, dtype, cformat):
    every = np.arange(1 << 16, dtype=np.uint32)
    for label, scale, bias in _factor_pairs(cformat):
        _compare(dtype, cformat, every, scale, bias, label)


@pytest.mark.parametrize("cformat", K.FORMATS)
def test_plan_sample_code_equals_the_model_on_random_fp32_patterns(mpcvr, cformat):
    """2^18 raw patterns (every exponent, NaNs and infinities among them) and as many values whose codes fall inside the format"""
    rng = np.random.default_rng(7)
    raw = rng.integers(0, 1 << 32, size=1 << 18, dtype=np.uint64).astype(np.uint32)
    for label, scale, bias in _factor_pairs(cformat):
        _compare(M.F32, cformat, raw, scale, bias, label + ", raw patterns")
    inside = (rng.random(1 << 16, dtype=np.float32) * np.float32(1.25) - np.float32(0.125)).view(np.uint32)
    for label, scale, bias in _factor_pairs(cformat):
        _compare(M.F32, cformat, inside, scale, bias, label + ", values around [0, 1]")


@pytest.mark.parametrize("cformat", K.FORMATS)
def test_plan_sample_code_on_the_named_rows(mpcvr, cformat):
    from videorenderer_amd import api
    m = M.MAXCODE[cformat]
    for name, b in K.named_rows(cformat):
        got, want = api.plan_sample_code(M.F32, cformat, b, 1.0, 0.0), int(M.code(np.uint32(b), M.F32, cformat, 1.0, 0.0))
        assert got == want, f"{name}: got {got}, model {want}"
    for name, b, scale, bias in K.FACTOR_ROWS:
        got, want = api.plan_sample_code(M.F32, cformat, b, scale, bias), int(M.code(np.uint32(b), M.F32, cformat, scale, bias))
        assert got == want, f"{name}: got {got}, model {want}"
    # ... and what the rows are there for, as literal codes
    v = lambda x, scale=1.0, bias=0.0: api.plan_sample_code(M.F32, cformat, K.bits(x), scale, bias)
    assert [v(0.5), v(1.5), v(2.5), v(3.5)] == [0, 2, 2, 4]                      # ties to even
    # maxcode is odd: maxcode - 0.5 is a tie that goes DOWN to the even maxcode - 1, and so does maxcode - 1.5, going up
    assert v(m - 0.5) == m - 1 and v(m - 1.5) == m - 1 and v(m - 2.5) == m - 3 and v(m) == m and v(m + 0.5) == m and v(float(np.nextafter(np.float32(m - 0.5), np.float32(m)))) == m
    assert v(np.inf) == m and v(-np.inf) == 0 and v(np.nan) == 0 and v(3.4028235e38) == m and v(-3.4028235e38) == 0
    assert v(np.inf, 0.0, 7.0) == 0 and v(123.0, 0.0, 7.0) == 7                   # inf * 0 is NaN
    assert api.plan_sample_code(M.F32, cformat, 0x007fffff, 2.0 ** 100, 3.0) == 3   # a subnormal element is +0
    assert v(0.0, 1.0, 12.5) == 12 and v(-100.5, -1.0) == 100
    # fp16 subnormals are kept: 2^-24 * 2^24 = 1; bf16 is the top half of fp32
    assert api.plan_sample_code(M.F16, cformat, 0x0001, 2.0 ** 24, 0.0) == 1 and api.plan_sample_code(M.F16, cformat, 0x03ff, 2.0 ** 24, 0.0) == min(1023, m)
    assert api.plan_sample_code(M.BF16, cformat, 0x3f80, 9.0, 0.0) == 9 and api.plan_sample_code(M.BF16, cformat, 0x0040, 2.0 ** 100, 5.0) == 5


def test_a_fused_multiply_add_would_show(mpcvr):
    """The ImageNet factors at GBRP16 tell two roundings from one: on at least 16 of 2^20 random elements an exactly evaluated fused
    multiply-add gives another code — and the host function gives the two-rounding code on every one of them.  (A condition, not a
    measurement: the same elements go through the kernel in tests/test_tensor_in_gpu.py.)"""
    rows = K.fma_sensitive()
    print(f"elements where a fused multiply-add differs: {len(rows)} of {1 << 20}")
    assert len(rows) >= 16
    from videorenderer_amd import api
    scale, bias = K.imagenet_factors(M.GBRP16)
    for b, ch, two, fma in rows:
        assert abs(two - fma) == 1
        assert api.plan_sample_code(M.F32, M.GBRP16, b, scale[ch], bias[ch]) == two, f"element {b:#x} channel {ch}: two roundings {two}, fused {fma}"


def test_plan_sample_code_refusals(mpcvr):
    from videorenderer_amd import api
    f, out = api.load_library().mpcvr_plan_sample_code, C.c_uint32()
    assert f(M.F32, M.GBRP8, 0, 1.0, 0.0, None) == E_POINTER
    for bad in [(3, M.GBRP8, 0, 1.0, 0.0), (-1, M.GBRP8, 0, 1.0, 0.0), (M.F32, 25, 0, 1.0, 0.0), (M.F32, 29, 0, 1.0, 0.0), (M.F32, 0, 0, 1.0, 0.0),
                (M.F16, M.GBRP8, 0x10000, 1.0, 0.0), (M.BF16, M.GBRP16, 0x10000, 1.0, 0.0),
                (M.F32, M.GBRP8, 0, float("inf"), 0.0), (M.F32, M.GBRP8, 0, float("nan"), 0.0), (M.F32, M.GBRP8, 0, 1.0, float("inf")),
                (M.F32, M.GBRP8, 0, 2.0 ** -101, 0.0), (M.F32, M.GBRP8, 0, 1.0, 2.0 ** 101), (M.F32, M.GBRP8, 0, 1.0, -(2.0 ** -101))]:
        assert f(*bad, C.byref(out)) == E_INVALIDARG, bad
    assert f(M.F32, M.GBRP8, 0, 2.0 ** -100, -(2.0 ** 100), C.byref(out)) == 0


T, S = 0x10000000, 0x20000000          # a tensor and a sample far apart: the refusals come before any launch, nothing is dereferenced


def _pass(tensor=T, dtype=M.F16, layout=M.PLANAR, order=M.RGB, reserved=0, row_pitch=None, plane_pitch=None, scale=(255.0,) * 3, bias=(0.0,) * 3,
          w=16, h=8, cformat=M.GBRP8, sample=S, pitch=None, desc=True):
    from videorenderer_amd import api
    es = M.ELEMENT_SIZE.get(dtype, 2)
    if row_pitch is None:
        row_pitch = w * es * (3 if layout == M.INTERLEAVED else 1)
    if plane_pitch is None:
        plane_pitch = row_pitch * h
    if pitch is None:
        pitch = w * M.BYTES.get(cformat, 1)
    d = api.tensor_desc(dtype, layout, row_pitch, plane_pitch, scale, bias, order)
    d.reserved = reserved
    return api.load_library().mpcvr_sample_pass(C.c_void_p(tensor), C.byref(d) if desc else None, w, h, cformat, C.c_void_p(sample), pitch, None)


def test_sample_pass_refusals(mpcvr):
    assert _pass(tensor=None) == E_POINTER and _pass(sample=None) == E_POINTER and _pass(desc=False) == E_POINTER
    bad = dict(
        cformat_nv12=dict(cformat=0), cformat_beyond=dict(cformat=29), dtype=dict(dtype=3), layout=dict(layout=2), order=dict(order=2), reserved=dict(reserved=1),
        w_zero=dict(w=0), h_zero=dict(h=0), w_large=dict(w=32769, row_pitch=1 << 20, pitch=1 << 20), h_large=dict(h=32769),
        tensor_odd=dict(tensor=T + 1), tensor_f32_on_2=dict(dtype=M.F32, tensor=T + 2), row_pitch_odd=dict(row_pitch=33), plane_pitch_odd=dict(plane_pitch=257),
        row_pitch_small=dict(row_pitch=30), row_pitch_small_hwc=dict(layout=M.INTERLEAVED, row_pitch=94), row_pitch_huge=dict(row_pitch=(1 << 47) + 2),
        plane_pitch_zero=dict(plane_pitch=0), plane_pitch_negative=dict(plane_pitch=-256), plane_pitch_huge=dict(plane_pitch=(1 << 47) + 2),
        sample_odd=dict(cformat=M.GBRP16, sample=S + 1), pitch_small=dict(pitch=15), pitch_small_16=dict(cformat=M.GBRP10, pitch=30), pitch_odd_16=dict(cformat=M.GBRP16, pitch=33),
        scale_inf=dict(scale=(255.0, float("inf"), 255.0)), bias_nan=dict(bias=(0.0, 0.0, float("nan"))), scale_tiny=dict(scale=(2.0 ** -101, 1.0, 1.0)), bias_huge=dict(bias=(0.0, 2.0 ** 101, 0.0)),
        tensor_in_sample=dict(tensor=S + 64), sample_in_tensor=dict(sample=T + 2 * 16 * 8 * 2), last_byte_shared=dict(sample=T + 3 * 16 * 8 * 2 - 1),
        tensor_behind_last_plane=dict(tensor=S + 3 * 16 * 8 - 2),
    )
    for name, kw in bad.items():
        assert _pass(**kw) == E_INVALIDARG, name


def test_batch_surface_integers(mpcvr):
    """frame_stride = 3 pitch h rounded up to 256; a chunk is what fits the budget, at least one frame, at most n"""
    from videorenderer_amd import api
    default = 4 << 30
    for pitch, h, n, budget in [(32, 16, 5, 0), (32, 16, 5, 2 * 1536), (32, 16, 5, 2 * 1536 + 1535), (32, 16, 5, 1), (32, 16, 1, 1536), (34, 15, 3, 2 * 1536),
                                (3840 * 2, 2160, 32, 0), (7680 * 2, 4320, 32, 0), (7680 * 2, 4320, 32, 1 << 30), (1, 1, 7, 0), (1, 1, 7, 512), (65536, 32768, 3, 0)]:
        got = api.plan_batch_from_tensors(pitch, h, n, budget)
        stride = (3 * pitch * h + 255) // 256 * 256
        fpc = max(1, min(n, (budget or default) // stride))
        assert got == dict(frame_stride=stride, frames_per_chunk=fpc, chunks=-(-n // fpc)), (pitch, h, n, budget, got)
    assert api.plan_batch_from_tensors(32, 16, 5, 2 * 1536) == dict(frame_stride=1536, frames_per_chunk=2, chunks=3)
    L = api.load_library()
    for bad in [(0, 16, 5), (32, 0, 5), (32, 16, 0), (32, 32769, 1), (-32, 16, 1)]:
        assert L.mpcvr_plan_batch_from_tensors(*bad, 0, None, None, None) == E_INVALIDARG, bad
