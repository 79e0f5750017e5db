"""The measure extension's host functions (include/mpcvr.h: mpcvr_light_level_from_histogram, mpcvr_histogram_percentile) on the CPU, against
the model (tests/measure_model.py), whose nits are evaluated in np.longdouble.  The kernel itself: tests/test_measure_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests import measure_model as MM

BGRA8, RGB10A2 = MM.BGRA8, MM.RGB10A2
# Measured, not fixed in advance: numpy's double evaluation of L(c) against the same formula in 80-bit np.longdouble, over all 1024 ten-bit
# and all 256 eight-bit codes, differs by at most 9.8e-14 relative (the cancellation in v^(1/m2) - c1 at small codes amplifies pow's last
# ulp about 500x; test_double_evaluation_of_the_eotf_against_long_double prints the figure).  The bar is 100x that, so that another libm's
# pow stays inside it.
NITS_RTOL = 1e-11


def _hist(pairs):
    h = np.zeros(MM.BINS, dtype=np.uint32)
    for c, n in pairs:
        h[c] = n
    return h


def _random_hist(seed, top, bins=MM.BINS):
    rng = np.random.default_rng(seed)
    h = np.zeros(MM.BINS, dtype=np.uint32)
    h[:bins] = rng.integers(0, top + 1, size=bins, dtype=np.uint64).astype(np.uint32)
    h[:bins][rng.random(bins) < 0.3] = 0
    return h


HISTOGRAMS = {
    "empty": (_hist([]), RGB10A2),
    "one_bin_at_0": (_hist([(0, 77)]), RGB10A2),
    "one_bin_at_maxin": (_hist([(1023, 5)]), RGB10A2),
    "two_bins": (_hist([(64, 1000), (940, 3)]), RGB10A2),
    "random_up_to_2_30": (_random_hist(1, 2 ** 30), RGB10A2),
    "random_small": (_random_hist(2, 50), RGB10A2),
    "bgra8_random": (_random_hist(3, 2 ** 20, bins=256), BGRA8),
    "bgra8_one_bin_at_maxin": (_hist([(255, 9)]), BGRA8),
}


def close(got, want):
    want = float(want)
    return got == want if want == 0.0 else abs(got - want) <= NITS_RTOL * abs(want)


@pytest.mark.parametrize("label", list(HISTOGRAMS))
def test_light_level_equals_the_model(mpcvr, label):
    from videorenderer_amd import api
    h, fmt = HISTOGRAMS[label]
    got = api.light_level_from_histogram(h, fmt)
    want = MM.light_level(h, fmt)
    assert (got["pixels"], got["min_code"], got["max_code"]) == (want["pixels"], want["min_code"], want["max_code"])
    print(label, "max_nits", got["max_nits"], "model", float(want["max_nits"]), "avg_nits", got["avg_nits"], "model", float(want["avg_nits"]))
    assert close(got["max_nits"], want["max_nits"]) and close(got["avg_nits"], want["avg_nits"]), (got, want)
    if not want["pixels"]:
        assert got["max_nits"] == 0.0 and got["avg_nits"] == 0.0 and got["min_code"] == -1 and got["max_code"] == -1


@pytest.mark.parametrize("fmt", [BGRA8, RGB10A2], ids=["bgra8", "rgb10a2"])
def test_the_eotf_of_every_code(mpcvr, fmt):
    """L(c) through the library (a histogram with the one bin c: max_nits = avg_nits = L(c)) against the long-double model for every code;
    L(0) == 0, L(maxin) == 10000 to the bar, L non-decreasing."""
    from videorenderer_amd import api
    top = MM.maxin(fmt)
    want = MM.pq_nits(np.arange(top + 1), fmt)
    got = np.zeros(top + 1)
    for c in range(top + 1):
        ll = api.light_level_from_histogram(_hist([(c, 1)]), fmt)
        assert ll["max_nits"] == ll["avg_nits"] and ll["min_code"] == ll["max_code"] == c and ll["pixels"] == 1
        got[c] = ll["max_nits"]
    rel = np.abs(got[1:] - want[1:].astype(np.float64)) / want[1:].astype(np.float64)
    print("L(c), library against long double: largest relative difference", rel.max(), "at code", 1 + int(rel.argmax()))
    assert rel.max() <= NITS_RTOL
    assert got[0] == 0.0 and abs(got[top] - 10000.0) <= NITS_RTOL * 10000.0
    assert (np.diff(got) >= 0).all()


def test_double_evaluation_of_the_eotf_against_long_double():
    """where NITS_RTOL comes from: the model's own formula in double against long double, over every code of both formats"""
    worst = 0.0
    for fmt in (BGRA8, RGB10A2):
        codes = np.arange(1, MM.maxin(fmt) + 1)
        d, ld = MM.pq_nits(codes, fmt, np.float64), MM.pq_nits(codes, fmt, np.longdouble)
        worst = max(worst, float((np.abs(d - ld) / ld).max()))
    print("double against long double: largest relative difference", worst)
    assert worst <= NITS_RTOL


def _percentile_cases():
    out = []
    # 1 000 000 texels: every ppm is a whole count, so cumulative counts land exactly on thresholds
    h = _hist([(10, 1), (20, 499999), (30, 1), (40, 499998), (50, 1)])
    for ppm in (1, 2, 500000, 500001, 999999, 1000000):
        out.append(("exact_1M", h, ppm))
    # 3 texels: ceil(ppm * 3 / 10^6)
    h3 = _hist([(5, 1), (6, 1), (1023, 1)])
    for ppm in (1, 333333, 333334, 500000, 666666, 666667, 999999, 1000000):
        out.append(("three", h3, ppm))
    # counts near 2^30 in many bins: the products need 64 bits
    big = _random_hist(4, 2 ** 30)
    for ppm in (1, 500000, 999999, 1000000):
        out.append(("big", big, ppm))
    # the cumulative count exactly on the threshold, and one short of it
    on = _hist([(100, 500000), (200, 500000)])
    short = _hist([(100, 499999), (200, 500001)])
    out += [("on_threshold", on, 500000), ("one_short", short, 500000), ("on_threshold", on, 500001)]
    return out


@pytest.mark.parametrize("label,h,ppm", _percentile_cases(), ids=["%s-%d" % (l, p) for l, _, p in _percentile_cases()])
def test_percentile_equals_the_model(mpcvr, label, h, ppm):
    from videorenderer_amd import api
    assert api.histogram_percentile(h, ppm) == MM.percentile(h, ppm)


def test_percentile_landmarks(mpcvr):
    from videorenderer_amd import api
    on = _hist([(100, 500000), (200, 500000)])
    short = _hist([(100, 499999), (200, 500001)])
    assert api.histogram_percentile(on, 500000) == 100 and api.histogram_percentile(on, 500001) == 200
    assert api.histogram_percentile(short, 500000) == 200
    assert api.histogram_percentile(on, 1) == 100 and api.histogram_percentile(on, 1000000) == 200


def test_refusals_of_the_host_functions(mpcvr):
    from videorenderer_amd import api
    L = api.load_library()
    h = _hist([(7, 1)])
    hp = C.c_void_p(h.ctypes.data)
    out = api.LightLevel()
    out.pixels, out.max_code = 123, 45
    code = C.c_int32(-7)
    assert L.mpcvr_light_level_from_histogram(None, RGB10A2, C.byref(out)) == api.E_POINTER
    assert L.mpcvr_light_level_from_histogram(hp, RGB10A2, None) == api.E_POINTER
    for fmt in (-1, 2, 30):
        assert L.mpcvr_light_level_from_histogram(hp, fmt, C.byref(out)) == api.E_INVALIDARG
    assert (out.pixels, out.max_code) == (123, 45), "a refusal wrote the result"
    assert L.mpcvr_histogram_percentile(None, 5, C.byref(code)) == api.E_POINTER
    assert L.mpcvr_histogram_percentile(hp, 5, None) == api.E_POINTER
    for ppm in (0, 1000001, 2 ** 32 - 1):
        assert L.mpcvr_histogram_percentile(hp, ppm, C.byref(code)) == api.E_INVALIDARG
    empty = _hist([])
    assert L.mpcvr_histogram_percentile(C.c_void_p(empty.ctypes.data), 5, C.byref(code)) == api.E_INVALIDARG
    assert code.value == -7, "a refusal wrote the code"
    assert L.mpcvr_histogram_percentile(hp, 5, C.byref(code)) == 0 and code.value == 7
    assert L.mpcvr_light_level_from_histogram(hp, RGB10A2, C.byref(out)) == 0 and (out.pixels, out.min_code, out.max_code) == (1, 7, 7)
