"""What tests/test_tensor_in.py (host function) and tests/test_tensor_in_gpu.py (kernel) both run against the model
(tests/tensor_in_model.py): the factor sets, the table of named fp32 rows and the elements on which a fused multiply-add would give another
code.  Computed once per process."""
import functools

import numpy as np

from tests import tensor_in_model as M

F32 = np.float32
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FORMATS = (M.GBRP8, M.GBRP10, M.GBRP16)


def identity_factors(cformat):
    """a tensor in [0, 1] -> codes: (maxcode, 0) for R, G, B"""
    return (float(M.MAXCODE[cformat]),) * 3, (0.0,) * 3


def imagenet_factors(cformat):
    """a tensor normalised with ImageNet's mean / std -> codes: three different (scale, bias) pairs, as fp32"""
    m = M.MAXCODE[cformat]
    return tuple(float(F32(m * s)) for s in IMAGENET_STD), tuple(float(F32(m * a)) for a in IMAGENET_MEAN)


def bits(x):
    return int(F32(x).view(np.uint32))


def named_rows(cformat):
    """[(name, fp32 element bits)] for the factors (1, 0): u is the element itself"""
    m = M.MAXCODE[cformat]
    up, down = (lambda v: float(np.nextafter(F32(v), F32(np.inf)))), (lambda v: float(np.nextafter(F32(v), F32(-np.inf))))
    rows = [("+0", 0x00000000), ("-0", 0x80000000),
            ("smallest fp32 subnormal", 0x00000001), ("largest fp32 subnormal", 0x007fffff), ("negative fp32 subnormal", 0x80400000),
            ("a bf16 subnormal (bits << 16)", 0x00400000), ("smallest normal", 0x00800000), ("negative smallest normal", 0x80800000),
            ("quiet NaN", 0x7fc00000), ("signalling NaN", 0x7f800001), ("negative NaN", 0xffc00000), ("NaN, all ones", 0x7fffffff),
            ("+inf", 0x7f800000), ("-inf", 0xff800000), ("largest finite", 0x7f7fffff), ("negative largest finite", 0xff7fffff),
            ("maxcode", bits(m)), ("maxcode - 0.5 (a tie: down to the even maxcode - 1)", bits(m - 0.5)), ("maxcode + 0.5", bits(m + 0.5)),
            ("just below maxcode - 0.5", bits(down(m - 0.5))), ("just above maxcode - 0.5", bits(up(m - 0.5))),
            ("maxcode - 1.5 (a tie: up to the even maxcode - 1)", bits(m - 1.5)), ("maxcode + 1", bits(m + 1)), ("just below maxcode", bits(down(m))),
            ("-0.5", bits(-0.5)), ("-1", bits(-1.0)), ("0.25", bits(0.25)), ("just below 0.5", bits(down(0.5))), ("just above 0.5", bits(up(0.5)))]
    for k in (0, 1, 2, 3, 4, 5, 100, 101, 126, 127, 128, 129, 253, 254):
        rows.append((f"tie {k} + 0.5 ({'even' if k % 2 == 0 else 'odd'} k)", bits(k + 0.5)))
        rows.append((f"just below {k} + 0.5", bits(down(k + 0.5))))
        rows.append((f"just above {k} + 0.5", bits(up(k + 0.5))))
    return rows


# rows with factors of their own: (name, fp32 element bits, scale, bias)
FACTOR_ROWS = [
    ("inf with scale 0", 0x7f800000, 0.0, 7.0), ("-inf with scale 0", 0xff800000, 0.0, 7.0), ("NaN with scale 0", 0x7fc00000, 0.0, 7.0),
    ("a finite element with scale 0", bits(123.0), 0.0, 7.0), ("a subnormal with scale 0", 0x00000001, 0.0, 7.0),
    ("a subnormal with the largest scale", 0x007fffff, 2.0 ** 100, 0.0), ("a subnormal with the largest scale and a bias", 0x007fffff, 2.0 ** 100, 3.0),
    ("a subnormal product, no bias", bits(2.0 ** -120), 2.0 ** -20, 0.0), ("a subnormal product, smallest bias", bits(2.0 ** -120), 2.0 ** -20, 2.0 ** -100),
    ("a subnormal product, bias 2.5", bits(2.0 ** -120), 2.0 ** -20, 2.5), ("a subnormal product, bias 3.5", bits(-(2.0 ** -120)), 2.0 ** -20, 3.5),
    ("overflow of the product to +inf", 0x7f7fffff, 2.0 ** 100, -(2.0 ** 100)), ("overflow of the product to -inf", 0xff7fffff, 2.0 ** 100, 2.0 ** 100),
    ("-inf and the largest bias", 0xff800000, 1.0, 2.0 ** 100), ("a negative scale", bits(-100.25), -1.0, 0.0), ("a negative scale, tie", bits(-100.5), -1.0, 0.0),
    ("cancelling exactly", bits(64.0), 1.0, -64.0), ("the bias alone, a tie", bits(0.0), 1.0, 12.5),
]


@functools.lru_cache(maxsize=None)
def fma_sensitive(draws=1 << 20, seed=20):
    """Among `draws` random fp32 elements in [0, 1) under the ImageNet factors at GBRP16 (channel = index mod 3): those where an exactly
    evaluated fused multiply-add gives another code than the two roundings.  Candidates come from a float64 evaluation (the product of two
    fp32 numbers is exact there); each is then decided exactly (M.fma_code).  Returns (element bits, channel, two-rounding code, fma code)."""
    rng = np.random.default_rng(seed)
    x = rng.random(draws, dtype=np.float32)
    xb = x.view(np.uint32)
    ch = (np.arange(draws) % 3).astype(np.int64)
    scale, bias = imagenet_factors(M.GBRP16)
    s32, b32 = np.array(scale, dtype=np.float32)[ch], np.array(bias, dtype=np.float32)[ch]
    two = np.empty(draws, dtype=np.uint32)
    for k in range(3):
        two[ch == k] = M.code(xb[ch == k], M.F32, M.GBRP16, scale[k], bias[k])
    once = (x.astype(np.float64) * s32.astype(np.float64) + b32.astype(np.float64)).astype(np.float32)
    cand = np.nonzero(M.code_of(once.view(np.uint32), M.MAXCODE[M.GBRP16]) != two)[0]
    keep = [(int(xb[i]), int(ch[i]), int(two[i]), f) for i in cand
            for f in [M.fma_code(int(xb[i]), M.F32, M.GBRP16, scale[ch[i]], bias[ch[i]])] if f != int(two[i])]
    return keep
