"""The numpy model of the sample pass (include/mpcvr.h: mpcvr_sample_pass, mpcvr_plan_sample_code): a float tensor as a planar RGB sample
(GBRP8 / GBRP10 / GBRP16).  Everything that could hide a choice is done on integer bit patterns: the widening of fp16 / bf16, the flush of
magnitudes below 2^-126, the classification of u (NaN, sign, infinity) and its rounding to an integer.  The two fp32 roundings in between are
numpy's float32 multiply and float32 add (one IEEE nearest-even operation each; numpy never fuses them); by the header's argument a
subnormal product cannot change a code, so the host's denormal mode does not enter either.
fma_code() evaluates x * scale + bias exactly (fractions) and rounds once: what a fused multiply-add would store."""
from fractions import Fraction

import numpy as np

F32, F16, BF16 = 0, 1, 2
PLANAR, INTERLEAVED = 0, 1
RGB, BGR = 0, 1
GBRP8, GBRP10, GBRP16 = 26, 27, 28                  # MPCVR_CF_GBRP8 / 10 / 16
MAXCODE = {GBRP8: 255, GBRP10: 1023, GBRP16: 65535}
BYTES = {GBRP8: 1, GBRP10: 2, GBRP16: 2}
SAMPLE_DTYPE = {GBRP8: np.uint8, GBRP10: np.uint16, GBRP16: np.uint16}
ELEMENT_SIZE = {F32: 4, F16: 2, BF16: 2}
ELEMENT_DTYPE = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}


def widen(bits, dtype):
    """element bits -> the fp32 bits (uint32) of the same value, magnitudes below 2^-126 as +0"""
    b = np.asarray(bits).astype(np.uint32)
    if dtype == F32:
        u = b
    elif dtype == BF16:
        u = b << np.uint32(16)
    else:
        sign = (b & np.uint32(0x8000)) << np.uint32(16)
        e = (b >> np.uint32(10)) & np.uint32(0x1f)
        m = b & np.uint32(0x3ff)
        normal = sign | ((e + np.uint32(112)) << np.uint32(23)) | (m << np.uint32(13))
        infnan = sign | np.uint32(0x7f800000) | (m << np.uint32(13))
        # a subnormal m * 2^-24: the position of its leading bit gives the exponent, the bits below it the mantissa
        top = np.zeros_like(m)
        for k in range(10):
            top = np.where((m >> np.uint32(k)) & np.uint32(1), np.uint32(k), top)
        sub = sign | ((top + np.uint32(103)) << np.uint32(23)) | ((m << (np.uint32(23) - top)) & np.uint32(0x7fffff))
        u = np.where(e == 0x1f, infnan, np.where(e != 0, normal, np.where(m != 0, sub, sign)))
    u = u.astype(np.uint32)
    return np.where(u & np.uint32(0x7f800000), u, np.uint32(0)).astype(np.uint32)


def value_bits(xbits, scale, bias):
    """the fp32 bits of u = (x * scale rounded to fp32) + bias rounded to fp32; scale and bias are rounded to fp32 first, as the C struct holds them"""
    x = np.asarray(xbits, dtype=np.uint32).view(np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        t = x * np.float32(scale)
        u = t + np.float32(bias)
    assert t.dtype == np.float32 and u.dtype == np.float32
    return u.view(np.uint32)


def code_of(ubits, maxcode):
    """the code of u, from its bits: 0 unless u > 0, maxcode from maxcode up, else the nearest integer, ties to even"""
    b = np.asarray(ubits, dtype=np.uint32).astype(np.int64)
    mag = b & 0x7fffffff
    positive = ((b >> 31) == 0) & (mag != 0) & (mag <= 0x7f800000)          # not NaN, not negative, not zero
    e = (mag >> 23) - 127
    mant = (mag & 0x7fffff) | 0x800000                                       # (a subnormal u is far below 0.5: e = -127)
    big = positive & (mag >= np.float32(maxcode).view(np.uint32).astype(np.int64))
    shift = np.clip(23 - e, 1, 40)                                           # maxcode < 2^16: the shift is at least 8 where it counts
    q = mant >> shift
    rem = mant & ((np.int64(1) << shift) - 1)
    half = np.int64(1) << (shift - 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    return np.where(big, maxcode, np.where(positive, q, 0)).astype(np.uint32)


def code(bits, dtype, cformat, scale, bias):
    """element bits -> codes (uint32), elementwise"""
    return code_of(value_bits(widen(bits, dtype), scale, bias), MAXCODE[cformat])


def fma_code(bits, dtype, cformat, scale, bias):
    """one element: the code if x * scale + bias were evaluated exactly and rounded to fp32 ONCE (finite x only)"""
    x = Fraction(float(widen(np.uint32(bits), dtype).view(np.float32)))
    v = x * Fraction(float(np.float32(scale))) + Fraction(float(np.float32(bias)))
    maxcode = MAXCODE[cformat]
    if v <= 0:
        return 0
    if v >= 2 ** 17:
        return maxcode
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    u = round(v / ulp) * ulp                          # Fraction rounds half to even
    return maxcode if u >= maxcode else int(round(u))


def sample(tbits, dtype, layout, channel_order, cformat, scale, bias):
    """the tensor's element bits — (3, h, w) for PLANAR, (h, w, 3) for INTERLEAVED — -> (3, h, w) codes, planes G, B, R, in the sample's
    component type.  scale / bias: three each, for R, G, B of the picture whatever the channel order"""
    t = np.asarray(tbits)
    if layout == INTERLEAVED:
        t = t.transpose(2, 0, 1)
    ch = {0: 0, 1: 1, 2: 2} if channel_order == RGB else {0: 2, 1: 1, 2: 0}      # picture channel -> tensor channel
    planes = [code(t[ch[k]], dtype, cformat, scale[k], bias[k]) for k in (1, 2, 0)]
    return np.stack(planes).astype(SAMPLE_DTYPE[cformat])


def place(buf, offset, codes, pitch):
    """writes the sample's planes into the uint8 array `buf` at byte `offset`: plane p at p * pitch * h, row y at y * pitch (what the pass
    must leave of a patterned buffer: these bytes changed, every other byte untouched)"""
    _, h, w = codes.shape
    es = codes.dtype.itemsize
    for p in range(3):
        for y in range(h):
            at = offset + p * pitch * h + y * pitch
            buf[at:at + w * es] = np.ascontiguousarray(codes[p, y]).view(np.uint8)
    return buf
