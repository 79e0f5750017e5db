"""The two exact rescalings k_fused_up2x_bp folds into neighbouring FMAs (csrc/vp_fused_up2x_bp.h, stage C of csrc/vp_fused_up2x.h):
the identities, in exact arithmetic, and what they take out of the compiled loop (no GPU needed).

A. The convert output is stored to m_TexConvertOutput (UNORM) and read back.  The generic kernel: u = fma(x, maxv, 2^23) = 2^23 + q exactly
   (q the UNORM code), then (u - 2^23) * inv.  The twin: fma(u, inv, -2^23 * inv).  The real number under the FMA's one rounding is
   (2^23 + q) * inv - 2^23 * inv = q * inv — what float(q) * inv rounds — provided 2^23 * inv is a float (a power of two times one).
   Checked for EVERY q of both internal formats.

B. The odd luma column's chroma.  The generic kernel: fma(m, fma(Un, .5, U0 * .5), acc).  The twin: fma(.5 * m, Un + U0, acc), the halved
   coefficient made on the host.  Un and U0 are chroma codes under quarter weights; halving is exact, so both inner values are roundings of
   the same real number scaled by two, and both FMAs round the same real number.  Checked bitwise with an exact FMA on > 200,000 tuples
   drawn from the codes, weights, matrices and accumulators the kernel meets.

The compiled loop: the twin's headline instantiation, compiled as tests/test_up2x_bp_loop.py compiles it, holds no more than
1,056 packed + 810 plain + 96 transcendental instructions and 3,310 issue units per four iterations (before the folds: 1,088 + 829 + 96 =
3,389), in at most 168 VGPRs at occupancy 3 without scratch or spills.
"""
import random
import struct
from fractions import Fraction

import numpy as np
import pytest

from tests.golden.cases import FULL, M709, M2020, MPEG2, P709, P2020, T709, TPQ, TV, ext
from tests.test_up2x_bp_loop import needs_tools, twin  # noqa: F401  (the fixture: the twin's headline kernel, compiled and disassembled)


# ---- exact arithmetic on floats: a value is an integer n over 2^k ----
def rne32(n, k):
    """n / 2^k rounded once to float32 (nearest, ties to even; subnormals included), as a Python float holding that value"""
    if n == 0:
        return 0.0
    sign, n = (-1.0, -n) if n < 0 else (1.0, n)
    shift = max(n.bit_length() - 24, k - 149, 0)         # bits to drop: 24 significant ones remain, none below 2^-149
    q = n
    if shift > 0:
        q, r = divmod(n, 1 << shift)
        half = 1 << (shift - 1)
        if r > half or (r == half and (q & 1)):
            q += 1
    return sign * float(np.ldexp(np.float64(q), shift - k))      # q < 2^25: exact in a double


def parts(x):
    n, d = float(x).as_integer_ratio()                   # exact; d is a power of two
    return n, d.bit_length() - 1


def fma32(a, b, c):
    """fma(a, b, c) of three float32 values: one rounding of the exact a * b + c"""
    (an, ak), (bn, bk), (cn, ck) = parts(a), parts(b), parts(c)
    k = max(ak + bk, ck)
    return rne32(an * bn * (1 << (k - ak - bk)) + cn * (1 << (k - ck)), k)       # (a zero result is +0: what RNE gives wherever a term is +0 or the sum cancels)


def bits(x):
    return struct.pack("<f", x)


def test_rne32_is_float32_rounding():
    r = random.Random(7)
    for _ in range(20000):
        x = r.uniform(-4.0, 4.0) * 2.0 ** r.randint(-140, 20)
        n, k = parts(x)
        assert bits(rne32(n, k)) == bits(float(np.float32(x))), x
    assert rne32(3, 1) == 1.5 and rne32((1 << 24) + 1, 0) == float(1 << 24) and rne32((1 << 24) + 3, 0) == float((1 << 24) + 4)


# ---- identity A ----
@pytest.mark.parametrize("maxv", [255, 1023])
def test_read_back_inside_an_fma_rounds_like_the_product(maxv):
    inv = np.float32(1.0) / np.float32(maxv)             # FillFusedArgs: a.inv_maxv = 1.0f / a.maxv
    big = Fraction(1 << 23)
    finv = Fraction(float(inv))
    nbc = np.float32(-8388608.0) * inv                   # fused_up2x_body: the FMA's addend
    assert Fraction(float(nbc)) == -big * finv, "2^23 * inv is a float"
    for q in range(maxv + 1):
        u = np.float32(8388608.0 + q)
        assert Fraction(float(u)) == big + q             # u = 2^23 + q exactly
        exact = (big + q) * finv - big * finv            # what the FMA rounds
        assert exact == q * finv
        folded = rne32(exact.numerator, exact.denominator.bit_length() - 1)
        assert bits(folded) == bits(fma32(float(u), float(inv), float(nbc)))
        plain = float(np.float32(q) * inv)               # (u - 2^23) * inv: the subtraction is exact
        assert bits(folded) == bits(plain), (maxv, q, folded, plain)
    assert bits(fma32(8388608.0, float(inv), float(nbc))) == bits(0.0)      # q = 0: +0 in both forms


# ---- identity B ----
def matrices(mpcvr):
    """(m[2], m[4], m[5], m[7], offsets) as FillFusedArgs hands them to the kernel, per sample format x matrix x range x ProcAmp"""
    api = mpcvr
    out = []
    for cformat, sc in ((2, np.float32(1.0) / np.float32(65535.0)), (1, np.float32(1.0) / np.float32(255.0))):
        for mat, prim, trc in ((M709, P709, T709), (M2020, P2020, TPQ)):
            for rng in (TV, FULL):
                for procamp in ((0.0, 1.0, 0.0, 1.0), (10.0, 1.2, 0.0, 1.3), (-20.0, 0.8, 0.0, 0.6)):
                    cm, _ = api.plan_color_matrix(cformat, 128, 72, ext(MPEG2, rng, mat, prim, trc), *procamp)
                    cm = np.array(cm, np.float32)
                    assert cm[1] == 0.0 and cm[8] == 0.0, "no hue: the structural zeros"
                    m = (cm[:9] * sc).astype(np.float32)
                    out.append(([float(m[i]) for i in (2, 4, 5, 7)], [float(c) for c in cm[9:12]], 1023 if cformat == 2 else 255, 6 if cformat == 2 else 0))
    return out


def test_halved_coefficient_on_the_sum_equals_the_coefficient_on_the_mean(mpcvr):
    r = random.Random(24)
    quarter_pairs = ((0.25, 0.75), (0.75, 0.25), (0.0, 1.0), (1.0, 0.0), (0.5, 0.5))      # (w0, w1) of chroma rows n, n + 1: quarter()

    def column(top, bot, w):          # Ucol[0] = fma(bot, w1, top * w0)
        return fma32(bot, w[1], fma32(top, w[0], 0.0))

    n = 0
    for coeffs, offs, top_code, shift in matrices(mpcvr):
        for m in coeffs:
            assert m == 0.0 or float(np.float32(0.5) * np.float32(m)) * 2.0 == m       # the gate's condition (FusedUp2xBpTakes)
        corners = [0, top_code, 64 if top_code == 1023 else 16, (top_code + 1) // 2]
        for i in range(800):
            code = lambda: float((r.choice(corners) if r.random() < 0.25 else r.randint(0, top_code)) << shift)
            w = r.choice(quarter_pairs)
            u0 = column(code(), code(), w)
            un = 0.0 if i % 16 == 0 else column(code(), code(), w)        # lane 63 reads 0.0 from the lane it does not have
            for m in coeffs:
                if m == 0.0:
                    continue
                h = float(np.float32(0.5) * np.float32(m))
                # accumulators: the matrix offsets, a partial sum of the chain (offset + another coefficient's term), anything of that size
                accs = [r.choice(offs), fma32(r.choice(coeffs), column(code(), code(), w), r.choice(offs)), r.uniform(-2.0, 2.0) * 2.0 ** r.randint(-12, 0)]
                for acc in accs:
                    acc = float(np.float32(acc))
                    old = fma32(m, fma32(un, 0.5, fma32(u0, 0.5, 0.0)), acc)
                    new = fma32(h, fma32(un, 1.0, u0), acc)
                    assert bits(old) == bits(new), (m, un, u0, acc, old, new)
                    n += 1
    print("tuples:", n)
    assert n >= 200000


# ---- the compiled loop ----
@needs_tools
def test_folds_take_their_instructions_out_of_the_loop(twin):  # noqa: F811
    res, body, lo, hi = twin["res"], twin["body"], twin["lo"], twin["hi"]
    cnt = {"packed": 0, "plain": 0, "trans": 0}
    for ins in body[lo:hi + 1]:
        if ins.op.startswith("v_pk_") and ins.op.endswith("_f32"):
            cnt["packed"] += 1
        elif ins.op.startswith(("v_exp", "v_log", "v_rcp", "v_rsq", "v_sqrt", "v_sin", "v_cos")):
            cnt["trans"] += 1
        elif ins.op.startswith("v_") and not ins.op.startswith("v_mfma"):
            cnt["plain"] += 1
    units = cnt["plain"] + 2 * cnt["packed"] + 4 * cnt["trans"]
    print("VALU instructions of the twin's loop:", cnt, "issue units:", units, "resources:", res)
    assert cnt["packed"] <= 1056 and cnt["plain"] <= 810 and cnt["trans"] <= 96, cnt
    assert units <= 3310, units
    assert res["vgprs"] <= 168 and res["occupancy"] == 3 and res["scratch"] == 0 and res["vgpr_spill"] == 0, res
