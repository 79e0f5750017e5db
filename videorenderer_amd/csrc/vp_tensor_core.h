// vp_tensor_core.h — the arithmetic of the tensor pass (EXTENSION: include/mpcvr.h, mpcvr_tensor_pass), shared by the kernel
// (vp_tensor.hip) and the host (mpcvr_plan_tensor_value, vp_plan.cpp) the way vp_errdiff_core.h serves both sides.  The reference has no
// float output (its frames end in a swap chain), so there is no reference line to cite: the definition is the text of include/mpcvr.h,
// modelled bit for bit by tests/tensor_model.py.
//
//   c = the channel's code (0 .. 255 / 0 .. 1023);  t = fp32(c) * scale, rounded to fp32;  v = t + bias, rounded to fp32: two IEEE
//   round-to-nearest-even operations, never a fused multiply-add.  F32 stores v, F16 v rounded to nearest even to binary16 (overflow to
//   +-inf, subnormals kept), BF16 (u + 0x7FFF + ((u >> 16) & 1)) >> 16 of v's bits u.
// scale and bias are 0 or of magnitude in [2^-100, 2^100] (TensorFactorOk): t is then 0 or in [2^-100, 1023 * 2^100], and t + bias is a sum
// of two multiples of 2^-123 below 2^111 — finite, and 0 or at least 2^-123: no fp32 subnormal, infinity or NaN arises on the way.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MPCVR_TN_HD __host__ __device__ __forceinline__
#else
#define MPCVR_TN_HD inline
#endif

namespace mpcvr {

enum TensorDtype { TN_F32 = 0, TN_F16 = 1, TN_BF16 = 2 };             // MPCVR_TENSOR_F32 / F16 / BF16 (mpcvr_capi.cpp asserts they agree)
enum TensorLayout { TN_PLANAR = 0, TN_INTERLEAVED = 1 };              // MPCVR_TENSOR_PLANAR / INTERLEAVED

MPCVR_TN_HD uint32_t TensorFloatBits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

// finite, and 0 or of magnitude in [2^-100, 2^100]: read off the bits (exponent field 27 .. 227; 2^100 itself has an empty mantissa)
MPCVR_TN_HD bool TensorFactorOk(float f)
{
    const uint32_t a = TensorFloatBits(f) & 0x7fffffffu;
    return a == 0 || (a >= ((127u - 100u) << 23) && a <= ((127u + 100u) << 23));
}

// v = c * scale + bias in two roundings
MPCVR_TN_HD float TensorValue(uint32_t code, float scale, float bias)
{
    // (HIP's __fmul_rn / __fadd_rn are a plain * and + that the default -ffp-contract=fast fuses into v_fma_f32 / v_pk_fma_f32 /
    // v_fma_mixlo_f16 all the same: the pragma takes the licence away from these two operations, on the device and on the host)
#if defined(__clang__)
#pragma clang fp contract(off)
#else
#pragma STDC FP_CONTRACT OFF
#endif
    const float t = (float)code * scale;
    return t + bias;
}

// binary16 of v, round to nearest even, in integers: what the device's conversion instruction gives on every finite v
MPCVR_TN_HD uint32_t TensorHalfBitsSoft(float v)
{
    const uint32_t u = TensorFloatBits(v), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a >= 0x7f800000u) return sign | (a > 0x7f800000u ? 0x7e00u : 0x7c00u);
    if (a >= 0x477ff000u) return sign | 0x7c00u;      // 65520 and above round to infinity
    if (a < 0x38800000u) {                            // below 2^-14: a multiple of 2^-24, or 0
        if (a <= 0x33000000u) return sign;            // up to 2^-25 (the tie goes to the even 0)
        const uint32_t m = (a & 0x7fffffu) | 0x800000u, shift = 126u - (a >> 23);      // 14 .. 24
        uint32_t r = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        if (rem > half || (rem == half && (r & 1u))) r++;
        return sign | r;
    }
    uint32_t r = (a - 0x38000000u) >> 13;
    const uint32_t rem = a & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) r++;
    return sign | r;
}

MPCVR_TN_HD uint32_t TensorHalfBits(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const _Float16 h = (_Float16)v;                   // v_cvt_f16_f32: nearest even, subnormals kept (the kernel's mode register is the default)
    uint16_t b; memcpy(&b, &h, 2); return b;
#else
    return TensorHalfBitsSoft(v);
#endif
}

// the top 16 bits of v, round to nearest even (v is finite: no NaN to keep quiet)
MPCVR_TN_HD uint32_t TensorBf16Bits(float v)
{
    const uint32_t u = TensorFloatBits(v);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// the stored bits of one element (the low 16 for F16 / BF16)
template <int DTYPE> MPCVR_TN_HD uint32_t TensorElementBits(uint32_t code, float scale, float bias)
{
    const float v = TensorValue(code, scale, bias);
    return DTYPE == TN_F32 ? TensorFloatBits(v) : DTYPE == TN_F16 ? TensorHalfBits(v) : TensorBf16Bits(v);
}

// the codes of R, G, B in a texel: B8G8R8A8 is B | G << 8 | R << 16, R10G10B10A2 is R | G << 10 | B << 20; A / X ignored
template <bool IN10> MPCVR_TN_HD uint32_t TensorCode(uint32_t texel, int k /* 0 R, 1 G, 2 B */)
{
    return IN10 ? (texel >> (10 * k)) & 0x3ffu : (texel >> (16 - 8 * k)) & 0xffu;
}

// ------------------------------------------------------------------------------------------------
// The way back (EXTENSION: include/mpcvr.h, mpcvr_sample_pass; kernel vp_tensor_in.hip; host mpcvr_plan_sample_code; model
// tests/tensor_in_model.py): a tensor element to the code of a GBRP8 / GBRP10 / GBRP16 sample.
//   x = the element widened exactly to fp32, magnitudes below 2^-126 taken as +0;  t = x * scale, rounded to fp32;  u = t + bias, rounded
//   to fp32 (two operations, never fused);  code = 0 unless u > 0, maxcode where u >= maxcode, else u rounded to the nearest integer, ties
//   to even.
// A subnormal t, kept or flushed, cannot change the code: without a bias u = t and |t| < 2^-126 < 0.5 gives code 0 either way (0, a
// positive value that rounds to 0, or a negative one); with a bias |bias| >= 2^-100, the spacing of fp32 there is at least 2^-123, and
// |t| < 2^-126 is under half of it, so t + bias rounds to bias whether t was kept or not.
// ------------------------------------------------------------------------------------------------
MPCVR_TN_HD float TensorBitsFloat(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }

// binary16 bits -> the fp32 bits of the same value, in integers (subnormals are normal fp32 numbers; NaN payloads move up)
MPCVR_TN_HD uint32_t TensorHalfWidenSoft(uint32_t h)
{
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 0x1fu;
    uint32_t m = h & 0x3ffu;
    if (e == 0x1fu) return sign | 0x7f800000u | (m << 13);
    if (e) return sign | ((e + 112u) << 23) | (m << 13);
    if (!m) return sign;
    uint32_t ex = 113u;                                // m * 2^-24: shift the leading bit up to the implicit one
    while (!(m & 0x400u)) { m <<= 1; ex--; }
    return sign | (ex << 23) | ((m & 0x3ffu) << 13);
}

// the fp32 bits of an element of the tensor (bits: the low 16 for F16 / BF16), magnitudes below 2^-126 as +0
template <int DTYPE> MPCVR_TN_HD uint32_t SampleWiden(uint32_t bits)
{
    uint32_t u;
    if (DTYPE == TN_F32) u = bits;
    else if (DTYPE == TN_BF16) u = bits << 16;
    else {
#if defined(__HIP_DEVICE_COMPILE__)
        uint16_t b = (uint16_t)bits; _Float16 h; memcpy(&h, &b, 2);
        u = TensorFloatBits((float)h);                 // v_cvt_f32_f16: exact, fp16 subnormals kept (the kernel's mode register is the default)
#else
        u = TensorHalfWidenSoft(bits & 0xffffu);
#endif
    }
    return (u & 0x7f800000u) ? u : 0u;                 // an empty exponent field: a subnormal or a zero of either sign
}

// u = x * scale + bias in two roundings (the pragma: as TensorValue)
MPCVR_TN_HD float SampleValue(float x, float scale, float bias)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#else
#pragma STDC FP_CONTRACT OFF
#endif
    const float t = x * scale;
    return t + bias;
}

// maxcode as a float is exact (255, 1023, 65535); below it and above 0 the nearest integer, ties to even (v_rndne_f32 / rintf in the
// default rounding mode), is at most maxcode
MPCVR_TN_HD uint32_t SampleCodeOf(float u, float maxcode)
{
    if (!(u > 0.0f)) return 0u;                        // NaN, -inf, negatives, 0
    if (u >= maxcode) return (uint32_t)maxcode;
    return (uint32_t)__builtin_rintf(u);
}

template <int DTYPE> MPCVR_TN_HD uint32_t SampleCode(uint32_t bits, float scale, float bias, float maxcode)
{
    return SampleCodeOf(SampleValue(TensorBitsFloat(SampleWiden<DTYPE>(bits)), scale, bias), maxcode);
}

}  // namespace mpcvr
