// vp_lut3d_core.h — the arithmetic of the 3D LUT pass (EXTENSION: include/mpcvr.h, mpcvr_lut3d_pass), shared by the kernel (vp_lut3d.hip)
// and the host (mpcvr_plan_lut3d_value, mpcvr_plan_lut3d_entries: vp_plan.cpp) the way vp_deint_core.h serves both sides.  The reference
// has no LUT, so there is no reference line to cite: the definition is the text of include/mpcvr.h, modelled bit for bit by
// tests/lut3d_model.py.
//
//   Per channel code c of the source (0 .. maxin):  t = c (n - 1);  i = min(t / maxin, n - 2);  f = t - i maxin, 0 .. maxin.
//   The channels ordered so that f(1) >= f(2) >= f(3):  V0 = lut[iR, iG, iB], V1 = V0 + one step along the axis of f(1), V2 = V1 + one
//   step along the axis of f(2), V3 = lut[iR + 1, iG + 1, iB + 1];  weights maxin - f(1), f(1) - f(2), f(2) - f(3), f(3).
//   Per output channel:  acc = sum w_j V_j[k] (at most 1023 * 65535);  v = (acc + (maxin >> 1)) / maxin;  out = (v maxout + 32767) / 65535.
// Everything is a 32-bit unsigned integer.  A tie between two f's gives the vertex the two orders disagree about the weight 0, so the
// order chosen among equals (below: R before G before B for the largest, B before G before R for the smallest) cannot show.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MPCVR_L3_HD __host__ __device__ __forceinline__
#else
#define MPCVR_L3_HD inline
#endif

namespace mpcvr {

constexpr int kLut3dMinN = 2, kLut3dMaxN = 65;

// one table entry as two words: lo = R | G << 16, hi = B | pad << 16 (four little-endian uint16_t {R, G, B, pad})
struct Lut3dEntry { uint32_t lo, hi; };

// the codes of R, G, B in a texel: B8G8R8A8 is B | G << 8 | R << 16, R10G10B10A2 is R | G << 10 | B << 20; A / X ignored
template <bool IN10> MPCVR_L3_HD uint32_t Lut3dCode(uint32_t texel, int k /* 0 R, 1 G, 2 B */)
{
    return IN10 ? (texel >> (10 * k)) & 0x3ffu : (texel >> (16 - 8 * k)) & 0xffu;
}

// a texel of the destination from its three codes, the A / X bits all ones
template <bool OUT10> MPCVR_L3_HD uint32_t Lut3dPack(uint32_t r, uint32_t g, uint32_t b)
{
    return OUT10 ? (r | g << 10 | b << 20 | 0xc0000000u) : (b | g << 8 | r << 16 | 0xff000000u);
}

// the cell and the fraction of one code
template <uint32_t MAXIN> MPCVR_L3_HD void Lut3dSplit(uint32_t c, uint32_t n, uint32_t *i, uint32_t *f)
{
    const uint32_t t = c * (n - 1u);
    uint32_t q = t / MAXIN;                            // (a constant divisor)
    if (q > n - 2u) q = n - 2u;
    *i = q; *f = t - q * MAXIN;
}

// one weighted channel sum to the destination's code
template <uint32_t MAXIN, uint32_t MAXOUT> MPCVR_L3_HD uint32_t Lut3dFinish(uint32_t acc)
{
    const uint32_t v = (acc + (MAXIN >> 1)) / MAXIN;
    return (v * MAXOUT + 32767u) / 65535u;
}

// One texel.  fetch(index) returns the Lut3dEntry at that index of the table: a global load, an LDS read or a host array.
template <bool IN10, bool OUT10, class Fetch> MPCVR_L3_HD uint32_t Lut3dTexel(uint32_t texel, uint32_t n, Fetch fetch)
{
    constexpr uint32_t MAXIN = IN10 ? 1023u : 255u, MAXOUT = OUT10 ? 1023u : 255u;
    uint32_t iR, iG, iB, fR, fG, fB;
    Lut3dSplit<MAXIN>(Lut3dCode<IN10>(texel, 0), n, &iR, &fR);
    Lut3dSplit<MAXIN>(Lut3dCode<IN10>(texel, 1), n, &iG, &fG);
    Lut3dSplit<MAXIN>(Lut3dCode<IN10>(texel, 2), n, &iB, &fB);
    const uint32_t sG = n, sB = n * n;                 // the axis strides: R 1, G n, B n^2
    // the axis of the largest and of the smallest fraction, never the same axis (all equal: R and B), without a branch
    const uint32_t sMax = (fR >= fG && fR >= fB) ? 1u : (fG >= fB ? sG : sB);
    const uint32_t sMin = (fB <= fR && fB <= fG) ? sB : (fG <= fR ? sG : 1u);
    const uint32_t fMax = fR > fG ? (fR > fB ? fR : fB) : (fG > fB ? fG : fB);
    const uint32_t fMin = fR < fG ? (fR < fB ? fR : fB) : (fG < fB ? fG : fB);
    const uint32_t fMid = fR + fG + fB - fMax - fMin;
    const uint32_t e0 = (iB * n + iG) * n + iR, e3 = e0 + 1u + sG + sB;
    const Lut3dEntry v0 = fetch(e0), v1 = fetch(e0 + sMax), v2 = fetch(e3 - sMin), v3 = fetch(e3);
    const uint32_t w0 = MAXIN - fMax, w1 = fMax - fMid, w2 = fMid - fMin, w3 = fMin;
    const uint32_t r = w0 * (v0.lo & 0xffffu) + w1 * (v1.lo & 0xffffu) + w2 * (v2.lo & 0xffffu) + w3 * (v3.lo & 0xffffu);
    const uint32_t g = w0 * (v0.lo >> 16) + w1 * (v1.lo >> 16) + w2 * (v2.lo >> 16) + w3 * (v3.lo >> 16);
    const uint32_t b = w0 * (v0.hi & 0xffffu) + w1 * (v1.hi & 0xffffu) + w2 * (v2.hi & 0xffffu) + w3 * (v3.hi & 0xffffu);
    return Lut3dPack<OUT10>(Lut3dFinish<MAXIN, MAXOUT>(r), Lut3dFinish<MAXIN, MAXOUT>(g), Lut3dFinish<MAXIN, MAXOUT>(b));
}

}  // namespace mpcvr
