// vp_deband_core.h — the arithmetic of the deband pass (EXTENSION: include/mpcvr.h, mpcvr_deband_pass), shared by the kernel (vp_deband.hip)
// and the host (mpcvr_deband_host: DebandSurfaceHost below) the way vp_lut3d_core.h serves both sides of the LUT pass.  The reference has
// no deband, so there is no reference line to cite: the definition is the text of include/mpcvr.h, modelled bit for bit by
// tests/deband_model.py.
//
//   H(x, y, k, seed):  h = x + y 0x9E3779B1 + k 0x85EBCA77 + seed 0xC2B2AE3D;  h ^= h >> 16;  h *= 0x7feb352d;  h ^= h >> 15;
//                      h *= 0x846ca68b;  h ^= h >> 16                                    (32-bit unsigned, wrapping)
//   Per texel (x, y):  cur = 4 c per channel.  For k = 1 .. iterations:  r = range k,  h = H(x, y, k, seed),
//     dx = (((h & 0xffff) (2 r + 1)) >> 16) - r,  dy = (((h >> 16) (2 r + 1)) >> 16) - r;  the taps are the SOURCE texels at
//     (x + dx, y + dy), (x - dy, y + dx), (x - dx, y - dy), (x + dy, y - dx), every coordinate clamped to the surface;  s = their sum per
//     channel;  cur = s where |s - cur| k <= threshold.
//   Output:  den = 4 maxin;  d = den / 2, or ((H(x, y, 0, seed) >> 8) den) >> 24 with the dither on;  out = (cur maxout + d) / den.
// Everything is a 32-bit integer but the dither's product (34 bits, taken as a 32 x 32 -> high word multiply); cur and s lie in
// 0 .. 4 maxin, so cur maxout + d < 2^23.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MPCVR_DB_HD __host__ __device__ __forceinline__
#else
#define MPCVR_DB_HD inline
#endif

namespace mpcvr {

constexpr int kDebandMaxRange = 64, kDebandMaxIterations = 4, kDebandMaxHalo = 64;

// the parameters of a pass as the kernel takes them (mpcvr_deband_params + the seed; checked by DebandParamsValid, vp_deband.h)
struct DebandArgs { int32_t range, iterations, threshold, dither; };

MPCVR_DB_HD uint32_t DebandHash(uint32_t x, uint32_t y, uint32_t k, uint32_t seed)
{
    uint32_t h = x + y * 0x9E3779B1u + k * 0x85EBCA77u + seed * 0xC2B2AE3Du;
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return h;
}

// the offset of iteration k's first tap; the other three are its quarter turns (-dy, dx), (-dx, -dy), (dy, -dx)
MPCVR_DB_HD void DebandOffset(uint32_t x, uint32_t y, int k, int range, uint32_t seed, int *dx, int *dy)
{
    const uint32_t r = (uint32_t)(range * k), h = DebandHash(x, y, (uint32_t)k, seed);
    *dx = (int)(((h & 0xffffu) * (2u * r + 1u)) >> 16) - (int)r;
    *dy = (int)(((h >> 16) * (2u * r + 1u)) >> 16) - (int)r;
}

// the coordinates of tap j (0 .. 3) of a texel at (x, y) with first offset (dx, dy), not clamped
MPCVR_DB_HD void DebandTapAt(int x, int y, int dx, int dy, int j, int *tx, int *ty)
{
    const int ox = j == 0 ? dx : j == 1 ? -dy : j == 2 ? -dx : dy;
    const int oy = j == 0 ? dy : j == 1 ? dx : j == 2 ? -dy : -dx;
    *tx = x + ox; *ty = y + oy;
}

// the codes of R, G, B in a texel: B8G8R8A8 is B | G << 8 | R << 16, R10G10B10A2 is R | G << 10 | B << 20; A / X ignored
template <bool IN10> MPCVR_DB_HD int DebandCode(uint32_t texel, int k /* 0 R, 1 G, 2 B */)
{
    return (int)(IN10 ? (texel >> (10 * k)) & 0x3ffu : (texel >> (16 - 8 * k)) & 0xffu);
}

template <bool OUT10> MPCVR_DB_HD uint32_t DebandPack(uint32_t r, uint32_t g, uint32_t b)
{
    return OUT10 ? (r | g << 10 | b << 20 | 0xc0000000u) : (b | g << 8 | r << 16 | 0xff000000u);
}

// one iteration of one texel: cur[3] (quarter codes) against the sum of the four taps
template <bool IN10> MPCVR_DB_HD void DebandStep(int cur[3], const uint32_t taps[4], int k, int threshold)
{
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int s = DebandCode<IN10>(taps[0], c) + DebandCode<IN10>(taps[1], c) + DebandCode<IN10>(taps[2], c) + DebandCode<IN10>(taps[3], c);
        const int d = s > cur[c] ? s - cur[c] : cur[c] - s;
        if (d * k <= threshold) cur[c] = s;
    }
}

// the destination texel of the quarter codes cur[3]
template <bool IN10, bool OUT10> MPCVR_DB_HD uint32_t DebandFinish(const int cur[3], uint32_t x, uint32_t y, uint32_t seed, int dither)
{
    constexpr uint32_t MAXIN = IN10 ? 1023u : 255u, MAXOUT = OUT10 ? 1023u : 255u, DEN = 4u * MAXIN;
    // (the product needs 34 bits: it is the high word of (H & 0xffffff00) * den)
    const uint32_t d = dither ? (uint32_t)(((uint64_t)(DebandHash(x, y, 0u, seed) & 0xffffff00u) * DEN) >> 32) : DEN / 2u;
    return DebandPack<OUT10>(((uint32_t)cur[0] * MAXOUT + d) / DEN, ((uint32_t)cur[1] * MAXOUT + d) / DEN, ((uint32_t)cur[2] * MAXOUT + d) / DEN);
}

// One texel.  fetch(tx, ty) returns the source texel at coordinates that are NOT clamped yet: the caller clamps, or reads an image that
// was clamped when it was staged.
template <bool IN10, bool OUT10, class Fetch>
MPCVR_DB_HD uint32_t DebandTexel(uint32_t texel, int x, int y, const DebandArgs &a, uint32_t seed, Fetch fetch)
{
    int cur[3] = {4 * DebandCode<IN10>(texel, 0), 4 * DebandCode<IN10>(texel, 1), 4 * DebandCode<IN10>(texel, 2)};
    for (int k = 1; k <= a.iterations; k++) {
        int dx, dy;
        DebandOffset((uint32_t)x, (uint32_t)y, k, a.range, seed, &dx, &dy);
        uint32_t taps[4];
        for (int j = 0; j < 4; j++) {
            int tx, ty;
            DebandTapAt(x, y, dx, dy, j, &tx, &ty);
            taps[j] = fetch(tx, ty);
        }
        DebandStep<IN10>(cur, taps, k, a.threshold);
    }
    return DebandFinish<IN10, OUT10>(cur, (uint32_t)x, (uint32_t)y, seed, a.dither);
}

// ---- one surface in HOST memory (mpcvr_deband_host): the definition executed texel by texel ----
template <bool IN10, bool OUT10>
inline void DebandSurfaceHostT(const uint8_t *src, int64_t srcPitch, int w, int h, const DebandArgs &a, uint32_t seed, uint8_t *dst, int64_t dstPitch)
{
    const auto at = [&](int tx, int ty) {
        tx = tx < 0 ? 0 : tx > w - 1 ? w - 1 : tx;
        ty = ty < 0 ? 0 : ty > h - 1 ? h - 1 : ty;
        return *(const uint32_t *)(src + (int64_t)ty * srcPitch + (int64_t)tx * 4);
    };
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            *(uint32_t *)(dst + (int64_t)y * dstPitch + (int64_t)x * 4) = DebandTexel<IN10, OUT10>(at(x, y), x, y, a, seed, at);
}

inline void DebandSurfaceHost(const uint8_t *src, int64_t srcPitch, bool in10, int w, int h, const DebandArgs &a, uint32_t seed, uint8_t *dst, int64_t dstPitch, bool out10)
{
    if (in10) out10 ? DebandSurfaceHostT<true, true>(src, srcPitch, w, h, a, seed, dst, dstPitch) : DebandSurfaceHostT<true, false>(src, srcPitch, w, h, a, seed, dst, dstPitch);
    else      out10 ? DebandSurfaceHostT<false, true>(src, srcPitch, w, h, a, seed, dst, dstPitch) : DebandSurfaceHostT<false, false>(src, srcPitch, w, h, a, seed, dst, dstPitch);
}

}  // namespace mpcvr
