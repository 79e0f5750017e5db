// vp_sharpen_core.h — the arithmetic of the sharpen pass (EXTENSION: include/mpcvr.h, mpcvr_sharpen_pass), shared by the kernel
// (vp_sharpen.hip) and the host (mpcvr_sharpen_host: SharpenSurfaceHost below) the way vp_deband_core.h serves both sides of the deband
// pass.  The reference has no sharpener, so there is no reference line to cite: the definition is the text of include/mpcvr.h, modelled
// bit for bit by tests/sharpen_model.py.
//
//   b_j = C(2 r, j + r), j = -r .. r (sum 4^r);  S = 16^r.  Per texel, every neighbour coordinate clamped to the surface:
//   f:      mode 0 each channel's code (the steps below per channel), mode 1 L = (54 R + 183 G + 19 B + 128) >> 8 (one field for the texel)
//   d:      S f(x, y) - sum_j sum_i b_j b_i f(x + i, y + j)                                  |d| <= S maxin <= 4,190,208
//   e:      d - min(max(d, -T), T),  T = threshold (S / 4)                                   (soft coring)
//   v:      64 S c + amount e  per channel c                                                 |v| < 2^31
//   limit:  v = min(max(v, 64 S lo), 64 S hi),  lo = max(mn - overshoot, 0),  hi = min(mx + overshoot, maxin),  mn / mx the least /
//           greatest code of the channel over the 3 x 3 neighbourhood
//   q:      (v + 8 S) >> (4 r + 4)                                                           quarter codes, 0 .. 4 maxin
//   out:    DebandFinish (vp_deband_core.h): the output stage of the deband pass, the same function
// Everything is a signed 32-bit integer.  The blur is a sum of exact integers, so the kernel's separable evaluation (SharpenRowSum over a
// row, then over the row sums) has the bits of the 2-D sum SharpenSurfaceHostT takes tap by tap.
#pragma once
#include <stdint.h>

#include "vp_deband_core.h"

namespace mpcvr {

constexpr int kSharpenMaxRadius = 3, kSharpenMaxAmount = 256;
enum { SHARPEN_RGB = 0, SHARPEN_LUMA = 1 };

// the parameters of a pass as the kernel takes them (mpcvr_sharpen_params; checked by SharpenArgsValid, vp_sharpen.h)
struct SharpenArgs { int32_t radius, amount, threshold, overshoot, mode, dither; };

// b_j = C(2 r, j + r) for j = -r .. r
template <int R> MPCVR_DB_HD constexpr int SharpenWeight(int j)
{
    static_assert(R >= 1 && R <= kSharpenMaxRadius, "radius 1 .. 3");
    const int k = j < 0 ? -j : j;
    return R == 1 ? (k == 0 ? 2 : 1) : R == 2 ? (k == 0 ? 6 : k == 1 ? 4 : 1) : (k == 0 ? 20 : k == 1 ? 15 : k == 2 ? 6 : 1);
}

// the luma of mode 1: in 0 .. maxin, the weights sum to 256
MPCVR_DB_HD int SharpenLuma(int r, int g, int b) { return (54 * r + 183 * g + 19 * b + 128) >> 8; }
template <bool IN10> MPCVR_DB_HD int SharpenLumaOf(uint32_t texel)
{
    return SharpenLuma(DebandCode<IN10>(texel, 0), DebandCode<IN10>(texel, 1), DebandCode<IN10>(texel, 2));
}

// step 3: the detail d = S f - Blur, cored softly at T = threshold (S / 4)
template <int R> MPCVR_DB_HD int SharpenCore(int d, int threshold)
{
    constexpr int S = 1 << (4 * R);
    const int T = threshold * (S / 4);
    const int m = d < -T ? -T : d > T ? T : d;         // (v_med3_i32 on the device)
    return d - m;
}

// steps 4 .. 6 of one channel: its code c, the cored detail e (its own or the luma's), the least and greatest code of its 3 x 3
// neighbourhood -> quarter codes 0 .. 4 maxin
template <bool IN10, int R> MPCVR_DB_HD int SharpenChannel(int c, int e, int mn, int mx, int amount, int overshoot)
{
    constexpr int MAXIN = IN10 ? 1023 : 255, SH = 4 * R + 6;       // 64 S = 1 << SH
    const int lo = mn - overshoot > 0 ? mn - overshoot : 0;
    const int hi = mx + overshoot < MAXIN ? mx + overshoot : MAXIN;
    int v = (c << SH) + amount * e;
    v = v < (lo << SH) ? (lo << SH) : v;
    v = v > (hi << SH) ? (hi << SH) : v;
    return (v + (8 << (4 * R))) >> (4 * R + 4);
}

// ---- one surface in HOST memory (mpcvr_sharpen_host): the definition executed texel by texel, the blur as the 2-D sum ----
template <bool IN10, bool OUT10, int R>
inline void SharpenSurfaceHostT(const uint8_t *src, int64_t srcPitch, int w, int h, const SharpenArgs &a, uint32_t seed, uint8_t *dst, int64_t dstPitch)
{
    constexpr int S = 1 << (4 * R);
    const auto at = [&](int tx, int ty) {
        tx = tx < 0 ? 0 : tx > w - 1 ? w - 1 : tx;
        ty = ty < 0 ? 0 : ty > h - 1 ? h - 1 : ty;
        return *(const uint32_t *)(src + (int64_t)ty * srcPitch + (int64_t)tx * 4);
    };
    const int fields = a.mode == SHARPEN_LUMA ? 1 : 3;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const uint32_t t = at(x, y);
            int e[3] = {0, 0, 0};
            for (int k = 0; k < fields; k++) {
                int blur = 0;
                for (int j = -R; j <= R; j++)
                    for (int i = -R; i <= R; i++) {
                        const uint32_t n = at(x + i, y + j);
                        blur += SharpenWeight<R>(j) * SharpenWeight<R>(i) * (a.mode == SHARPEN_LUMA ? SharpenLumaOf<IN10>(n) : DebandCode<IN10>(n, k));
                    }
                const int f = a.mode == SHARPEN_LUMA ? SharpenLumaOf<IN10>(t) : DebandCode<IN10>(t, k);
                e[k] = SharpenCore<R>(S * f - blur, a.threshold);
            }
            if (a.mode == SHARPEN_LUMA) e[1] = e[2] = e[0];
            int q[3];
            for (int k = 0; k < 3; k++) {
                int mn = 1023, mx = 0;
                for (int j = -1; j <= 1; j++)
                    for (int i = -1; i <= 1; i++) {
                        const int n = DebandCode<IN10>(at(x + i, y + j), k);
                        mn = n < mn ? n : mn;
                        mx = n > mx ? n : mx;
                    }
                q[k] = SharpenChannel<IN10, R>(DebandCode<IN10>(t, k), e[k], mn, mx, a.amount, a.overshoot);
            }
            *(uint32_t *)(dst + (int64_t)y * dstPitch + (int64_t)x * 4) = DebandFinish<IN10, OUT10>(q, (uint32_t)x, (uint32_t)y, seed, a.dither);
        }
}

template <bool IN10, bool OUT10>
inline void SharpenSurfaceHostR(const uint8_t *src, int64_t srcPitch, int w, int h, const SharpenArgs &a, uint32_t seed, uint8_t *dst, int64_t dstPitch)
{
    if (a.radius == 1)      SharpenSurfaceHostT<IN10, OUT10, 1>(src, srcPitch, w, h, a, seed, dst, dstPitch);
    else if (a.radius == 2) SharpenSurfaceHostT<IN10, OUT10, 2>(src, srcPitch, w, h, a, seed, dst, dstPitch);
    else                    SharpenSurfaceHostT<IN10, OUT10, 3>(src, srcPitch, w, h, a, seed, dst, dstPitch);
}

inline void SharpenSurfaceHost(const uint8_t *src, int64_t srcPitch, bool in10, int w, int h, const SharpenArgs &a, uint32_t seed, uint8_t *dst, int64_t dstPitch, bool out10)
{
    if (in10) out10 ? SharpenSurfaceHostR<true, true>(src, srcPitch, w, h, a, seed, dst, dstPitch) : SharpenSurfaceHostR<true, false>(src, srcPitch, w, h, a, seed, dst, dstPitch);
    else      out10 ? SharpenSurfaceHostR<false, true>(src, srcPitch, w, h, a, seed, dst, dstPitch) : SharpenSurfaceHostR<false, false>(src, srcPitch, w, h, a, seed, dst, dstPitch);
}

}  // namespace mpcvr
