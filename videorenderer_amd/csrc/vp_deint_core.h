// vp_deint_core.h — the arithmetic of the motion-adaptive deinterlacer (EXTENSION: include/mpcvr.h, mpcvr_deint_pass), shared by the kernel
// (vp_deint.hip) and the host (mpcvr_deint_plane_host, mpcvr_capi.cpp) the way vp_tensor_core.h serves both sides of the tensor passes.  The
// reference hands deinterlacing to the fixed-function video processor (out of scope), so there is no reference line to cite:
// the definition is the text of include/mpcvr.h, modelled bit for bit by tests/deint_model.py.
//
// One missing component from its taps.  Everything is signed 32-bit integer arithmetic on components of at most 16 bits: no sum below
// leaves 19 bits, and >> is an arithmetic shift of a value that is negative only in the interlacing check.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MPCVR_DI_HD __host__ __device__ __forceinline__
#else
#define MPCVR_DI_HD inline
#endif

namespace mpcvr {

enum DeintMode { DI_ADAPTIVE = 0, DI_ADAPTIVE_NOCHECK = 1 };          // MPCVR_DEINT_ADAPTIVE_EXT / _NOCHECK_EXT (mpcvr_capi.cpp asserts they agree)

constexpr int kDeintReach = 3;                                        // channel steps the directional scores reach to either side

MPCVR_DI_HD int DeintAbs(int v) { return v < 0 ? -v : v; }
MPCVR_DI_HD int DeintMin(int a, int b) { return a < b ? a : b; }
MPCVR_DI_HD int DeintMax(int a, int b) { return a > b ? a : b; }

// |a - b| + acc for components a, b in 0 .. 65535: on the device the packed 16-bit sum of absolute differences with empty high halves
MPCVR_DI_HD int DeintSad(int a, int b, int acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)__builtin_amdgcn_sad_u16((unsigned)a, (unsigned)b, (unsigned)acc);
#else
    return DeintAbs(a - b) + acc;
#endif
}

// up / dn point at the CENTRE of the line above / below: up[k] = cur[ym][x + k cs], k = -3 .. 3, column clamped into the channel
MPCVR_DI_HD int DeintScore(const int *up, const int *dn, int j)
{
    return DeintSad(up[-1 + j], dn[-1 - j], DeintSad(up[j], dn[-j], DeintSad(up[1 + j], dn[1 - j], 0)));
}
MPCVR_DI_HD int DeintPred(const int *up, const int *dn, int j) { return (up[j] + dn[-j]) >> 1; }

// The taps of one missing component at line y:
//   up, dn           cur[ym], cur[yp] around the column (above)
//   a, b             A[y][x], B[y][x]: the frames holding the missing-parity field just before / after the shown field
//   pm, pp, nm, np   prev[ym][x], prev[yp][x], next[ym][x], next[yp][x]
//   check            the interlacing check applies (mode 0, and y - 2 >= 0, y + 2 < lines); then am2, bm2 = A, B at y - 2, ap2, bp2 at y + 2
MPCVR_DI_HD int DeintComponent(const int *up, const int *dn, int a, int b, int pm, int pp, int nm, int np,
                               bool check, int am2, int bm2, int ap2, int bp2)
{
    const int c = up[0], e = dn[0], d = (a + b) >> 1;
    const int t0 = DeintSad(a, b, 0);
    const int t1 = DeintSad(pm, c, DeintSad(pp, e, 0)) >> 1;
    const int t2 = DeintSad(nm, c, DeintSad(np, e, 0)) >> 1;
    int diff = DeintMax(DeintMax(t0 >> 1, t1), t2);

    int best = DeintScore(up, dn, 0) - 1, sp = DeintPred(up, dn, 0);
#if defined(__clang__)
#pragma unroll
#endif
    for (int s = -1; s <= 1; s += 2) {
        const int s1 = DeintScore(up, dn, s);
        if (s1 < best) {
            best = s1; sp = DeintPred(up, dn, s);
            const int s2 = DeintScore(up, dn, 2 * s);
            if (s2 < best) { best = s2; sp = DeintPred(up, dn, 2 * s); }
        }
    }
    if (check) {
        const int bb = (am2 + bm2) >> 1, f = (ap2 + bp2) >> 1;
        const int mx = DeintMax(DeintMax(d - e, d - c), DeintMin(bb - c, f - e));
        const int mn = DeintMin(DeintMin(d - e, d - c), DeintMax(bb - c, f - e));
        diff = DeintMax(DeintMax(diff, mn), -mx);
    }
    return DeintMin(DeintMax(sp, d - diff), d + diff);
}

// ---- one plane in HOST memory (mpcvr_deint_plane_host): the definition executed component by component ----
inline int DeintLoadHost(const uint8_t *row, int64_t comp, int bytes, int mask)
{
    return (bytes == 2 ? (int)((const uint16_t *)row)[comp] : (int)row[comp]) & mask;
}

inline void DeintPlaneHost(const uint8_t *prev, const uint8_t *cur, const uint8_t *next, int64_t srcPitch, int comps, int lines, int bytes, int cs,
                           int mask, int keep, int first, int mode, uint8_t *dst, int64_t dstPitch)
{
    const uint8_t *const A = first ? prev : cur, *const B = first ? cur : next;
    for (int y = 0; y < lines; y++) {
        uint8_t *const drow = dst + (int64_t)y * dstPitch;
        auto put = [&](int x, int v) { if (bytes == 2) ((uint16_t *)drow)[x] = (uint16_t)v; else drow[x] = (uint8_t)v; };
        if ((y & 1) == keep) {
            for (int x = 0; x < comps; x++) put(x, DeintLoadHost(cur + (int64_t)y * srcPitch, x, bytes, mask));
            continue;
        }
        const int ym = y - 1 >= 0 ? y - 1 : y + 1, yp = y + 1 < lines ? y + 1 : y - 1;
        const bool check = mode == DI_ADAPTIVE && y - 2 >= 0 && y + 2 < lines;
        auto at = [&](const uint8_t *f, int row, int x) { return DeintLoadHost(f + (int64_t)row * srcPitch, x, bytes, mask); };
        for (int x = 0; x < comps; x++) {
            const int lo = x % cs, hi = comps - cs + lo;
            int up[2 * kDeintReach + 1], dn[2 * kDeintReach + 1];
            for (int k = -kDeintReach; k <= kDeintReach; k++) {
                const int xc = DeintMin(DeintMax(x + k * cs, lo), hi);
                up[k + kDeintReach] = at(cur, ym, xc);
                dn[k + kDeintReach] = at(cur, yp, xc);
            }
            put(x, DeintComponent(up + kDeintReach, dn + kDeintReach, at(A, y, x), at(B, y, x), at(prev, ym, x), at(prev, yp, x), at(next, ym, x), at(next, yp, x),
                                  check, check ? at(A, y - 2, x) : 0, check ? at(B, y - 2, x) : 0, check ? at(A, y + 2, x) : 0, check ? at(B, y + 2, x) : 0));
        }
    }
}

}  // namespace mpcvr
