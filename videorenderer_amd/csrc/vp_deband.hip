// vp_deband.hip — EXTENSION: k_deband, hashed four-tap debanding of 32-bit RGB texels in integers (vp_deband.h; definition:
// include/mpcvr.h, mpcvr_deband_pass; arithmetic: vp_deband_core.h; bit-exact model: tests/deband_model.py).  There is no reference line
// to cite: the reference has no deband.
//
// Data flow.  4 bytes in and 4 out per texel, and 4 x iterations reads of source texels up to R = range * iterations away in both
// directions, at offsets a hash of (x, y, k, seed) decides: the first pass of the project that reads a neighbourhood.
//   * a workgroup of kDebandWaves wavefronts owns a tile of 64 x 64 texels; a wavefront owns 8 rows of it and walks them 4 at a time:
//     16 lanes per row, a lane 4 columns — one 16-byte load and one 16-byte store where the surface, its pitch and every frame are on
//     16 bytes and the four columns lie inside the surface, dword accesses at clamped / guarded columns otherwise;
//   * a lane fetches all the taps of its four texels (4 x iterations x 4) before it uses the first, then runs the iterations and the
//     output stage (DebandStep, DebandFinish);
//   * PLACE = DB_GLOBAL: a tap is a 4-byte global load at coordinates clamped to the surface;
//   * PLACE = DB_LDS: the workgroup first stages the tile and R texels around it into LDS, (64 + 2 R)^2 dwords, every coordinate clamped
//     to the surface WHILE STAGING, so that a tap indexes the image without a bounds check: one LDS dword read.  The reads of a wavefront
//     fall on banks the hash decides ((a / 4) mod 32 within each half of the wavefront): lanes collide as balls in bins do;
//   * a batch (mpcvr_process_batch_deband) is one launch: the frame's {src, dst, seed} row of DebandParams::frames is read at blockIdx.z.
// All address arithmetic is 64-bit: pitches are int64_t and a surface's last row may begin beyond 4 GiB.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "vp_deband.h"

namespace mpcvr {
namespace {

typedef uint32_t db_u4 __attribute__((ext_vector_type(4)));

template <bool IN10, bool OUT10, int PLACE>
__global__ __launch_bounds__(64 * kDebandWaves) void k_deband(DebandParams p)
{
    extern __shared__ uint32_t image[];                // DB_LDS: (64 + 2 R) x (64 + 2 R) texels, clamped to the surface
    const int lane = threadIdx.x, wv = threadIdx.y;
    const uint8_t *src = p.src;
    uint8_t *dst = p.dst;
    uint32_t seed = p.seed;
    if (p.frames) { const DebandFrame f = p.frames[blockIdx.z]; src = f.src; dst = f.dst; seed = f.seed; }
    const int tx0 = (int)blockIdx.x * kDebandTileCols, ty0 = (int)blockIdx.y * kDebandTileRows;
    const int R = p.a.range * p.a.iterations;
    const int side_x = kDebandTileCols + 2 * R, side_y = kDebandTileRows + 2 * R;
    if (PLACE == DB_LDS) {
        // 16 rows x 32 columns of the image per step: a half wavefront reads 128 consecutive bytes of a row
        const int t = wv * 64 + lane;
        for (int ly = t >> 5; ly < side_y; ly += 2 * kDebandWaves) {
            const int sy = min(max(ty0 - R + ly, 0), p.h - 1);
            const uint8_t *row = src + (int64_t)sy * p.src_pitch;
            for (int lx = t & 31; lx < side_x; lx += 32) {
                const int sx = min(max(tx0 - R + lx, 0), p.w - 1);
                image[ly * side_x + lx] = *(const uint32_t *)(row + (int64_t)sx * 4);
            }
        }
        __syncthreads();
    }
    const auto fetch = [&](int tx, int ty) -> uint32_t {
        if (PLACE == DB_LDS) return image[(ty - (ty0 - R)) * side_x + (tx - (tx0 - R))];
        tx = min(max(tx, 0), p.w - 1);
        ty = min(max(ty, 0), p.h - 1);
        return *(const uint32_t *)(src + (int64_t)ty * p.src_pitch + (int64_t)tx * 4);
    };
    const int x0 = tx0 + (lane & 15) * 4;
    if (x0 >= p.w) return;
    const bool full = x0 + 4 <= p.w;
    const bool vin = p.src16 && full, vout = p.dst16 && full;
#pragma unroll 1
    for (int step = 0; step < kDebandWaveRows / 4; step++) {
        const int y = ty0 + wv * kDebandWaveRows + step * 4 + (lane >> 4);
        if (y >= p.h) return;
        uint32_t t[4];
        const uint8_t *row = src + (int64_t)y * p.src_pitch;
        if (vin) {
            const db_u4 q = *(const db_u4 *)(row + (int64_t)x0 * 4);
            t[0] = q.x; t[1] = q.y; t[2] = q.z; t[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) t[j] = *(const uint32_t *)(row + (int64_t)min(x0 + j, p.w - 1) * 4);
        }
        // every tap of the lane, then the arithmetic.  A column beyond the surface computes the last column's texel and is not stored
        uint32_t taps[kDebandMaxIterations][4][4] = {};
#pragma unroll
        for (int k = 1; k <= kDebandMaxIterations; k++) {
            if (k > p.a.iterations) break;             // (uniform)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int x = min(x0 + j, p.w - 1);
                int dx, dy;
                DebandOffset((uint32_t)x, (uint32_t)y, k, p.a.range, seed, &dx, &dy);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    int tx, ty;
                    DebandTapAt(x, y, dx, dy, i, &tx, &ty);
                    taps[k - 1][j][i] = fetch(tx, ty);
                }
            }
        }
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int cur[3] = {4 * DebandCode<IN10>(t[j], 0), 4 * DebandCode<IN10>(t[j], 1), 4 * DebandCode<IN10>(t[j], 2)};
#pragma unroll
            for (int k = 1; k <= kDebandMaxIterations; k++) {
                if (k > p.a.iterations) break;
                DebandStep<IN10>(cur, taps[k - 1][j], k, p.a.threshold);
            }
            o[j] = DebandFinish<IN10, OUT10>(cur, (uint32_t)min(x0 + j, p.w - 1), (uint32_t)y, seed, p.a.dither);
        }
        uint8_t *const d = dst + (int64_t)y * p.dst_pitch + (int64_t)x0 * 4;
        if (vout) *(db_u4 *)d = db_u4{o[0], o[1], o[2], o[3]};
        else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (x0 + j < p.w) *(uint32_t *)(d + j * 4) = o[j];
        }
    }
}

template <bool IN10, bool OUT10>
hipError_t LaunchFormats(const DebandParams &p, int place, uint32_t frames, hipStream_t stream)
{
    const dim3 grid((uint32_t)((p.w + kDebandTileCols - 1) / kDebandTileCols), (uint32_t)((p.h + kDebandTileRows - 1) / kDebandTileRows), frames);
    const dim3 block(64, kDebandWaves);
    if (place == DB_LDS) hipLaunchKernelGGL((k_deband<IN10, OUT10, DB_LDS>), grid, block, DebandLdsBytes(p.a.range * p.a.iterations), stream, p);
    else                 hipLaunchKernelGGL((k_deband<IN10, OUT10, DB_GLOBAL>), grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace

int DebandPlaceFor(int R, int w, int h)
{
    // MPCVR_DEBAND_TAPS=lds | global: the other placement where it is possible (A/B runs: tools/bench_deband.py); read per launch
    if (const char *e = std::getenv("MPCVR_DEBAND_TAPS")) {
        if (!std::strcmp(e, "lds") && R <= kDebandLdsFitR) return DB_LDS;
        if (!std::strcmp(e, "global")) return DB_GLOBAL;
    }
    return DebandPlacement(R, w, h);
}

hipError_t LaunchDeband(const DebandParams &params, bool in10, bool out10, hipStream_t stream, int n_frames)
{
    DebandParams p = params;
    if (p.w < 1 || p.h < 1 || p.w > 32768 || p.h > 32768 || !DebandArgsValid(p.a, in10) || n_frames < 1 || (n_frames > 1 && !p.frames) ||
        (!p.frames && (!p.src || !p.dst)))
        return hipErrorInvalidValue;
    const int place = DebandPlaceFor(p.a.range * p.a.iterations, p.w, p.h);
    for (int at = 0; at < n_frames;) {
        if (params.frames) p.frames = params.frames + at;
        const uint32_t frames = std::min((uint32_t)(n_frames - at), 65535u);      // the grid's z extent
        const hipError_t e = in10 ? (out10 ? LaunchFormats<true, true>(p, place, frames, stream) : LaunchFormats<true, false>(p, place, frames, stream))
                                  : (out10 ? LaunchFormats<false, true>(p, place, frames, stream) : LaunchFormats<false, false>(p, place, frames, stream));
        if (e != hipSuccess) return e;
        at += (int)frames;
    }
    return hipSuccess;
}

}  // namespace mpcvr
