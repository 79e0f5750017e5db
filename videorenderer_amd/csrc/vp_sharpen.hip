// vp_sharpen.hip — EXTENSION: k_sharpen, a binomial unsharp mask over 32-bit RGB texels in integers (vp_sharpen.h; definition:
// include/mpcvr.h, mpcvr_sharpen_pass; arithmetic: vp_sharpen_core.h; bit-exact model: tests/sharpen_model.py).  There is no reference
// line to cite: the reference has no sharpener.
//
// Data flow.  4 bytes in and 4 out per texel, and a fixed (2 r + 1)^2 neighbourhood, r <= 3: a separable stencil.
//   * a workgroup of kSharpenWaves wavefronts owns a tile of 64 x 64 texels (k_deband's launch shape; frames are the grid's z);
//   * stage: the tile's rows and r above and below, 72 columns (the tile's and 4 either side), into LDS, every coordinate clamped to the
//     surface WHILE STAGING so that no later step checks a bound.  A quad of four columns inside the surface is one 16-byte load where the
//     surface, its pitch and every frame are on 16 bytes (the tile starts on a multiple of 64 columns), four clamped dword loads otherwise;
//     the only global reads of the kernel;
//   * rows: every staged row's horizontal binomial sums over the tile's 64 columns, a lane four columns from three 16-byte LDS reads.  Mode
//     0: two dwords per texel — the two outer channels of the word ride in one (a sum is <= 64 * 1023 < 2^16), G in the other; mode 1: the
//     luma's, one dword;
//   * columns and the rest: a wavefront owns 8 rows of the tile and walks them 4 at a time, 16 lanes per row, a lane 4 columns: the
//     vertical binomial sum of the row sums (2 r + 1 16-byte LDS reads per plane), the 3 x 3 minimum and maximum per channel from the image,
//     coring, limiter, the output stage (SharpenCore, SharpenChannel, DebandFinish) and one 16-byte store where the destination allows it,
//     guarded dword stores otherwise;
//   * a batch (mpcvr_process_batch_sharpen) is one launch: the frame's {src, dst, seed} row of SharpenParams::frames is read at blockIdx.z.
// All address arithmetic is 64-bit: pitches are int64_t and a surface's last row may begin beyond 4 GiB.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "vp_sharpen.h"

namespace mpcvr {
namespace {

typedef uint32_t sh_u4 __attribute__((ext_vector_type(4)));

template <bool IN10, bool OUT10, int MODE, int R>
__global__ __launch_bounds__(64 * kSharpenWaves) void k_sharpen(SharpenParams p)
{
    constexpr int ROWS = kSharpenTileRows + 2 * R, IW = kSharpenImageCols, HW = kSharpenTileCols, QUADS = IW / 4;
    constexpr int PLANES = MODE == SHARPEN_LUMA ? 1 : 2, THREADS = 64 * kSharpenWaves, S = 1 << (4 * R);
    __shared__ __attribute__((aligned(16))) uint32_t image[ROWS * IW];
    __shared__ __attribute__((aligned(16))) uint32_t sums[PLANES][ROWS * HW];
    const int lane = threadIdx.x, wv = threadIdx.y, t = wv * 64 + lane;
    const uint8_t *src = p.src;
    uint8_t *dst = p.dst;
    uint32_t seed = p.seed;
    if (p.frames) { const SharpenFrame f = p.frames[blockIdx.z]; src = f.src; dst = f.dst; seed = f.seed; }
    const int tx0 = (int)blockIdx.x * kSharpenTileCols, ty0 = (int)blockIdx.y * kSharpenTileRows;

    // ---- stage: image[ly][lx] = the texel at (tx0 - 4 + lx, ty0 - R + ly), clamped ----
    for (int item = t; item < ROWS * QUADS; item += THREADS) {
        const int ly = item / QUADS, q = item - ly * QUADS;
        const int sy = min(max(ty0 - R + ly, 0), p.h - 1), sx = tx0 - kSharpenPad + 4 * q;
        const uint8_t *row = src + (int64_t)sy * p.src_pitch;
        sh_u4 v;
        if (p.src16 && sx >= 0 && sx + 4 <= p.w) v = *(const sh_u4 *)(row + (int64_t)sx * 4);
        else {
            v.x = *(const uint32_t *)(row + (int64_t)min(max(sx, 0), p.w - 1) * 4);
            v.y = *(const uint32_t *)(row + (int64_t)min(max(sx + 1, 0), p.w - 1) * 4);
            v.z = *(const uint32_t *)(row + (int64_t)min(max(sx + 2, 0), p.w - 1) * 4);
            v.w = *(const uint32_t *)(row + (int64_t)min(max(sx + 3, 0), p.w - 1) * 4);
        }
        *(sh_u4 *)&image[ly * IW + 4 * q] = v;
    }
    __syncthreads();

    // ---- rows: sums[.][ly][c] = sum_i b_i f(image[ly][4 + c + i]) for the tile's columns c ----
    for (int item = t; item < ROWS * (HW / 4); item += THREADS) {
        const int ly = item >> 4, qx = item & 15;
        const sh_u4 *in = (const sh_u4 *)&image[ly * IW + 4 * qx];
        const sh_u4 a = in[0], b = in[1], c = in[2];
        const uint32_t n[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        uint32_t f0[12], f1[12];
#pragma unroll
        for (int i = kSharpenPad - R; i < 2 * kSharpenPad + R; i++) {
            if (MODE == SHARPEN_LUMA) f0[i] = (uint32_t)SharpenLumaOf<IN10>(n[i]);
            else if (IN10) { f0[i] = (n[i] & 0x3ffu) | ((n[i] >> 4) & 0x03ff0000u); f1[i] = (n[i] >> 10) & 0x3ffu; }      // R | B << 16, G
            else           { f0[i] = n[i] & 0x00ff00ffu; f1[i] = (n[i] >> 8) & 0xffu; }                                    // B | R << 16, G
        }
        uint32_t s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int i = -R; i <= R; i++) {
                s0[k] += (uint32_t)SharpenWeight<R>(i) * f0[kSharpenPad + k + i];
                if (MODE != SHARPEN_LUMA) s1[k] += (uint32_t)SharpenWeight<R>(i) * f1[kSharpenPad + k + i];
            }
        *(sh_u4 *)&sums[0][ly * HW + 4 * qx] = sh_u4{s0[0], s0[1], s0[2], s0[3]};
        if (MODE != SHARPEN_LUMA) *(sh_u4 *)&sums[PLANES - 1][ly * HW + 4 * qx] = sh_u4{s1[0], s1[1], s1[2], s1[3]};
    }
    __syncthreads();

    // ---- columns, coring, limiter, output ----
    const int qx = lane & 15, x0 = tx0 + 4 * qx;
    if (x0 >= p.w) return;
    const bool vout = p.dst16 && x0 + 4 <= p.w;
#pragma unroll 1
    for (int step = 0; step < kSharpenWaveRows / 4; step++) {
        const int ry = wv * kSharpenWaveRows + step * 4 + (lane >> 4), y = ty0 + ry;
        if (y >= p.h) return;
        // blur[field][column]: mode 0 the fields are R, G, B; mode 1 the luma
        int blur[3][4] = {};
#pragma unroll
        for (int j = -R; j <= R; j++) {
            const int wj = SharpenWeight<R>(j);
            const sh_u4 u = *(const sh_u4 *)&sums[0][(ry + R + j) * HW + 4 * qx];
            const uint32_t uu[4] = {u.x, u.y, u.z, u.w};
            if (MODE == SHARPEN_LUMA) {
#pragma unroll
                for (int k = 0; k < 4; k++) blur[0][k] += wj * (int)uu[k];
            } else {
                const sh_u4 g = *(const sh_u4 *)&sums[PLANES - 1][(ry + R + j) * HW + 4 * qx];
                const uint32_t gg[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    blur[IN10 ? 0 : 2][k] += wj * (int)(uu[k] & 0xffffu);
                    blur[IN10 ? 2 : 0][k] += wj * (int)(uu[k] >> 16);
                    blur[1][k] += wj * (int)gg[k];
                }
            }
        }
        // the 3 x 3 neighbourhoods of the four columns: image columns 4 qx + 3 .. 4 qx + 8, rows ry + R - 1 .. ry + R + 1
        uint32_t nb[3][6];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const uint32_t *row = &image[(ry + R - 1 + j) * IW + 4 * qx + kSharpenPad];
            const sh_u4 m = *(const sh_u4 *)row;
            nb[j][0] = row[-1]; nb[j][1] = m.x; nb[j][2] = m.y; nb[j][3] = m.z; nb[j][4] = m.w; nb[j][5] = row[4];
        }
        int cmn[3][6], cmx[3][6];                       // per channel and image column: the least / greatest of the three rows
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const int c0 = DebandCode<IN10>(nb[0][i], ch), c1 = DebandCode<IN10>(nb[1][i], ch), c2 = DebandCode<IN10>(nb[2][i], ch);
                cmn[ch][i] = min(min(c0, c1), c2);
                cmx[ch][i] = max(max(c0, c1), c2);
            }
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t texel = nb[1][k + 1];
            int e[3];
            if (MODE == SHARPEN_LUMA) e[0] = e[1] = e[2] = SharpenCore<R>(S * SharpenLumaOf<IN10>(texel) - blur[0][k], p.a.threshold);
            int q[3];
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const int c = DebandCode<IN10>(texel, ch);
                if (MODE != SHARPEN_LUMA) e[ch] = SharpenCore<R>(S * c - blur[ch][k], p.a.threshold);
                const int mn = min(min(cmn[ch][k], cmn[ch][k + 1]), cmn[ch][k + 2]), mx = max(max(cmx[ch][k], cmx[ch][k + 1]), cmx[ch][k + 2]);
                q[ch] = SharpenChannel<IN10, R>(c, e[ch], mn, mx, p.a.amount, p.a.overshoot);
            }
            o[k] = DebandFinish<IN10, OUT10>(q, (uint32_t)(x0 + k), (uint32_t)y, seed, p.a.dither);      // (a column beyond the surface is computed and not stored)
        }
        uint8_t *const d = dst + (int64_t)y * p.dst_pitch + (int64_t)x0 * 4;
        if (vout) *(sh_u4 *)d = sh_u4{o[0], o[1], o[2], o[3]};
        else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (x0 + k < p.w) *(uint32_t *)(d + k * 4) = o[k];
        }
    }
}

template <bool IN10, bool OUT10, int MODE>
hipError_t LaunchRadius(const SharpenParams &p, uint32_t frames, hipStream_t stream)
{
    const dim3 grid((uint32_t)((p.w + kSharpenTileCols - 1) / kSharpenTileCols), (uint32_t)((p.h + kSharpenTileRows - 1) / kSharpenTileRows), frames);
    const dim3 block(64, kSharpenWaves);
    if (p.a.radius == 1)      hipLaunchKernelGGL((k_sharpen<IN10, OUT10, MODE, 1>), grid, block, 0, stream, p);
    else if (p.a.radius == 2) hipLaunchKernelGGL((k_sharpen<IN10, OUT10, MODE, 2>), grid, block, 0, stream, p);
    else                      hipLaunchKernelGGL((k_sharpen<IN10, OUT10, MODE, 3>), grid, block, 0, stream, p);
    return hipGetLastError();
}

template <bool IN10, bool OUT10>
hipError_t LaunchMode(const SharpenParams &p, uint32_t frames, hipStream_t stream)
{
    return p.a.mode == SHARPEN_LUMA ? LaunchRadius<IN10, OUT10, SHARPEN_LUMA>(p, frames, stream) : LaunchRadius<IN10, OUT10, SHARPEN_RGB>(p, frames, stream);
}

}  // namespace

hipError_t LaunchSharpen(const SharpenParams &params, bool in10, bool out10, hipStream_t stream, int n_frames)
{
    SharpenParams p = params;
    if (p.w < 1 || p.h < 1 || p.w > 32768 || p.h > 32768 || !SharpenArgsValid(p.a, in10) || n_frames < 1 || (n_frames > 1 && !p.frames) ||
        (!p.frames && (!p.src || !p.dst)))
        return hipErrorInvalidValue;
    // MPCVR_SHARPEN_STAGING=dword: stage with guarded dword loads where the rule takes 16-byte loads (A/B runs: tools/bench_sharpen.py); read per launch
    if (const char *e = std::getenv("MPCVR_SHARPEN_STAGING"))
        if (!std::strcmp(e, "dword")) p.src16 = 0;
    for (int at = 0; at < n_frames;) {
        if (params.frames) p.frames = params.frames + at;
        const uint32_t frames = std::min((uint32_t)(n_frames - at), 65535u);      // the grid's z extent
        const hipError_t e = in10 ? (out10 ? LaunchMode<true, true>(p, frames, stream) : LaunchMode<true, false>(p, frames, stream))
                                  : (out10 ? LaunchMode<false, true>(p, frames, stream) : LaunchMode<false, false>(p, frames, stream));
        if (e != hipSuccess) return e;
        at += (int)frames;
    }
    return hipSuccess;
}

}  // namespace mpcvr
