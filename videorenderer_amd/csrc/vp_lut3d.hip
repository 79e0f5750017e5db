// vp_lut3d.hip — EXTENSION: k_lut3d, a 3D colour LUT over 32-bit RGB texels, tetrahedral interpolation in integers (vp_lut3d.h;
// definition: include/mpcvr.h, mpcvr_lut3d_pass; arithmetic: vp_lut3d_core.h; bit-exact model: tests/lut3d_model.py).  There is no
// reference line to cite: the reference has no LUT.
//
// Data flow.  4 bytes in and 4 out per texel, and four 8-byte table reads per texel at addresses the picture decides: a gather.
//   * a lane owns 4 columns of a row: one 16-byte load and one 16-byte store where the surface, its pitch and every frame are on 16 bytes
//     and the four columns lie inside the surface, dword accesses at clamped / guarded columns otherwise.  A lane loads all its texels
//     before it stores one, and no lane reads a texel of another: dst == src is safe;
//   * a wavefront owns 256 columns of a row, a workgroup of kLut3dWaves wavefronts kLut3dGroupRows rows;
//   * per texel: three (cell, fraction) splits, the three vertex offsets from the order of the fractions without a branch, 4 table reads
//     (16 per lane, issued together), 12 multiply-adds, two divisions by constants per channel (Lut3dTexel);
//   * PLACE = L3_GLOBAL: the table is read where the caller put it, 8 bytes per lane and instruction; one workgroup per tile, the frame
//     is blockIdx.z;
//   * PLACE = L3_LDS: a workgroup copies the whole table into LDS once (dynamic LDS of n^3 * 8 bytes, up to 157,464), then walks tiles
//     blockIdx.x, + gridDim.x, ... of all frames; the grid is as many workgroups as stay resident — of kLut3dWaves wavefronts while four fit
//     a CU, of kLut3dLdsWideWaves above that (blockDim.y says which), so that a CU whose LDS holds one or two tables still holds 16 or 32
//     wavefronts.  8-byte LDS reads bank on (a / 4) mod 64 within each half of the wavefront: lanes that read the same entry share one
//     access, others may collide;
//   * surface loads and stores are plain: non-temporal ones were measured and bought nothing;
//   * a batch (mpcvr_process_batch_lut3d) is one launch: the frame's {src, dst} row of Lut3dParams::frames is read at a uniform index.
// All address arithmetic is 64-bit: pitches are int64_t and a surface's last row may begin beyond 4 GiB.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>

#include "vp_lut3d.h"

namespace mpcvr {
namespace {

typedef uint32_t l3_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t l3_u2 __attribute__((ext_vector_type(2)));

// the wavefront's share of one tile: kLut3dWaveRows rows from row0, 256 columns from xw
template <bool IN10, bool OUT10, class Fetch>
__device__ __forceinline__ void Lut3dWaveTile(const Lut3dParams &p, const uint8_t *src, uint8_t *dst, int xw, int row0, int lane, Fetch fetch)
{
    const int x0 = xw + lane * 4;
    if (x0 >= p.w) return;
    const bool full = x0 + 4 <= p.w;
    const bool vin = p.src16 && full, vout = p.dst16 && full;

    uint32_t t[kLut3dWaveRows][4] = {};
#pragma unroll
    for (int i = 0; i < kLut3dWaveRows; i++) {
        if (row0 + i >= p.h) break;                    // (uniform)
        const uint8_t *row = src + (int64_t)(row0 + i) * p.src_pitch;
        if (vin) {
            const l3_u4 q = *(const l3_u4 *)(row + (int64_t)x0 * 4);
            t[i][0] = q.x; t[i][1] = q.y; t[i][2] = q.z; t[i][3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) t[i][j] = *(const uint32_t *)(row + (int64_t)min(x0 + j, p.w - 1) * 4);
        }
    }
    uint32_t o[kLut3dWaveRows][4] = {};
#pragma unroll
    for (int i = 0; i < kLut3dWaveRows; i++) {
        if (row0 + i >= p.h) break;
#pragma unroll
        for (int j = 0; j < 4; j++) o[i][j] = Lut3dTexel<IN10, OUT10>(t[i][j], (uint32_t)p.n, fetch);
    }
#pragma unroll
    for (int i = 0; i < kLut3dWaveRows; i++) {
        if (row0 + i >= p.h) break;
        uint8_t *const d = dst + (int64_t)(row0 + i) * p.dst_pitch + (int64_t)x0 * 4;
        if (vout) *(l3_u4 *)d = l3_u4{o[i][0], o[i][1], o[i][2], o[i][3]};
        else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (x0 + j < p.w) *(uint32_t *)(d + j * 4) = o[i][j];
        }
    }
}

template <bool IN10, bool OUT10, int PLACE>
__global__ __launch_bounds__(64 * (PLACE == L3_LDS ? kLut3dLdsWideWaves : kLut3dWaves)) void k_lut3d(Lut3dParams p, uint32_t col_blocks, uint32_t row_blocks, uint32_t tiles)
{
    const int lane = threadIdx.x, wv = threadIdx.y;
    if (PLACE == L3_GLOBAL) {
        const Lut3dEntry *const lut = p.lut;
        const uint8_t *src = p.src;
        uint8_t *dst = p.dst;
        if (p.frames) { const Lut3dFrame f = p.frames[blockIdx.z]; src = f.src; dst = f.dst; }
        const int row0 = ((int)blockIdx.y * kLut3dWaves + wv) * kLut3dWaveRows;       // the same for a whole wavefront
        if (row0 >= p.h) return;
        Lut3dWaveTile<IN10, OUT10>(p, src, dst, (int)blockIdx.x * kLut3dWaveCols, row0, lane, [lut](uint32_t at) {
            const l3_u2 v = *(const l3_u2 *)(lut + at);
            return Lut3dEntry{v.x, v.y};
        });
    } else {
        extern __shared__ l3_u2 table[];               // n^3 entries
        const uint32_t entries = (uint32_t)(p.n * p.n * p.n);
        const l3_u2 *const from = (const l3_u2 *)p.lut;
        const int waves = (int)blockDim.y;             // kLut3dWaves, or kLut3dLdsWideWaves where few workgroups fit a CU (LaunchFormats)
        for (uint32_t at = (uint32_t)(wv * 64 + lane); at < entries; at += 64u * (uint32_t)waves) table[at] = from[at];
        __syncthreads();
        for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {            // (uniform)
            const uint32_t cb = tile % col_blocks, rest = tile / col_blocks, rb = rest % row_blocks, z = rest / row_blocks;
            const int row0 = ((int)rb * waves + wv) * kLut3dWaveRows;
            if (row0 >= p.h) continue;
            const uint8_t *src = p.src;
            uint8_t *dst = p.dst;
            if (p.frames) { const Lut3dFrame f = p.frames[z]; src = f.src; dst = f.dst; }
            Lut3dWaveTile<IN10, OUT10>(p, src, dst, (int)cb * kLut3dWaveCols, row0, lane, [](uint32_t at) {
                const l3_u2 v = table[at];
                return Lut3dEntry{v.x, v.y};
            });
        }
    }
}

int ComputeUnits()
{
    static std::mutex mu;
    static std::map<int, int> cus;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    auto it = cus.find(dev);
    if (it != cus.end()) return it->second;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    return cus[dev] = n;
}

// more than 64 KiB of dynamic LDS has to be asked for, once per kernel and device (as vp_fused_strip.hip does)
hipError_t GrantLds(const void *kern, size_t lds)
{
    if (lds <= 64 * 1024) return hipSuccess;
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, size_t> granted;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    size_t &g = granted[{kern, dev}];
    if (g >= lds) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) g = lds;
    return e;
}

template <bool IN10, bool OUT10>
hipError_t LaunchFormats(const Lut3dParams &p, int place, uint32_t frames, hipStream_t stream, uint32_t most_tiles, uint32_t *done)
{
    const uint32_t cb = (uint32_t)((p.w + kLut3dGroupCols - 1) / kLut3dGroupCols);
    if (place == L3_GLOBAL) {
        const uint32_t rb = (uint32_t)((p.h + kLut3dGroupRows - 1) / kLut3dGroupRows);
        *done = std::min(frames, 65535u);               // the grid's z extent
        hipLaunchKernelGGL((k_lut3d<IN10, OUT10, L3_GLOBAL>), dim3(cb, rb, *done), dim3(64, kLut3dWaves), 0, stream, p, cb, rb, 0u);
        return hipGetLastError();
    }
    const size_t lds = Lut3dTableBytes(p.n);
    const void *const kern = (const void *)k_lut3d<IN10, OUT10, L3_LDS>;
    if (const hipError_t e = GrantLds(kern, lds)) return e;
    // as many workgroups as stay resident: what the LDS of a CU holds, at most the 32 wavefronts of a CU — in workgroups of
    // kLut3dWaves while four of them fit a CU, of kLut3dLdsWideWaves above that (a table of 157 KB leaves room for one workgroup)
    const uint32_t fit = (uint32_t)std::max<size_t>((size_t)160 * 1024 / lds, 1);
    const uint32_t waves = fit * kLut3dWaves >= 32 ? kLut3dWaves : kLut3dLdsWideWaves;
    const uint32_t per_cu = std::min(fit, 32u / waves);
    const uint32_t rows = waves * kLut3dWaveRows, rb = ((uint32_t)p.h + rows - 1) / rows;
    *done = std::min(frames, most_tiles / (cb * rb));  // a tile count inside 31 bits (cb * rb <= 2^19)
    const uint32_t tiles = cb * rb * *done;
    const uint32_t grid = std::min(tiles, (uint32_t)ComputeUnits() * per_cu);
    hipLaunchKernelGGL((k_lut3d<IN10, OUT10, L3_LDS>), dim3(grid), dim3(64, waves), lds, stream, p, cb, rb, tiles);
    return hipGetLastError();
}

}  // namespace

int Lut3dPlaceFor(int n)
{
    // MPCVR_LUT3D_TABLE=lds | global: the other placement for a table that fits LDS (A/B runs: tools/bench_lut3d.py); read per launch
    if (const char *e = std::getenv("MPCVR_LUT3D_TABLE")) {
        if (!std::strcmp(e, "lds") && n <= kLut3dLdsFitN) return L3_LDS;
        if (!std::strcmp(e, "global")) return L3_GLOBAL;
    }
    return Lut3dPlacement(n);
}

hipError_t LaunchLut3d(const Lut3dParams &params, bool in10, bool out10, hipStream_t stream, int n_frames)
{
    Lut3dParams p = params;
    if (p.w < 1 || p.h < 1 || p.w > 32768 || p.h > 32768 || p.n < kLut3dMinN || p.n > kLut3dMaxN || !p.lut || n_frames < 1 ||
        (n_frames > 1 && !p.frames) || (!p.frames && (!p.src || !p.dst)))
        return hipErrorInvalidValue;
    const int place = Lut3dPlaceFor(p.n);
    for (int at = 0; at < n_frames;) {
        if (params.frames) p.frames = params.frames + at;
        const uint32_t frames = (uint32_t)(n_frames - at);
        uint32_t done = 0;
        const hipError_t e = in10 ? (out10 ? LaunchFormats<true, true>(p, place, frames, stream, 0x7fffffffu, &done) : LaunchFormats<true, false>(p, place, frames, stream, 0x7fffffffu, &done))
                                  : (out10 ? LaunchFormats<false, true>(p, place, frames, stream, 0x7fffffffu, &done) : LaunchFormats<false, false>(p, place, frames, stream, 0x7fffffffu, &done));
        if (e != hipSuccess) return e;
        at += (int)done;
    }
    return hipSuccess;
}

}  // namespace mpcvr
