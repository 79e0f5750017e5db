// vp_measure.hip — EXTENSION: k_measure_maxrgb, the histogram of max(R, G, B) over a rectangle of 32-bit RGB texels (vp_measure.h; definition:
// include/mpcvr.h, mpcvr_measure_pass; bit-exact model: tests/measure_model.py).  There is no reference line to cite: the reference's
// statistics are an on-screen overlay.
//
// Data flow.  The kernel reads 4 bytes per texel once and writes at most 4 KiB per workgroup, so it is bound by the reads — unless the
// counting serialises: neighbouring texels of real video share a code, and adds of many lanes to one LDS word take turns.
//   * a lane owns 4 columns on the surface's 16-byte grid (the grid starts at left & ~3, not at the rectangle's edge): one 16-byte load
//     per row where the surface, its pitch and the frame stride are on 16 bytes and the four columns lie inside the surface, four dword
//     loads at columns clamped into the rectangle otherwise.  Which of its four texels lie in [left, right) a lane decides once per
//     256-column step ([lo, hi) below), not per texel or per row; a lane without any loads nothing;
//   * a wavefront owns 256 columns of one row per step; a workgroup of kMeasureWaves wavefronts walks a band of kMeasureBandRows rows
//     over wg_cols columns.  A wavefront loads its kMeasureBandRows / kMeasureWaves rows of a step before it counts the first;
//   * every wavefront counts into 32-bit LDS bins of its own (1024 or 256 words: no other wavefront adds there, and no barrier stands
//     between its rows).  Three defences against adds to one word, cheapest first:
//       - every texel of the wavefront's row piece holds one code (flat areas, the letterbox): nothing is added; the piece's texel count
//         joins a pending (code, count) pair in scalar registers, which is added by ONE lane when the code changes or the tile ends;
//       - a lane whose own texels hold one code adds their number once;
//       - any other lane merges equal codes among its texels and adds once per distinct code;
//   * flush: the workgroup sums its wavefronts' copies and adds the non-empty bins to the frame's row of the histogram with 32-bit global
//     atomic adds whose result is unused (64 consecutive bins per wavefront instruction).  The rows are cleared in front of the launch.
//   * a batch is one launch: blockIdx.z is the frame, at frame_stride bytes and kHistBins words from the one before.
// All counters are 32-bit integers: the result does not depend on the order of the additions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "vp_measure.h"

namespace mpcvr {
namespace {

typedef uint32_t me_u4 __attribute__((ext_vector_type(4)));
constexpr int kRowsPerWave = kMeasureBandRows / kMeasureWaves;
static_assert(kMeasureBandRows % kMeasureWaves == 0 && kMeasureWaveCols == 256, "a wavefront takes whole rows of 64 lanes x 4 columns");

template <bool IN10> __device__ __forceinline__ uint32_t MaxRgb(uint32_t t)
{
    if (IN10) return max(max(t & 0x3ffu, (t >> 10) & 0x3ffu), (t >> 20) & 0x3ffu);      // R10G10B10A2: the top two bits are A
    return max(max(t & 0xffu, (t >> 8) & 0xffu), (t >> 16) & 0xffu);                      // B8G8R8A8: the top byte is A
}

template <bool IN10>
__global__ __launch_bounds__(64 * kMeasureWaves) void k_measure_maxrgb(MeasureParams p)
{
    constexpr int NB = IN10 ? 1024 : 256;
    __shared__ uint32_t bins[kMeasureWaves][NB];
    const int lane = threadIdx.x, wv = threadIdx.y;
    uint32_t *const my = bins[wv];
    for (int i = lane; i < NB; i += 64) my[i] = 0;     // (the wavefront's own copy: its LDS accesses stay in order, no barrier needed)

    const uint8_t *const src = p.src + (size_t)blockIdx.z * p.frame_stride;
    const int row0 = p.top + (int)blockIdx.y * kMeasureBandRows + wv;
    const int col0 = (p.left & ~3) + (int)blockIdx.x * p.wg_cols;
    uint32_t pendCode = 0, pendCount = 0;              // wavefront-uniform: texels of flat row pieces not yet added

    for (int xs = 0; xs < p.wg_cols; xs += kMeasureWaveCols) {
        const int cw = col0 + xs;                      // the wavefront's first column of this step
        if (cw >= p.right) break;                      // (uniform)
        const int c = cw + lane * 4;
        // the lane's texels inside the rectangle: [lo, hi) of its four (lane 0 always holds one: cw < right and cw + 4 > left)
        const int lo = min(max(p.left - c, 0), 4), hi = min(max(p.right - c, 0), 4);
        const int nv = max(hi - lo, 0);
        const bool v0 = lo <= 0 && 0 < hi, v1 = lo <= 1 && 1 < hi, v2 = lo <= 2 && 2 < hi, v3 = lo <= 3 && 3 < hi;
        const bool vec = p.src16 && c + 4 <= p.w;
        const uint32_t piece = (uint32_t)(min(p.right, cw + kMeasureWaveCols) - max(p.left, cw));      // texels of the wavefront's row piece

        uint32_t t[kRowsPerWave][4];
        if (nv > 0) {
#pragma unroll
            for (int i = 0; i < kRowsPerWave; i++) {
                const int r = row0 + i * kMeasureWaves;
                if (r >= p.bottom) break;              // (uniform)
                const uint8_t *row = src + (size_t)r * p.src_pitch;
                if (vec) {
                    const me_u4 q = *(const me_u4 *)(row + (size_t)c * 4);
                    t[i][0] = q.x; t[i][1] = q.y; t[i][2] = q.z; t[i][3] = q.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) t[i][k] = *(const uint32_t *)(row + (size_t)min(max(c + k, p.left), p.right - 1) * 4);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kRowsPerWave; i++) {
            if (row0 + i * kMeasureWaves >= p.bottom) break;      // (uniform)
            uint32_t m[4];
#pragma unroll
            for (int k = 0; k < 4; k++) m[k] = nv > 0 ? MaxRgb<IN10>(t[i][k]) : 0u;
            const uint32_t c0 = v0 ? m[0] : v1 ? m[1] : v2 ? m[2] : m[3];
            const bool uni = (!v0 || m[0] == c0) && (!v1 || m[1] == c0) && (!v2 || m[2] == c0) && (!v3 || m[3] == c0);
            const uint32_t ref = (uint32_t)__builtin_amdgcn_readfirstlane((int)c0);
            if (__all(nv == 0 || (uni && c0 == ref))) {
                // one code in the whole piece: nothing is added here
                if (ref == pendCode) pendCount += piece;
                else {
                    if (pendCount && lane == 0) atomicAdd(&my[pendCode], pendCount);
                    pendCode = ref; pendCount = piece;
                }
            } else if (nv > 0) {
                if (uni) atomicAdd(&my[c0], (uint32_t)nv);
                else {
                    const bool v[4] = {v0, v1, v2, v3};
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        bool first = v[k];
                        uint32_t n = 0;
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const bool same = v[j] && m[j] == m[k];
                            if (j < k && same) first = false;
                            if (j >= k && same) n++;
                        }
                        if (first) atomicAdd(&my[m[k]], n);
                    }
                }
            }
        }
    }
    if (pendCount && lane == 0) atomicAdd(&my[pendCode], pendCount);
    __syncthreads();

    uint32_t *const hist = p.hist + (size_t)blockIdx.z * kHistBins;
    for (int i = wv * 64 + lane; i < NB; i += 64 * kMeasureWaves) {
        uint32_t s = 0;
#pragma unroll
        for (int v = 0; v < kMeasureWaves; v++) s += bins[v][i];
        if (s) atomicAdd(hist + i, s);
    }
}

}  // namespace

int MeasureGroupCols(int rect_w, int rect_h, int n_frames)
{
    static const int forced = [] {
        const char *e = std::getenv("MPCVR_MEASURE_WG_COLS");
        const int v = e ? std::atoi(e) : 0;
        return v > 0 ? (v + kMeasureWaveCols - 1) / kMeasureWaveCols * kMeasureWaveCols : 0;
    }();
    if (forced) return forced;
    const long long bands = (rect_h + kMeasureBandRows - 1) / kMeasureBandRows;
    int cols = kMeasureMaxGroupCols;
    // (rect_w + 3: a left edge off the 16-byte grid adds up to three columns in front)
    while (cols > kMeasureWaveCols && (long long)((rect_w + 3 + cols - 1) / cols) * bands * n_frames < kMeasureMinGroups) cols /= 2;
    return cols;
}

hipError_t LaunchMeasure(const MeasureParams &params, bool in10, hipStream_t stream, int n_frames, int *launches)
{
    if (launches) *launches = 0;
    MeasureParams p = params;
    if (!p.hist || n_frames < 1) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(p.hist, 0, (size_t)n_frames * kHistBins * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const int rw = p.right - p.left, rh = p.bottom - p.top;
    if (rw <= 0 || rh <= 0) return hipSuccess;         // an empty rectangle: the cleared words
    if (!p.src || p.left < 0 || p.top < 0 || p.right > p.w) return hipErrorInvalidValue;
    if (p.wg_cols <= 0) p.wg_cols = MeasureGroupCols(rw, rh, n_frames);
    if (p.wg_cols % kMeasureWaveCols) return hipErrorInvalidValue;
    const int cols = p.right - (p.left & ~3);
    constexpr int kMaxZ = 65535;                        // the grid's z extent
    for (int at = 0; at < n_frames; at += kMaxZ) {
        p.src = params.src + (size_t)at * p.frame_stride;
        p.hist = params.hist + (size_t)at * kHistBins;
        const dim3 grid((unsigned)((cols + p.wg_cols - 1) / p.wg_cols), (unsigned)((rh + kMeasureBandRows - 1) / kMeasureBandRows),
                        (unsigned)std::min(kMaxZ, n_frames - at));
        const dim3 block(64, kMeasureWaves);
        if (in10) hipLaunchKernelGGL((k_measure_maxrgb<true>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((k_measure_maxrgb<false>), grid, block, 0, stream, p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (launches) ++*launches;
    }
    return hipSuccess;
}

}  // namespace mpcvr
