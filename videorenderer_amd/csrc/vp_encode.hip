// vp_encode.hip — EXTENSION: k_encode420, 32-bit RGB texels -> NV12 / P010 (vp_encode.h; definition: include/mpcvr.h, mpcvr_encode_pass;
// bit-exact model: tests/encode_model.py).  There is no reference line to cite: the reference has no RGB -> YUV path.
//
// Data flow.  The kernel is memory-bound (4 bytes in, 1.5 or 3 out per pixel) and has no reuse beyond a 2x2 block and the one-texel halo of
// the [1 2 1] sitings, so nothing goes through LDS:
//   * a lane owns 4 columns x 2 rows (two 2x2 blocks): one 16-byte load per row where the source and its pitch are on 16 bytes, four
//     dword loads otherwise and in the lane that holds the last two columns of a width that is no multiple of 4;
//   * a wavefront owns 256 columns x 2 rows, a workgroup of four wavefronts 8 rows: every load and store instruction of a wavefront covers
//     one contiguous piece of a row (1 KiB in; 256 / 512 bytes of Y per row and as much UV out);
//   * left and top-left siting need the texel left of the lane's first column: it is the neighbouring lane's last texel, fetched across lanes
//     (__shfl_up: ds_bpermute_b32, no LDS traffic); lane 0 of a wavefront loads it itself (column 0 replicates itself).  No tap reaches
//     right of a block's second column.  Top-left siting loads the row above the pair as a third row (row 0 replicates itself);
//   * B and R are summed as two 16-bit halves of one dword (16 taps of a 10-bit code are 16368), G on its own; the dot products are 32-bit
//     integer multiply-adds, modulo 2^32 until the final value, which fits (tests/test_encode.py bounds it for every plan);
//   * stores: NV12 one dword of Y per row and one of UV; P010 8 bytes each where both planes and pitches are on 8 bytes, else two dwords.
//     The lane with only two columns left stores half of that; lanes past the width store nothing.
//   * a batch (mpcvr_process_batch_yuv) is one launch: blockIdx.z is the frame, its {src, y, uv} row of EncodeParams::frames is read once per
//     wavefront with scalar loads (the address is uniform); a single frame (no table) takes its pointers from the arguments as before,
//     behind one uniform branch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "vp_encode.h"

namespace mpcvr {
namespace {

typedef uint32_t en_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t en_u2 __attribute__((ext_vector_type(2)));

// R and B of a texel as the 16-bit halves of one dword (sums of up to 16 taps stay inside a half), G alone
template <bool IN10> __device__ __forceinline__ void Split(uint32_t t, uint32_t &rb, uint32_t &g)
{
    if (IN10) { rb = (t & 0x3ffu) | ((t >> 4) & 0x03ff0000u); g = (t >> 10) & 0x3ffu; }        // R10G10B10A2: R | G << 10 | B << 20
    else { rb = t & 0x00ff00ffu; g = (t >> 8) & 0xffu; }                                         // B8G8R8A8: B | G << 8 | R << 16
}
template <bool IN10> __device__ __forceinline__ uint32_t RedOf(uint32_t rb) { return IN10 ? (rb & 0xffffu) : (rb >> 16); }
template <bool IN10> __device__ __forceinline__ uint32_t BlueOf(uint32_t rb) { return IN10 ? (rb >> 16) : (rb & 0xffffu); }

// clamp((c . (R, G, B) + bias) >> shift, 0, maxv): the sum modulo 2^32, read as a signed value (it fits), arithmetic shift
template <bool IN10> __device__ __forceinline__ uint32_t Dot(const int32_t *c, uint32_t rb, uint32_t g, int32_t bias, int shift, int maxv)
{
    const uint32_t acc = (uint32_t)c[0] * RedOf<IN10>(rb) + (uint32_t)c[1] * g + (uint32_t)c[2] * BlueOf<IN10>(rb) + (uint32_t)bias;
    const int v = (int32_t)acc >> shift;
    return (uint32_t)min(max(v, 0), maxv);
}

// the lane's four texels of one row (+ the texel left of them where the siting reads it)
template <bool HALO> __device__ __forceinline__ void LoadRow(const uint8_t *row, int x0, int w, bool vec, int lane, uint32_t t[4], uint32_t &left)
{
    if (vec) {
        const en_u4 v = *(const en_u4 *)(row + (size_t)x0 * 4);
        t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) t[k] = *(const uint32_t *)(row + (size_t)min(x0 + k, w - 1) * 4);
    }
    if (HALO) {
        left = __shfl_up(t[3], 1);                     // (every lane of the wavefront is here: lanes past the width hold clamped texels)
        if (lane == 0) left = *(const uint32_t *)(row + (size_t)max(x0 - 1, 0) * 4);
    }
}

template <bool IN10, bool OUT10, int SITING>
__global__ __launch_bounds__(256) void k_encode420(EncodeParams p)
{
    constexpr int S = kEncodeShift;
    constexpr int LOGW = SITING == ENC_CENTRE ? 2 : SITING == ENC_LEFT ? 3 : 4;
    constexpr int MAXV = OUT10 ? 1023 : 255;
    constexpr bool HALO = SITING != ENC_CENTRE;
    const int lane = threadIdx.x;
    const int pr = blockIdx.y * 4 + threadIdx.y;       // row pair: the same for a whole wavefront
    if (2 * pr >= p.h) return;
    const int x0 = (blockIdx.x * 64 + lane) * 4;
    const bool full = x0 + 4 <= p.w, any = x0 < p.w;
    const bool vec = p.src16 && full;

    // the frame: from the arguments, or its row of the table (uniform: blockIdx.z)
    uintptr_t a_src = (uintptr_t)p.src, a_y = (uintptr_t)p.y, a_uv = (uintptr_t)p.uv;
    // (the empty statement pins the arguments' pointers in scalar registers here, in front of the branch: folded into a select of
    // addresses, the single frame's pointers would come through a second load that depends on the one of p.frames)
    asm volatile("" : "+s"(a_src), "+s"(a_y), "+s"(a_uv));
    if (p.frames) {
        // (read through the constant address space: the row's address is uniform, so these are scalar loads like the arguments' own)
        typedef const EncodeFrame __attribute__((address_space(4))) *ConstRow;
        const ConstRow f = (ConstRow)(uintptr_t)(p.frames + blockIdx.z);
        a_src = (uintptr_t)f->src; a_y = (uintptr_t)f->y; a_uv = (uintptr_t)f->uv;
    }
    // (device memory either way: named as such, so that the loads and stores below stay global ones)
    typedef uint8_t __attribute__((address_space(1))) *GlobalBytes;
    const uint8_t *src = (const uint8_t *)(GlobalBytes)a_src;
    uint8_t *yp = (uint8_t *)(GlobalBytes)a_y, *uvp = (uint8_t *)(GlobalBytes)a_uv;
    const uint8_t *r0 = src + (size_t)(2 * pr) * p.src_pitch;
    uint32_t t[2][4], left[2] = {0, 0};
    LoadRow<HALO>(r0, x0, p.w, vec, lane, t[0], left[0]);
    LoadRow<HALO>(r0 + p.src_pitch, x0, p.w, vec, lane, t[1], left[1]);

    // chroma: the weighted sums of the lane's two blocks
    uint32_t srb[2], sg[2];
    if (SITING == ENC_CENTRE) {
#pragma unroll
        for (int b = 0; b < 2; b++) {
            srb[b] = sg[b] = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                uint32_t rb, g;
                Split<IN10>(t[q >> 1][2 * b + (q & 1)], rb, g);
                srb[b] += rb; sg[b] += g;
            }
        }
    } else {
        // horizontal [1 2 1] centred on the block's first column, of each row
        uint32_t hrb[3][2], hg[3][2];
#pragma unroll
        for (int r = 0; r < 2; r++) {
            uint32_t rb[5], g[5];
            Split<IN10>(left[r], rb[0], g[0]);
#pragma unroll
            for (int k = 0; k < 4; k++) Split<IN10>(t[r][k], rb[k + 1], g[k + 1]);
#pragma unroll
            for (int b = 0; b < 2; b++) {
                hrb[r][b] = rb[2 * b] + 2 * rb[2 * b + 1] + rb[2 * b + 2];
                hg[r][b] = g[2 * b] + 2 * g[2 * b + 1] + g[2 * b + 2];
            }
        }
        if (SITING == ENC_LEFT) {
#pragma unroll
            for (int b = 0; b < 2; b++) { srb[b] = hrb[0][b] + hrb[1][b]; sg[b] = hg[0][b] + hg[1][b]; }
        } else {
            // vertical [1 2 1] centred on the pair's first row: the row above (row 0 replicates itself)
            uint32_t ta[4], la = 0;
            LoadRow<true>(src + (size_t)max(2 * pr - 1, 0) * p.src_pitch, x0, p.w, vec, lane, ta, la);
            uint32_t rb[5], g[5];
            Split<IN10>(la, rb[0], g[0]);
#pragma unroll
            for (int k = 0; k < 4; k++) Split<IN10>(ta[k], rb[k + 1], g[k + 1]);
#pragma unroll
            for (int b = 0; b < 2; b++) {
                hrb[2][b] = rb[2 * b] + 2 * rb[2 * b + 1] + rb[2 * b + 2];
                hg[2][b] = g[2 * b] + 2 * g[2 * b + 1] + g[2 * b + 2];
                srb[b] = hrb[2][b] + 2 * hrb[0][b] + hrb[1][b];
                sg[b] = hg[2][b] + 2 * hg[0][b] + hg[1][b];
            }
        }
    }
    if (!any) return;                                   // (behind the cross-lane reads)

    const int32_t ybias = p.off[0] + (1 << (S - 1));
    uint32_t yv[2][4], cv[2][2];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t rb, g;
            Split<IN10>(t[r][k], rb, g);
            yv[r][k] = Dot<IN10>(p.coef, rb, g, ybias, S, MAXV);
        }
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int32_t cbias = p.off[1 + c] * (1 << LOGW) + (1 << (S - 1 + LOGW));
#pragma unroll
        for (int b = 0; b < 2; b++) cv[b][c] = Dot<IN10>(p.coef + 3 * (1 + c), srb[b], sg[b], cbias, S + LOGW, MAXV);
    }

    uint8_t *yrow = yp + (size_t)(2 * pr) * p.y_pitch;
    uint8_t *crow = uvp + (size_t)pr * p.uv_pitch;
    if (!OUT10) {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            uint8_t *d = yrow + (size_t)r * p.y_pitch + x0;
            if (full) *(uint32_t *)d = yv[r][0] | yv[r][1] << 8 | yv[r][2] << 16 | yv[r][3] << 24;
            else *(uint16_t *)d = (uint16_t)(yv[r][0] | yv[r][1] << 8);
        }
        uint8_t *d = crow + x0;
        if (full) *(uint32_t *)d = cv[0][0] | cv[0][1] << 8 | cv[1][0] << 16 | cv[1][1] << 24;
        else *(uint16_t *)d = (uint16_t)(cv[0][0] | cv[0][1] << 8);
    } else {
        // the 10-bit code in the top of a 16-bit word
#pragma unroll
        for (int r = 0; r < 3; r++) {
            uint8_t *d = (r < 2 ? yrow + (size_t)r * p.y_pitch : crow) + (size_t)x0 * 2;
            const uint32_t lo = r < 2 ? (yv[r][0] << 6 | yv[r][1] << 22) : (cv[0][0] << 6 | cv[0][1] << 22);
            const uint32_t hi = r < 2 ? (yv[r][2] << 6 | yv[r][3] << 22) : (cv[1][0] << 6 | cv[1][1] << 22);
            if (!full) *(uint32_t *)d = lo;
            else if (p.dst8) *(en_u2 *)d = en_u2{lo, hi};
            else { *(uint32_t *)d = lo; *(uint32_t *)(d + 4) = hi; }
        }
    }
}

template <bool IN10, bool OUT10>
hipError_t LaunchSiting(const EncodeParams &p, int siting, dim3 grid, hipStream_t stream)
{
    const dim3 block(64, 4);
    switch (siting) {
    case ENC_CENTRE: hipLaunchKernelGGL((k_encode420<IN10, OUT10, ENC_CENTRE>), grid, block, 0, stream, p); break;
    case ENC_LEFT: hipLaunchKernelGGL((k_encode420<IN10, OUT10, ENC_LEFT>), grid, block, 0, stream, p); break;
    case ENC_TOPLEFT: hipLaunchKernelGGL((k_encode420<IN10, OUT10, ENC_TOPLEFT>), grid, block, 0, stream, p); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t LaunchEncode420(const EncodeParams &params, bool in10, bool out10, int siting, hipStream_t stream, int n_frames)
{
    EncodeParams p = params;
    if (p.w < 2 || p.h < 2 || ((p.w | p.h) & 1) || n_frames < 1 || (n_frames > 1 && !p.frames)) return hipErrorInvalidValue;
    constexpr int kMaxZ = 65535;                        // the grid's z extent
    for (int at = 0; at < n_frames; at += kMaxZ) {
        if (params.frames) p.frames = params.frames + at;
        const dim3 grid((unsigned)((p.w + 255) / 256), (unsigned)((p.h / 2 + 3) / 4), (unsigned)std::min(kMaxZ, n_frames - at));
        const hipError_t e = in10 ? (out10 ? LaunchSiting<true, true>(p, siting, grid, stream) : LaunchSiting<true, false>(p, siting, grid, stream))
                                  : (out10 ? LaunchSiting<false, true>(p, siting, grid, stream) : LaunchSiting<false, false>(p, siting, grid, stream));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace mpcvr
