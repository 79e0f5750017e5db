// vp_deint.hip — EXTENSION: k_deint, motion-adaptive deinterlacing of the planes of a sample at field rate (vp_deint.h; definition:
// include/mpcvr.h, mpcvr_deint_pass; arithmetic: vp_deint_core.h, DeintComponent; bit-exact model: tests/deint_model.py).  There is no
// reference line to cite: the reference hands deinterlacing to the fixed-function video processor.
//
// Data flow.  A vertical stencil over three frames: per output frame 2.5 frames are read (the frame holding the other field contributes
// only its lines of the shown parity's neighbours) and one is written.  Per missing component twenty sums of absolute differences,
// five averages and a dozen min / max: at 8 bits the vector ALU, not memory, bounds the kernel.
//   * a wavefront whose 256 steps all lie inside the plane, in a launch with srcvec and dstvec, runs Strip with the literal `true` for both
//     choices: no per-lane branch, one load per row.  Every other wavefront (the last of a row of a width that is no multiple of 256, a
//     launch off the vector grid) runs the same Strip with the choice per lane;
//   * |a - b| + c is v_sad_u16 on words whose upper halves are empty (DeintSad, vp_deint_core.h): one instruction where the plain form
//     takes three;
//   * columns are counted in channel steps (cs components: 1, or one U,V pair).  A lane owns kDeintLaneSteps = 4 consecutive steps of a row
//     — 4 cs bytes-per-component bytes: one 4-, 8- or 16-byte load per row where every source plane of the launch and its pitch are on that
//     many bytes and the four steps lie inside the plane (p.srcvec, chosen per launch); component loads at clamped columns otherwise.  A
//     wavefront instruction then reads 256 / 512 / 1024 contiguous bytes of one row;
//   * a wavefront walks down a strip of kDeintStripRows rows, one row pair (a kept line and a missing line) per step, and keeps in registers
//     what the next pair needs again: cur at y + 1 becomes cur at y - 1, prev / next at y + 1 become those at y - 1, and with the interlacing
//     check A and B at y, y + 2 become those at y - 2, y.  A step loads five rows (three without the check: A, B at y are then loaded, not
//     carried), the first step of a strip all of them;
//   * the directional scores reach three steps to either side: a lane's halo of a cur row comes from its two neighbours in the wavefront
//     (two packed words each way, ds_bpermute through __shfl_up / __shfl_down), and only lanes 0 and 63 load theirs (three clamped steps);
//     a cur row gets its halo once, when it is loaded, and keeps it when it is carried;
//   * lanes past the plane's last step load clamped columns like everyone (their values are the right-hand clamp of their left neighbour's
//     halo) and store nothing: all 64 lanes stay in the cross-lane operations;
//   * kept lines are stored from the registers that hold them as cur at y - 1 / y + 1; stores are one vector per lane and row where every
//     destination plane and its pitch allow (p.dstvec), component stores otherwise and in the lane holding the last steps of a partial group;
//   * keep, first and the four pointers are per frame: by value, or the frame's row of DeintParams::frames read with scalar loads
//     (blockIdx.z = frame * n_planes + plane), as k_sample_from_tensor reads its table.
// All address arithmetic is 64-bit: pitches and plane offsets are int64_t and rows may lie more than 4 GiB apart.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "vp_deint.h"

namespace mpcvr {
namespace {

constexpr int LS = kDeintLaneSteps, R = kDeintReach, EW = LS + 2 * R;
static_assert(LS == 4 && R == 3, "the halo exchange packs four steps into two words and takes three from each neighbour");

typedef uint32_t di_u2 __attribute__((ext_vector_type(2)));
typedef uint32_t di_u4 __attribute__((ext_vector_type(4)));

// a lane's LS * CS components of a row as one vector
template <int NB> struct DiVec;
template <> struct DiVec<4> {
    typedef uint32_t T;
    static __device__ __forceinline__ uint32_t Word(T v, int) { return v; }
    static __device__ __forceinline__ T Make(const uint32_t *w) { return w[0]; }
};
template <> struct DiVec<8> {
    typedef di_u2 T;
    static __device__ __forceinline__ uint32_t Word(T v, int i) { return v[i]; }
    static __device__ __forceinline__ T Make(const uint32_t *w) { return di_u2{w[0], w[1]}; }
};
template <> struct DiVec<16> {
    typedef di_u4 T;
    static __device__ __forceinline__ uint32_t Word(T v, int i) { return v[i]; }
    static __device__ __forceinline__ T Make(const uint32_t *w) { return di_u4{w[0], w[1], w[2], w[3]}; }
};

template <int BYTES, int CS>
__device__ __forceinline__ int LoadOne(const uint8_t *row, int step, int c, int mask)
{
    const int64_t comp = (int64_t)step * CS + c;
    return (int)(BYTES == 2 ? (uint32_t)*(const uint16_t *)(row + comp * 2) : (uint32_t)row[comp]) & mask;
}

// v[c][j] = channel c of step x0 + j (clamped to the plane's last step)
template <int BYTES, int CS>
__device__ __forceinline__ void LoadRow(const uint8_t *row, int x0, int steps, bool vec, int mask, int (&v)[CS][LS])
{
    constexpr int NB = LS * CS * BYTES;
    if (vec) {
        const typename DiVec<NB>::T t = *(const typename DiVec<NB>::T *)(row + (int64_t)x0 * (CS * BYTES));
#pragma unroll
        for (int j = 0; j < LS; j++)
#pragma unroll
            for (int c = 0; c < CS; c++) {
                const int at = (j * CS + c) * BYTES;
                v[c][j] = (int)((DiVec<NB>::Word(t, at / 4) >> ((at % 4) * 8)) & (BYTES == 1 ? 0xffu : 0xffffu)) & mask;
            }
    } else {
#pragma unroll
        for (int j = 0; j < LS; j++)
#pragma unroll
            for (int c = 0; c < CS; c++) v[c][j] = LoadOne<BYTES, CS>(row, min(x0 + j, steps - 1), c, mask);
    }
}

// e[c][R + j] = v[c][j]; the R steps to either side from the neighbouring lanes, from memory in the wavefront's edge lanes
template <int BYTES, int CS>
__device__ __forceinline__ void WithHalo(const uint8_t *row, int lane, int x0, int steps, int mask, const int (&v)[CS][LS], int (&e)[CS][EW])
{
#pragma unroll
    for (int c = 0; c < CS; c++) {
        const int w0 = v[c][0] | (v[c][1] << 16), w1 = v[c][2] | (v[c][3] << 16);
        const uint32_t l0 = (uint32_t)__shfl_up(w0, 1), l1 = (uint32_t)__shfl_up(w1, 1);
        const uint32_t r0 = (uint32_t)__shfl_down(w0, 1), r1 = (uint32_t)__shfl_down(w1, 1);
        e[c][0] = (int)(l0 >> 16); e[c][1] = (int)(l1 & 0xffffu); e[c][2] = (int)(l1 >> 16);
#pragma unroll
        for (int j = 0; j < LS; j++) e[c][R + j] = v[c][j];
        e[c][R + LS] = (int)(r0 & 0xffffu); e[c][R + LS + 1] = (int)(r0 >> 16); e[c][R + LS + 2] = (int)(r1 & 0xffffu);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < CS; c++)
#pragma unroll
            for (int i = 0; i < R; i++) e[c][i] = LoadOne<BYTES, CS>(row, min(max(x0 - R + i, 0), steps - 1), c, mask);
    }
    if (lane == 63) {
#pragma unroll
        for (int c = 0; c < CS; c++)
#pragma unroll
            for (int i = 0; i < R; i++) e[c][R + LS + i] = LoadOne<BYTES, CS>(row, min(x0 + LS + i, steps - 1), c, mask);
    }
}

template <int BYTES, int CS>
__device__ __forceinline__ void StoreRow(uint8_t *row, int x0, int steps, bool vec, const int (&v)[CS][LS])
{
    constexpr int NB = LS * CS * BYTES;
    if (x0 >= steps) return;
    if (vec) {
        uint32_t w[NB / 4] = {};
#pragma unroll
        for (int j = 0; j < LS; j++)
#pragma unroll
            for (int c = 0; c < CS; c++) {
                const int at = (j * CS + c) * BYTES;
                w[at / 4] |= (uint32_t)v[c][j] << ((at % 4) * 8);
            }
        *(typename DiVec<NB>::T *)(row + (int64_t)x0 * (CS * BYTES)) = DiVec<NB>::Make(w);
    } else {
#pragma unroll
        for (int j = 0; j < LS; j++) {
            if (x0 + j >= steps) break;
#pragma unroll
            for (int c = 0; c < CS; c++) {
                const int64_t comp = (int64_t)(x0 + j) * CS + c;
                if (BYTES == 2) *(uint16_t *)(row + comp * 2) = (uint16_t)v[c][j];
                else row[comp] = (uint8_t)v[c][j];
            }
        }
    }
}

template <int CS>
__device__ __forceinline__ void Centre(const int (&e)[CS][EW], int (&v)[CS][LS])
{
#pragma unroll
    for (int c = 0; c < CS; c++)
#pragma unroll
        for (int j = 0; j < LS; j++) v[c][j] = e[c][R + j];
}

template <int CS, int N>
__device__ __forceinline__ void Copy(int (&d)[CS][N], const int (&s)[CS][N])
{
#pragma unroll
    for (int c = 0; c < CS; c++)
#pragma unroll
        for (int j = 0; j < N; j++) d[c][j] = s[c][j];
}

// one strip of one wavefront.  lv / sv: this lane takes vector loads / stores; the kernel passes the literal `true` for a wavefront whose 256
// steps all lie inside the plane of a launch with srcvec and dstvec, so that the choice costs nothing there
template <int BYTES, int CS, int CHECK>
__device__ __forceinline__ void Strip(const uint8_t *__restrict__ prev, const uint8_t *__restrict__ cur, const uint8_t *__restrict__ next, uint8_t *__restrict__ dst,
                                      int first, int keep, int64_t sp, int64_t dp, int lines, int steps, int mask, int r0, int x0, int lane, bool lv, bool sv)
{
    // the frames holding the missing-parity field just before and just after the shown field
    const uint8_t *const A = first ? prev : cur, *const B = first ? cur : next;
    int cu[CS][EW] = {}, cd[CS][EW] = {};
    int a0[CS][LS] = {}, a1[CS][LS] = {}, a2[CS][LS] = {}, b0[CS][LS] = {}, b1[CS][LS] = {}, b2[CS][LS] = {};
    int pu[CS][LS] = {}, pd[CS][LS] = {}, nu[CS][LS] = {}, nd[CS][LS] = {};
    int t[CS][LS];

#pragma unroll
    for (int it = 0; it < kDeintStripRows / 2; it++) {
        const bool fresh = it == 0;
        const int base = r0 + 2 * it;
        if (base >= lines) break;                      // (uniform)
        const int y = base + (keep ? 0 : 1);           // the missing line of the pair
        if (y >= lines) {                              // keep == 0 and an odd number of lines: the last line is kept and has no missing line below
            if (fresh) LoadRow<BYTES, CS>(cur + (int64_t)base * sp, x0, steps, lv, mask, t);
            else Centre<CS>(cd, t);                    // (the pair above loaded cur[base] as its line below)
            StoreRow<BYTES, CS>(dst + (int64_t)base * dp, x0, steps, sv, t);
            break;
        }
        const int ym = y - 1 >= 0 ? y - 1 : y + 1, yp = y + 1 < lines ? y + 1 : y - 1;
        const bool chk = CHECK && y - 2 >= 0 && y + 2 < lines;
        if (fresh) {
            LoadRow<BYTES, CS>(cur + (int64_t)ym * sp, x0, steps, lv, mask, t);
            WithHalo<BYTES, CS>(cur + (int64_t)ym * sp, lane, x0, steps, mask, t, cu);
            LoadRow<BYTES, CS>(prev + (int64_t)ym * sp, x0, steps, lv, mask, pu);
            LoadRow<BYTES, CS>(next + (int64_t)ym * sp, x0, steps, lv, mask, nu);
            if (CHECK && y - 2 >= 0) {
                LoadRow<BYTES, CS>(A + (int64_t)(y - 2) * sp, x0, steps, lv, mask, a0);
                LoadRow<BYTES, CS>(B + (int64_t)(y - 2) * sp, x0, steps, lv, mask, b0);
            }
        } else {                                       // (y >= 2 here: ym = y - 1 is the pair above's line below)
            Copy<CS, EW>(cu, cd); Copy<CS, LS>(pu, pd); Copy<CS, LS>(nu, nd);
            if (CHECK) { Copy<CS, LS>(a0, a1); Copy<CS, LS>(b0, b1); Copy<CS, LS>(a1, a2); Copy<CS, LS>(b1, b2); }
        }
        if (fresh || !CHECK) {
            LoadRow<BYTES, CS>(A + (int64_t)y * sp, x0, steps, lv, mask, a1);
            LoadRow<BYTES, CS>(B + (int64_t)y * sp, x0, steps, lv, mask, b1);
        }
        LoadRow<BYTES, CS>(cur + (int64_t)yp * sp, x0, steps, lv, mask, t);
        WithHalo<BYTES, CS>(cur + (int64_t)yp * sp, lane, x0, steps, mask, t, cd);
        LoadRow<BYTES, CS>(prev + (int64_t)yp * sp, x0, steps, lv, mask, pd);
        LoadRow<BYTES, CS>(next + (int64_t)yp * sp, x0, steps, lv, mask, nd);
        if (CHECK && y + 2 < lines) {
            LoadRow<BYTES, CS>(A + (int64_t)(y + 2) * sp, x0, steps, lv, mask, a2);
            LoadRow<BYTES, CS>(B + (int64_t)(y + 2) * sp, x0, steps, lv, mask, b2);
        }

        int o[CS][LS];
#pragma unroll
        for (int c = 0; c < CS; c++)
#pragma unroll
            for (int j = 0; j < LS; j++)
                o[c][j] = DeintComponent(&cu[c][R + j], &cd[c][R + j], a1[c][j], b1[c][j], pu[c][j], pd[c][j], nu[c][j], nd[c][j],
                                         chk, a0[c][j], b0[c][j], a2[c][j], b2[c][j]);
        StoreRow<BYTES, CS>(dst + (int64_t)y * dp, x0, steps, sv, o);
        // the kept line of the pair, from the registers that hold it
        if (!keep) { Centre<CS>(cu, t); StoreRow<BYTES, CS>(dst + (int64_t)(y - 1) * dp, x0, steps, sv, t); }
        else if (y + 1 < lines) { Centre<CS>(cd, t); StoreRow<BYTES, CS>(dst + (int64_t)(y + 1) * dp, x0, steps, sv, t); }
    }
}

template <int BYTES, int CS, int CHECK>
__global__ __launch_bounds__(64 * kDeintWaves) void k_deint(DeintParams p)
{
    const int lane = threadIdx.x, wv = threadIdx.y;
    // the plane and the frame (uniform: blockIdx.z)
    const int fi = (int)blockIdx.z / p.n_planes, pi = (int)blockIdx.z - fi * p.n_planes;
    DeintLaunchPlane pl = p.plane[0];
    if (pi == 1) pl = p.plane[1];
    if (pi == 2) pl = p.plane[2];
    const int lines = pl.lines, steps = pl.steps, mask = p.mask;
    const int r0 = ((int)blockIdx.y * kDeintWaves + wv) * kDeintStripRows;          // the same for a whole wavefront
    const int xw = (int)blockIdx.x * kDeintWaveCols;
    if (r0 >= lines || xw >= steps) return;            // (a smaller plane of the launch)

    uintptr_t a_prev = (uintptr_t)p.one.prev, a_cur = (uintptr_t)p.one.cur, a_next = (uintptr_t)p.one.next, a_dst = (uintptr_t)p.one.dst;
    int keep = p.one.keep, first = p.one.first;
    if (p.frames) {
        typedef const DeintFrame __attribute__((address_space(4))) *ConstRow;
        const ConstRow f = (ConstRow)(uintptr_t)(p.frames + fi);
        a_prev = (uintptr_t)f->prev; a_cur = (uintptr_t)f->cur; a_next = (uintptr_t)f->next; a_dst = (uintptr_t)f->dst;
        keep = f->keep; first = f->first;
    }
    typedef uint8_t __attribute__((address_space(1))) *GlobalBytes;
    const uint8_t *const prev = (const uint8_t *)(GlobalBytes)a_prev + pl.src_off;
    const uint8_t *const cur = (const uint8_t *)(GlobalBytes)a_cur + pl.src_off;
    const uint8_t *const next = (const uint8_t *)(GlobalBytes)a_next + pl.src_off;
    uint8_t *const dst = (uint8_t *)(GlobalBytes)a_dst + pl.dst_off;
    const int x0 = xw + lane * LS;
    if (p.srcvec && p.dstvec && xw + kDeintWaveCols <= steps)      // (uniform) every lane of the wavefront on the vector paths
        Strip<BYTES, CS, CHECK>(prev, cur, next, dst, first, keep, pl.src_pitch, pl.dst_pitch, lines, steps, mask, r0, x0, lane, true, true);
    else {
        const bool full = x0 + LS <= steps;
        Strip<BYTES, CS, CHECK>(prev, cur, next, dst, first, keep, pl.src_pitch, pl.dst_pitch, lines, steps, mask, r0, x0, lane, p.srcvec && full, p.dstvec && full);
    }
}

template <int BYTES, int CS>
hipError_t LaunchMode(const DeintParams &p, int mode, dim3 grid, hipStream_t stream)
{
    const dim3 block(64, kDeintWaves);
    switch (mode) {
    case DI_ADAPTIVE: hipLaunchKernelGGL((k_deint<BYTES, CS, 1>), grid, block, 0, stream, p); break;
    case DI_ADAPTIVE_NOCHECK: hipLaunchKernelGGL((k_deint<BYTES, CS, 0>), grid, block, 0, stream, p); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t LaunchDeint(const DeintParams &params, int bytes, int cs, int mode, hipStream_t stream, int n_frames)
{
    DeintParams p = params;
    if ((bytes != 1 && bytes != 2) || (cs != 1 && cs != 2)) return hipErrorInvalidValue;
    if (p.n_planes < 1 || p.n_planes > kDeintMaxPlanes || n_frames < 1 || (n_frames > 1 && !p.frames)) return hipErrorInvalidValue;
    if (!p.frames && (!p.one.prev || !p.one.cur || !p.one.next || !p.one.dst)) return hipErrorInvalidValue;
    int steps = 0, lines = 0;
    for (int i = 0; i < p.n_planes; i++) {
        if (p.plane[i].steps < 1 || p.plane[i].lines < 2) return hipErrorInvalidValue;
        steps = std::max(steps, p.plane[i].steps); lines = std::max(lines, p.plane[i].lines);
    }
    const int lot = 65535 / p.n_planes;                 // frames per launch: the grid's z extent holds frame x plane
    for (int at = 0; at < n_frames; at += lot) {
        if (params.frames) p.frames = params.frames + at;
        const dim3 grid((unsigned)((steps + kDeintGroupCols - 1) / kDeintGroupCols), (unsigned)((lines + kDeintGroupRows - 1) / kDeintGroupRows),
                        (unsigned)(std::min(lot, n_frames - at) * p.n_planes));
        hipError_t e;
        switch (bytes * 2 + cs) {
        case 1 * 2 + 1: e = LaunchMode<1, 1>(p, mode, grid, stream); break;
        case 1 * 2 + 2: e = LaunchMode<1, 2>(p, mode, grid, stream); break;
        case 2 * 2 + 1: e = LaunchMode<2, 1>(p, mode, grid, stream); break;
        case 2 * 2 + 2: e = LaunchMode<2, 2>(p, mode, grid, stream); break;
        default: return hipErrorInvalidValue;
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace mpcvr
