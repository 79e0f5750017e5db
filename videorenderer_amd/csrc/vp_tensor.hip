// vp_tensor.hip — EXTENSION: k_tensor, 32-bit RGB texels -> the float tensor a model takes (vp_tensor.h; definition: include/mpcvr.h,
// mpcvr_tensor_pass; arithmetic: vp_tensor_core.h; bit-exact model: tests/tensor_model.py).  There is no reference line to cite: the
// reference has no float output.
//
// Data flow.  The kernel is memory-bound and write-dominated (4 bytes in, 6 or 12 out per texel) with no reuse at all:
//   * a lane owns 4 columns of kTensorWaveRows rows: one 16-byte load per row where the source, its pitch and every frame are on 16 bytes and
//     the four columns lie inside the surface, dword loads at clamped columns otherwise; every row is loaded before the first is converted;
//   * a wavefront owns 256 columns, a workgroup of kTensorWaves wavefronts kTensorGroupRows rows;
//   * per element: code -> fp32, one multiply, one add (never contracted: TensorValue), one conversion.  Which of R / B goes to tensor
//     channel 0 is a wave-uniform select (p.bgr);
//   * C,H,W: a lane's four elements of a plane are one 16-byte (fp32) / 8-byte (fp16, bf16) store where dst and its pitches are on that many
//     bytes — a wavefront instruction writes 1 KiB / 512 contiguous bytes of one plane's row; element stores otherwise and in the lane that
//     holds the last columns of a width that is no multiple of 4;
//   * H,W,C: a lane's 12 elements are 48 / 24 contiguous bytes, so a store per lane would write a third of every cache line per wavefront
//     instruction.  The wavefront's row piece (768 elements) goes through LDS of its own instead: every lane writes its 12 elements, then
//     reads back four elements at (q * 64 + lane) * 4, q = 0 .. 2 — each of the three store instructions covers 1 KiB / 512 contiguous
//     bytes.  A group of four that reaches past the row's last element, or a tensor off the vector grid, leaves as element stores;
//   * stores are plain: the tensor is read next (by a model), and plain stores keep lines in the L2 of the XCD;
//   * a batch (mpcvr_process_batch_tensor) is one launch: blockIdx.z is the frame, its {src, dst} row of TensorParams::frames is read with
//     scalar loads as in k_encode420.
// All address arithmetic is 64-bit: pitches are int64_t and planes may lie more than 4 GiB apart.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "vp_tensor.h"

namespace mpcvr {
namespace {

typedef uint32_t tn_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t tn_u2 __attribute__((ext_vector_type(2)));

// four elements as one vector: 16 bytes of fp32, 8 bytes of two packed pairs
template <int DTYPE> struct Vec4;
template <> struct Vec4<TN_F32> {
    typedef tn_u4 T;
    static __device__ __forceinline__ T Pack(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return T{a, b, c, d}; }
    static __device__ __forceinline__ uint32_t Get(T v, int j) { return v[j]; }
    static __device__ __forceinline__ void StoreOne(uint8_t *at, uint32_t bits) { *(uint32_t *)at = bits; }
};
template <int DTYPE> struct Vec4 {
    typedef tn_u2 T;
    static __device__ __forceinline__ T Pack(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return T{a | b << 16, c | d << 16}; }
    static __device__ __forceinline__ uint32_t Get(T v, int j) { return (v[j >> 1] >> (16 * (j & 1))) & 0xffffu; }
    static __device__ __forceinline__ void StoreOne(uint8_t *at, uint32_t bits) { *(uint16_t *)at = (uint16_t)bits; }
};

template <bool IN10, int DTYPE, int LAYOUT>
__global__ __launch_bounds__(64 * kTensorWaves) void k_tensor(TensorParams p)
{
    constexpr int ES = TensorElementSize(DTYPE), VB = TensorVectorBytes(DTYPE);
    typedef Vec4<DTYPE> V;
    typedef typename V::T VT;
    // (H,W,C only) a wavefront's row piece: 768 elements = 192 vectors, its own — no other wavefront reads or writes it, no barrier
    __shared__ VT piece[LAYOUT == TN_INTERLEAVED ? kTensorWaves : 1][LAYOUT == TN_INTERLEAVED ? 3 * 64 : 1];

    const int lane = threadIdx.x, wv = threadIdx.y;
    const int row0 = ((int)blockIdx.y * kTensorWaves + wv) * kTensorWaveRows;       // the same for a whole wavefront
    if (row0 >= p.h) return;
    const int xw = (int)blockIdx.x * kTensorWaveCols, x0 = xw + lane * 4;
    const bool full = x0 + 4 <= p.w, any = x0 < p.w;
    const bool vec = p.src16 && full;

    // the frame: from the arguments, or its row of the table (uniform: blockIdx.z) — as k_encode420 reads it
    uintptr_t a_src = (uintptr_t)p.src, a_dst = (uintptr_t)p.dst;
    asm volatile("" : "+s"(a_src), "+s"(a_dst));
    if (p.frames) {
        typedef const TensorFrame __attribute__((address_space(4))) *ConstRow;
        const ConstRow f = (ConstRow)(uintptr_t)(p.frames + blockIdx.z);
        a_src = (uintptr_t)f->src; a_dst = (uintptr_t)f->dst;
    }
    typedef uint8_t __attribute__((address_space(1))) *GlobalBytes;
    const uint8_t *src = (const uint8_t *)(GlobalBytes)a_src;
    uint8_t *dst = (uint8_t *)(GlobalBytes)a_dst;

    uint32_t t[kTensorWaveRows][4] = {};
    if (any) {
#pragma unroll
        for (int i = 0; i < kTensorWaveRows; i++) {
            if (row0 + i >= p.h) break;                // (uniform)
            const uint8_t *row = src + (int64_t)(row0 + i) * p.src_pitch;
            if (vec) {
                const tn_u4 q = *(const tn_u4 *)(row + (int64_t)x0 * 4);
                t[i][0] = q.x; t[i][1] = q.y; t[i][2] = q.z; t[i][3] = q.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) t[i][j] = *(const uint32_t *)(row + (int64_t)min(x0 + j, p.w - 1) * 4);
            }
        }
    }

#pragma unroll
    for (int i = 0; i < kTensorWaveRows; i++) {
        if (row0 + i >= p.h) break;                    // (uniform)
        uint32_t e[3][4];                              // [tensor channel][column]
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t r = TensorElementBits<DTYPE>(TensorCode<IN10>(t[i][j], 0), p.scale[0], p.bias[0]);
            const uint32_t b = TensorElementBits<DTYPE>(TensorCode<IN10>(t[i][j], 2), p.scale[2], p.bias[2]);
            e[1][j] = TensorElementBits<DTYPE>(TensorCode<IN10>(t[i][j], 1), p.scale[1], p.bias[1]);
            e[0][j] = p.bgr ? b : r;
            e[2][j] = p.bgr ? r : b;
        }
        uint8_t *const drow = dst + (int64_t)(row0 + i) * p.row_pitch;
        if (LAYOUT == TN_PLANAR) {
            if (!any) continue;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                uint8_t *const d = drow + (int64_t)c * p.plane_pitch + (int64_t)x0 * ES;
                if (p.dstvec && full) *(VT *)d = V::Pack(e[c][0], e[c][1], e[c][2], e[c][3]);
                else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (x0 + j < p.w) V::StoreOne(d + j * ES, e[c][j]);
                }
            }
        } else {
            VT *const mine = piece[wv];
            // the lane's 12 elements in row order: column, then channel
            mine[lane * 3 + 0] = V::Pack(e[0][0], e[1][0], e[2][0], e[0][1]);
            mine[lane * 3 + 1] = V::Pack(e[1][1], e[2][1], e[0][2], e[1][2]);
            mine[lane * 3 + 2] = V::Pack(e[2][2], e[0][3], e[1][3], e[2][3]);
            // (the wavefront's LDS accesses execute in order; the fences keep the compiler from moving them across each other)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int nvalid = 3 * min(kTensorWaveCols, p.w - xw);                   // elements of the row piece
            uint8_t *const d0 = drow + (int64_t)xw * (3 * ES);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const int idx = q * 64 + lane;
                if (idx * 4 >= nvalid) continue;
                const VT v = mine[idx];
                uint8_t *const d = d0 + (int64_t)idx * VB;
                if (p.dstvec && idx * 4 + 4 <= nvalid) *(VT *)d = v;
                else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (idx * 4 + j < nvalid) V::StoreOne(d + j * ES, V::Get(v, j));
                }
            }
            // (the next row's writes stay behind these reads)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
}

template <bool IN10, int DTYPE>
hipError_t LaunchLayout(const TensorParams &p, int layout, dim3 grid, hipStream_t stream)
{
    const dim3 block(64, kTensorWaves);
    switch (layout) {
    case TN_PLANAR: hipLaunchKernelGGL((k_tensor<IN10, DTYPE, TN_PLANAR>), grid, block, 0, stream, p); break;
    case TN_INTERLEAVED: hipLaunchKernelGGL((k_tensor<IN10, DTYPE, TN_INTERLEAVED>), grid, block, 0, stream, p); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <bool IN10>
hipError_t LaunchDtype(const TensorParams &p, int dtype, int layout, dim3 grid, hipStream_t stream)
{
    switch (dtype) {
    case TN_F32: return LaunchLayout<IN10, TN_F32>(p, layout, grid, stream);
    case TN_F16: return LaunchLayout<IN10, TN_F16>(p, layout, grid, stream);
    case TN_BF16: return LaunchLayout<IN10, TN_BF16>(p, layout, grid, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t LaunchTensor(const TensorParams &params, bool in10, int dtype, int layout, hipStream_t stream, int n_frames)
{
    TensorParams p = params;
    if (p.w < 1 || p.h < 1 || n_frames < 1 || (n_frames > 1 && !p.frames) || (!p.frames && (!p.src || !p.dst))) return hipErrorInvalidValue;
    constexpr int kMaxZ = 65535;                        // the grid's z extent
    for (int at = 0; at < n_frames; at += kMaxZ) {
        if (params.frames) p.frames = params.frames + at;
        const dim3 grid((unsigned)((p.w + kTensorGroupCols - 1) / kTensorGroupCols), (unsigned)((p.h + kTensorGroupRows - 1) / kTensorGroupRows),
                        (unsigned)std::min(kMaxZ, n_frames - at));
        const hipError_t e = in10 ? LaunchDtype<true>(p, dtype, layout, grid, stream) : LaunchDtype<false>(p, dtype, layout, grid, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace mpcvr
