// vp_tensor_in.hip — EXTENSION: k_sample_from_tensor, the float tensor a model leaves -> a planar RGB sample the convert path reads
// (vp_tensor_in.h; definition: include/mpcvr.h, mpcvr_sample_pass; arithmetic: vp_tensor_core.h, SampleCode; bit-exact model:
// tests/tensor_in_model.py).  There is no reference line to cite: the reference has no float input.
//
// Data flow.  The kernel is k_tensor (vp_tensor.hip) turned round: memory-bound and read-dominated (12 or 6 bytes in, 3 or 6 out per pixel)
// with no reuse at all:
//   * a lane owns 4 columns of kSampleWaveRows rows, a wavefront 256 columns, a workgroup of kSampleWaves wavefronts kSampleGroupRows rows;
//     every load of every row is issued before the first conversion;
//   * C,H,W: a lane's four elements of a plane are one 16-byte (fp32) / 8-byte (fp16, bf16) load where the tensor and its pitches are on
//     that many bytes and the four columns lie inside the picture — a wavefront instruction reads 1 KiB / 512 contiguous bytes of one
//     plane's row; element loads at clamped columns otherwise;
//   * H,W,C: a lane's four pixels are 48 / 24 contiguous bytes, so a load per lane would touch every cache line of the piece with a third
//     of its bytes per instruction.  The wavefront's row piece (768 elements) is loaded as three vectors at (q * 64 + lane) * 4, q = 0 .. 2
//     — each instruction covers 1 KiB / 512 contiguous bytes — and goes through LDS of the wavefront's own: every lane writes the three
//     vectors it loaded, then reads back the three that hold its 12 elements.  A group of four that reaches past the row's last element,
//     or a tensor off the vector grid, is read as element loads at clamped positions;
//   * per element: widen, flush, one multiply, one add (never contracted: SampleValue), compare, round.  Which tensor channel is R / B
//     is a wave-uniform select (p.bgr);
//   * stores: a lane's four codes of a plane are one 8-byte (16-bit components) / 4-byte (8-bit) store where sample and pitch are on that
//     many bytes; element stores otherwise and in the lane that holds the last columns of a width that is no multiple of 4.  Stores are
//     plain: the convert path reads the sample next, and plain stores keep their lines in the L2 of the XCD;
//   * a batch (mpcvr_process_batch_from_tensors) is one launch: blockIdx.z is the frame, its {src, dst} row of SampleParams::frames is
//     read with scalar loads as in k_tensor.
// All address arithmetic is 64-bit: pitches are int64_t and planes and rows may lie more than 4 GiB apart.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "vp_tensor_in.h"

namespace mpcvr {
namespace {

typedef uint32_t si_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t si_u2 __attribute__((ext_vector_type(2)));

// four elements as one vector: 16 bytes of fp32, 8 bytes of two packed pairs
template <int DTYPE> struct In4;
template <> struct In4<TN_F32> {
    typedef si_u4 T;
    static __device__ __forceinline__ uint32_t Get(T v, int j) { return v[j]; }
    static __device__ __forceinline__ T Set(T v, int j, uint32_t bits) { v[j] = bits; return v; }
    static __device__ __forceinline__ uint32_t LoadOne(const uint8_t *at) { return *(const uint32_t *)at; }
};
template <int DTYPE> struct In4 {
    typedef si_u2 T;
    static __device__ __forceinline__ uint32_t Get(T v, int j) { return (v[j >> 1] >> (16 * (j & 1))) & 0xffffu; }
    static __device__ __forceinline__ T Set(T v, int j, uint32_t bits) { v[j >> 1] |= bits << (16 * (j & 1)); return v; }
    static __device__ __forceinline__ uint32_t LoadOne(const uint8_t *at) { return *(const uint16_t *)at; }
};

template <int DTYPE, int LAYOUT, int BYTES>
__global__ __launch_bounds__(64 * kSampleWaves) void k_sample_from_tensor(SampleParams p)
{
    constexpr int ES = TensorElementSize(DTYPE), VB = TensorVectorBytes(DTYPE);
    typedef In4<DTYPE> V;
    typedef typename V::T VT;
    // (H,W,C only) a wavefront's row piece: 768 elements = 192 vectors, its own — no other wavefront reads or writes it, no barrier
    __shared__ VT piece[LAYOUT == TN_INTERLEAVED ? kSampleWaves : 1][LAYOUT == TN_INTERLEAVED ? 3 * 64 : 1];

    const int lane = threadIdx.x, wv = threadIdx.y;
    const int row0 = ((int)blockIdx.y * kSampleWaves + wv) * kSampleWaveRows;       // the same for a whole wavefront
    if (row0 >= p.h) return;
    const int xw = (int)blockIdx.x * kSampleWaveCols, x0 = xw + lane * 4;
    const bool full = x0 + 4 <= p.w, any = x0 < p.w;

    // the frame: from the arguments, or its row of the table (uniform: blockIdx.z) — as k_tensor reads it
    uintptr_t a_src = (uintptr_t)p.src, a_dst = (uintptr_t)p.dst;
    asm volatile("" : "+s"(a_src), "+s"(a_dst));
    if (p.frames) {
        typedef const SampleFrame __attribute__((address_space(4))) *ConstRow;
        const ConstRow f = (ConstRow)(uintptr_t)(p.frames + blockIdx.z);
        a_src = (uintptr_t)f->src; a_dst = (uintptr_t)f->dst;
    }
    typedef uint8_t __attribute__((address_space(1))) *GlobalBytes;
    const uint8_t *src = (const uint8_t *)(GlobalBytes)a_src;
    uint8_t *dst = (uint8_t *)(GlobalBytes)a_dst;

    // the loads.  C,H,W: t[i][c] = the lane's four columns of tensor channel c.  H,W,C: t[i][q] = elements (q * 64 + lane) * 4 .. + 3 of
    // the wavefront's row piece
    VT t[kSampleWaveRows][3] = {};
    const int nvalid = 3 * min(kSampleWaveCols, p.w - xw);                          // (H,W,C) elements of the row piece
#pragma unroll
    for (int i = 0; i < kSampleWaveRows; i++) {
        if (row0 + i >= p.h) break;                    // (uniform)
        const uint8_t *const row = src + (int64_t)(row0 + i) * p.row_pitch;
        if (LAYOUT == TN_PLANAR) {
            if (!any) continue;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const uint8_t *const s = row + (int64_t)c * p.plane_pitch;
                if (p.srcvec && full) t[i][c] = *(const VT *)(s + (int64_t)x0 * ES);
                else {
#pragma unroll
                    for (int j = 0; j < 4; j++) t[i][c] = V::Set(t[i][c], j, V::LoadOne(s + (int64_t)min(x0 + j, p.w - 1) * ES));
                }
            }
        } else {
            const uint8_t *const s0 = row + (int64_t)xw * (3 * ES);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const int idx = q * 64 + lane;
                if (idx * 4 >= nvalid) continue;
                if (p.srcvec && idx * 4 + 4 <= nvalid) t[i][q] = *(const VT *)(s0 + (int64_t)idx * VB);
                else {
#pragma unroll
                    for (int j = 0; j < 4; j++) t[i][q] = V::Set(t[i][q], j, V::LoadOne(s0 + (int64_t)min(idx * 4 + j, nvalid - 1) * ES));
                }
            }
        }
    }

#pragma unroll
    for (int i = 0; i < kSampleWaveRows; i++) {
        if (row0 + i >= p.h) break;                    // (uniform)
        uint32_t e[3][4];                              // [tensor channel][column]: element bits
        if (LAYOUT == TN_PLANAR) {
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int j = 0; j < 4; j++) e[c][j] = V::Get(t[i][c], j);
        } else {
            VT *const mine = piece[wv];
#pragma unroll
            for (int q = 0; q < 3; q++) mine[q * 64 + lane] = t[i][q];
            // (the wavefront's LDS accesses execute in order; the fences keep the compiler from moving them across each other)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // the lane's 12 elements in row order: column, then channel
            const VT a = mine[lane * 3 + 0], b = mine[lane * 3 + 1], c = mine[lane * 3 + 2];
#pragma unroll
            for (int m = 0; m < 12; m++) {
                const VT &v = m < 4 ? a : m < 8 ? b : c;
                e[m % 3][m / 3] = V::Get(v, m & 3);
            }
            // (the next row's writes stay behind these reads)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (!any) continue;
        uint8_t *const drow = dst + (int64_t)(row0 + i) * p.dst_pitch + (int64_t)x0 * BYTES;
#pragma unroll
        for (int pl = 0; pl < 3; pl++) {               // the sample's planes are G, B, R; picture channel k = 0 R, 1 G, 2 B is tensor channel k, or 2 - k (p.bgr)
            const int k = pl == 0 ? 1 : pl == 1 ? 2 : 0;
            uint32_t code[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t bits = k == 1 ? e[1][j] : k == 0 ? (p.bgr ? e[2][j] : e[0][j]) : (p.bgr ? e[0][j] : e[2][j]);
                code[j] = SampleCode<DTYPE>(bits, p.scale[k], p.bias[k], p.maxcode);
            }
            uint8_t *const d = drow + (int64_t)pl * p.dst_plane;
            if (p.dstvec && full) {
                if (BYTES == 2) *(si_u2 *)d = si_u2{code[0] | code[1] << 16, code[2] | code[3] << 16};
                else *(uint32_t *)d = code[0] | code[1] << 8 | code[2] << 16 | code[3] << 24;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (x0 + j >= p.w) break;
                    if (BYTES == 2) *(uint16_t *)(d + 2 * j) = (uint16_t)code[j];
                    else d[j] = (uint8_t)code[j];
                }
            }
        }
    }
}

template <int DTYPE, int LAYOUT>
hipError_t LaunchBytes(const SampleParams &p, int bytes, dim3 grid, hipStream_t stream)
{
    const dim3 block(64, kSampleWaves);
    switch (bytes) {
    case 1: hipLaunchKernelGGL((k_sample_from_tensor<DTYPE, LAYOUT, 1>), grid, block, 0, stream, p); break;
    case 2: hipLaunchKernelGGL((k_sample_from_tensor<DTYPE, LAYOUT, 2>), grid, block, 0, stream, p); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int DTYPE>
hipError_t LaunchLayout(const SampleParams &p, int layout, int bytes, dim3 grid, hipStream_t stream)
{
    switch (layout) {
    case TN_PLANAR: return LaunchBytes<DTYPE, TN_PLANAR>(p, bytes, grid, stream);
    case TN_INTERLEAVED: return LaunchBytes<DTYPE, TN_INTERLEAVED>(p, bytes, grid, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t LaunchSampleFromTensor(const SampleParams &params, int dtype, int layout, int bytes, hipStream_t stream, int n_frames)
{
    SampleParams p = params;
    if (p.w < 1 || p.h < 1 || n_frames < 1 || (n_frames > 1 && !p.frames) || (!p.frames && (!p.src || !p.dst))) return hipErrorInvalidValue;
    constexpr int kMaxZ = 65535;                        // the grid's z extent
    for (int at = 0; at < n_frames; at += kMaxZ) {
        if (params.frames) p.frames = params.frames + at;
        const dim3 grid((unsigned)((p.w + kSampleGroupCols - 1) / kSampleGroupCols), (unsigned)((p.h + kSampleGroupRows - 1) / kSampleGroupRows),
                        (unsigned)std::min(kMaxZ, n_frames - at));
        hipError_t e;
        switch (dtype) {
        case TN_F32: e = LaunchLayout<TN_F32>(p, layout, bytes, grid, stream); break;
        case TN_F16: e = LaunchLayout<TN_F16>(p, layout, bytes, grid, stream); break;
        case TN_BF16: e = LaunchLayout<TN_BF16>(p, layout, bytes, grid, stream); break;
        default: return hipErrorInvalidValue;
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace mpcvr
