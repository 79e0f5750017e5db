// vp_encode.h — EXTENSION (include/mpcvr.h: mpcvr_encode_pass / mpcvr_render_yuv): a rendered frame of 32-bit RGB texels written as NV12 or P010
// for a video encoder.  The reference has no RGB -> YCbCr path (its frames end in a swap chain), so there is no reference line to cite: the
// definition is the integer arithmetic of include/mpcvr.h, modelled bit for bit by tests/encode_model.py.
// The kernel's parameters and its launcher (the coefficients come from PlanEncode, vp_plan.h); nothing here is shared with the frame path's kernels.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "vp_plan.h"

namespace mpcvr {

constexpr int kEncodeShift = 16;                       // S: fractional bits of the coefficients
enum EncodeSiting { ENC_CENTRE = 0, ENC_LEFT = 1, ENC_TOPLEFT = 2 };      // MPEG-1 / MPEG-2 / co-sited chroma: tap weights sum to 4 / 8 / 16

// The integers of include/mpcvr.h (mpcvr_plan_encode): the inverse, in double by the adjugate, of what ComputeColorMatrix plans for
// (out_cformat, extfmt) with a neutral ProcAmp, scaled from input codes to output codes and rounded at kEncodeShift fractional bits.
// Host only, no device work; implemented in vp_plan.cpp beside ComputeColorMatrix (declared here: vp_plan.h is part of every fused
// kernel's translation unit, this header of none).
struct EncodePlan {
    int32_t coef[9];             // row-major: rows Y, U, V; columns R, G, B
    int32_t off[3];
    int32_t shift;               // kEncodeShift
    int32_t siting;              // EncodeSiting, from the description's chroma field as the convert path reads it for 4:2:0 input
    uint32_t extfmt;             // the description after SpecifyExtendedFormat
    bool in10, out10;            // MPCVR_OUT_RGB10A2 source / P010 output
};
// out_cformat: MPCVR_CF_NV12 | MPCVR_CF_P010; src_fmt: MPCVR_OUT_*; w x h: the surface (SpecifyExtendedFormat's matrix default depends
// on it).  false: another output or source format, or a description that plans as RGB (value == 0)
bool PlanEncode(int out_cformat, int src_fmt, uint32_t extfmt, int w, int h, EncodePlan *plan);

// The layout integers of include/mpcvr.h (mpcvr_plan_batch_yuv): the context-owned RGB surface a batch is rendered into on its way to the
// planes, and how a batch of n frames is cut into chunks under a budget of bytes.  Host only (vp_plan.cpp).  false: n <= 0 or a window
// that is odd or outside 2 .. 32768
struct BatchYuvLayout : ChunkLayout { int32_t surfacePitch; };
bool PlanBatchYuv(int w, int h, int n, size_t budget, BatchYuvLayout *out);
// the same three formulas for a window of any parity, 1 .. 32768 (mpcvr_plan_batch_tensor: the tensor pass has no 2x2 blocks)
bool PlanBatchTensor(int w, int h, int n, size_t budget, BatchYuvLayout *out);

// one frame of a launch with a frame dimension: its source surface and its two planes (pitches, size and format are the launch's)
struct EncodeFrame { const uint8_t *src; uint8_t *y, *uv; };

struct EncodeParams {
    const uint8_t *src; int src_pitch;                 // w x h texels of 4 bytes
    uint8_t *y; int y_pitch;                           // h rows of w components
    uint8_t *uv; int uv_pitch;                         // h / 2 rows of w / 2 (U, V) pairs
    int w, h;                                          // even, >= 2
    int32_t coef[9], off[3];                           // rows Y, U, V; columns R, G, B
    int src16;                                         // source and its pitch on 16 bytes: a lane with four columns takes one 16-byte load per row
    int dst8;                                          // P010: both planes and pitches on 8 bytes: one 8-byte store per row piece (else two of 4)
    // DEVICE table of n_frames {src, y, uv} rows, frame = blockIdx.z (the convention of the FusedFrame tables, vp_launch.h); null: one frame,
    // src / y / uv above.  With a table src16 and dst8 hold only if EVERY frame of the launch allows them
    const EncodeFrame *frames;
};
// every pointer and pitch a multiple of 4 and the planes apart from each other and from the source (the caller checks: mpcvr_encode_pass,
// mpcvr_process_batch_yuv); one launch for up to 65535 frames (the grid's z extent), one more per further 65535
hipError_t LaunchEncode420(const EncodeParams &p, bool in10, bool out10, int siting, hipStream_t stream, int n_frames = 1);

}  // namespace mpcvr
