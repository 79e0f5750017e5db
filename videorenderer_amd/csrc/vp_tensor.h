// vp_tensor.h — EXTENSION (include/mpcvr.h: mpcvr_tensor_pass / mpcvr_render_tensor / mpcvr_process_batch_tensor): a rendered frame of 32-bit
// RGB texels written as the float tensor a model takes (fp32 / fp16 / bf16; C,H,W or H,W,C; RGB or BGR; value = code * scale + bias per
// channel).  The reference has no float output, so there is no reference line to cite: the definition is the text of include/mpcvr.h, the
// arithmetic vp_tensor_core.h, modelled bit for bit by tests/tensor_model.py.
// The kernel's parameters and its launcher; nothing here is shared with the frame path's kernels.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "vp_tensor_core.h"

namespace mpcvr {

// The tile of one workgroup: kTensorWaves wavefronts, each kTensorWaveRows consecutive rows of kTensorWaveCols columns (64 lanes x 4).
constexpr int kTensorWaveCols = 256;
constexpr int kTensorWaves = 4;
constexpr int kTensorWaveRows = 2;
constexpr int kTensorGroupCols = kTensorWaveCols;
constexpr int kTensorGroupRows = kTensorWaves * kTensorWaveRows;

constexpr int TensorElementSize(int dtype) { return dtype == TN_F32 ? 4 : 2; }
// the bytes of one vector store: four elements (a lane's four columns of one plane; a quarter of a lane's share of an interleaved row piece)
constexpr int TensorVectorBytes(int dtype) { return 4 * TensorElementSize(dtype); }

// one frame of a launch with a frame dimension: its source surface and its tensor (pitches, size, formats and factors are the launch's)
struct TensorFrame { const uint8_t *src; uint8_t *dst; };

struct TensorParams {
    const uint8_t *src; int src_pitch;                 // w x h texels of 4 bytes
    uint8_t *dst;                                      // channel 0, row 0, column 0
    int64_t row_pitch, plane_pitch;                    // bytes; plane_pitch for TN_PLANAR only
    int w, h;
    float scale[3], bias[3];                           // for R, G, B of the picture
    int bgr;                                           // tensor channel 0, 1, 2 = B, G, R instead of R, G, B
    int src16;                                         // source and its pitch on 16 bytes: a lane with four columns inside the surface takes one 16-byte load
    int dstvec;                                        // dst and its pitches on TensorVectorBytes: vector stores where the columns allow, element stores otherwise
    // DEVICE table of n_frames {src, dst} rows, frame = blockIdx.z (the EncodeFrame convention, vp_encode.h); null: one frame, src / dst
    // above.  With a table src16 and dstvec hold only if EVERY frame of the launch allows them
    const TensorFrame *frames;
};
// src and src_pitch multiples of 4, dst and its pitches multiples of the element size, the planes apart from each other and from the source
// (the caller checks: TensorSurface, hip_video_processor_ext.cpp); one launch for up to 65535 frames (the grid's z extent), one more per further 65535
hipError_t LaunchTensor(const TensorParams &p, bool in10, int dtype, int layout, hipStream_t stream, int n_frames = 1);

// ---- host only, no device work (vp_plan.cpp) ----
// the stored bits of one element (mpcvr_plan_tensor_value).  false: another dtype or src_fmt, a code beyond the format's, a factor TensorFactorOk refuses
bool PlanTensorValue(int dtype, int src_fmt, uint32_t code, float scale, float bias, uint32_t *bits);

}  // namespace mpcvr
