// vp_tensor_in.h — EXTENSION (include/mpcvr.h: mpcvr_sample_pass / mpcvr_copy_sample_tensor / mpcvr_process_batch_from_tensors): the float
// tensor a model leaves (fp32 / fp16 / bf16; C,H,W or H,W,C; RGB or BGR) written as the planar RGB sample the convert path reads directly
// (GBRP8 / GBRP10 / GBRP16; code = round(x * scale + bias) per channel, clamped).  The mirror image of vp_tensor.h; the reference has no
// float input, so there is no reference line to cite: the definition is the text of include/mpcvr.h, the arithmetic vp_tensor_core.h
// (SampleCode), modelled bit for bit by tests/tensor_in_model.py.
// The kernel's parameters and its launcher; nothing here is shared with the frame path's kernels.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "vp_plan.h"
#include "vp_tensor.h"

namespace mpcvr {

// The tile of one workgroup: kSampleWaves wavefronts, each kSampleWaveRows consecutive rows of kSampleWaveCols columns (64 lanes x 4).
constexpr int kSampleWaveCols = 256;
constexpr int kSampleWaves = 4;
constexpr int kSampleWaveRows = 2;
constexpr int kSampleGroupCols = kSampleWaveCols;
constexpr int kSampleGroupRows = kSampleWaves * kSampleWaveRows;

// one frame of a launch with a frame dimension: its tensor and its sample (pitches, size, formats and factors are the launch's)
struct SampleFrame { const uint8_t *src; uint8_t *dst; };

struct SampleParams {
    const uint8_t *src;                                // tensor channel 0, row 0, column 0
    int64_t row_pitch, plane_pitch;                    // of the tensor, bytes; plane_pitch for TN_PLANAR only
    uint8_t *dst;                                      // plane G, row 0; planes G, B, R are dst_plane bytes apart
    int64_t dst_pitch, dst_plane;                      // dst_plane = dst_pitch * h
    int w, h;
    float scale[3], bias[3];                           // for R, G, B of the picture
    float maxcode;                                     // 255 / 1023 / 65535
    int bgr;                                           // tensor channel 0, 1, 2 = B, G, R instead of R, G, B
    int srcvec;                                        // tensor and its pitches on TensorVectorBytes: vector loads where the columns allow, element loads otherwise
    int dstvec;                                        // sample and its pitch on 4 x the component size: one store per lane and plane where the columns allow
    // DEVICE table of n_frames {src, dst} rows, frame = blockIdx.z (the TensorFrame convention); null: one frame, src / dst above.  With
    // a table srcvec and dstvec hold only if EVERY frame of the launch allows them
    const SampleFrame *frames;
};
// bytes: 1 (GBRP8) or 2 (GBRP10 / GBRP16) per component.  The caller has checked sizes, alignments and overlaps (SampleSurface,
// hip_video_processor_ext.cpp); one launch for up to 65535 frames (the grid's z extent), one more per further 65535
hipError_t LaunchSampleFromTensor(const SampleParams &p, int dtype, int layout, int bytes, hipStream_t stream, int n_frames = 1);

// ---- host only, no device work (vp_plan.cpp) ----
// component bytes and the largest code of a planar RGB sample format; false: not MPCVR_CF_GBRP8 / GBRP10 / GBRP16
bool SampleFormat(int cformat, int *bytes, int *maxcode);
// the code of one element (mpcvr_plan_sample_code; element_bits: the low 16 for F16 / BF16).  false: another dtype or cformat, element bits
// beyond 16 for a 16-bit dtype, a factor TensorFactorOk refuses
bool PlanSampleCode(int dtype, int cformat, uint32_t element_bits, float scale, float bias, uint32_t *code);
// the context-owned sample surface of mpcvr_process_batch_from_tensors: frame i of a chunk at i * frameStride (3 planes of pitch * h bytes,
// rounded up to 256), chunks by PlanChunks (vp_plan.h) under `budget`
bool PlanBatchSamples(int pitch, int h, int n, size_t budget, ChunkLayout *out);

}  // namespace mpcvr
