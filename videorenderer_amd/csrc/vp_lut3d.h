// vp_lut3d.h — EXTENSION (include/mpcvr.h: mpcvr_lut3d_pass / mpcvr_render_lut3d / mpcvr_process_batch_lut3d): a 3D colour LUT applied to
// a surface of 32-bit RGB texels, tetrahedral interpolation in 32-bit integers.  The reference has no LUT, so there is no reference line
// to cite: the definition is the text of include/mpcvr.h, the arithmetic vp_lut3d_core.h, modelled bit for bit by tests/lut3d_model.py.
// The kernel's parameters and its launcher; nothing here is shared with the frame path's kernels.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "vp_lut3d_core.h"

namespace mpcvr {

// The tile of one workgroup: kLut3dWaves wavefronts, each kLut3dWaveRows consecutive rows of kLut3dWaveCols columns (64 lanes x 4).
constexpr int kLut3dWaveCols = 256;
constexpr int kLut3dWaves = 8;
constexpr int kLut3dWaveRows = 1;
constexpr int kLut3dGroupCols = kLut3dWaveCols;
constexpr int kLut3dGroupRows = kLut3dWaves * kLut3dWaveRows;
// ... and of the workgroups that read a table from LDS of which fewer than four fit a CU (tables above 40 KB: n >= 18)
constexpr int kLut3dLdsWideWaves = 16;

// Where a launch reads the table from.  L3_LDS: persistent workgroups copy the whole table into LDS once and read vertices from there —
// possible while n^3 * 8 bytes fit the 160 KiB of a CU (n <= kLut3dLdsFitN).  L3_GLOBAL: every vertex is an 8-byte global load (the
// table stays in the L2: 2.2 MB at n = 65).
enum Lut3dPlace { L3_GLOBAL = 0, L3_LDS = 1 };
constexpr int kLut3dLdsFitN = 27;                      // 27^3 * 8 = 157,464 <= 163,840 < 28^3 * 8
constexpr size_t Lut3dTableBytes(int n) { return (size_t)n * (size_t)n * (size_t)n * sizeof(Lut3dEntry); }
// The dispatcher's rule: LDS wherever the table fits.  Measured (profiles/r18/lut3d_pass.txt): from LDS the pass takes
// the same time for every picture — within 2-14 % of the global placement on a rendered 4K / 8K frame (23 % behind at 1080p with n = 27, where
// staging the table outweighs the frame) and 1.1-3.1 x ahead of it on noise, where a wavefront's 64 reads fall on 64 different cache lines
constexpr int kLut3dLdsMaxN = 27;
constexpr int Lut3dPlacement(int n) { return n <= kLut3dLdsMaxN ? L3_LDS : L3_GLOBAL; }
// ... and what a launch takes: the rule, or what MPCVR_LUT3D_TABLE names in its place (vp_lut3d.hip)
int Lut3dPlaceFor(int n);
inline const char *Lut3dPlaceName(int place) { return place == L3_LDS ? "lds" : "global"; }

// one frame of a launch with a frame dimension: its source and its destination (pitches, size, formats and the table are the launch's)
struct Lut3dFrame { const uint8_t *src; uint8_t *dst; };

struct Lut3dParams {
    const uint8_t *src; int64_t src_pitch;             // w x h texels of 4 bytes
    uint8_t *dst; int64_t dst_pitch;                   // may be src with the same pitch: a lane reads its texels before it writes them
    int w, h;
    const Lut3dEntry *lut; int n;                      // DEVICE, n^3 entries, R fastest
    int src16, dst16;                                  // surface and its pitch on 16 bytes: a lane with four columns inside the surface takes one 16-byte load / store
    // DEVICE table of n_frames {src, dst} rows (the EncodeFrame convention, vp_encode.h); null: one frame, src / dst above.  With a table
    // src16 and dst16 hold only if EVERY frame of the launch allows them
    const Lut3dFrame *frames;
};
// pointers and pitches multiples of 4, the table on 8 bytes, no overlap but dst == src (the caller checks: Lut3dSurface,
// hip_video_processor_ext.cpp).  One launch for a chunk of a batch; further launches only beyond 65535 frames (the grid's z extent) or
// 2^31 tiles
hipError_t LaunchLut3d(const Lut3dParams &p, bool in10, bool out10, hipStream_t stream, int n_frames = 1);

// ---- host only, no device work (vp_plan.cpp) ----
// n^3 float triplets in .cube order -> the 8-byte entries (mpcvr_plan_lut3d_entries)
void PlanLut3dEntries(const float *rgb, int n, uint16_t *entries);
// one texel on the host (mpcvr_plan_lut3d_value).  false: another format or n
bool PlanLut3dValue(int src_fmt, int dst_fmt, const uint16_t *entries, int n, uint32_t texel, uint32_t *out);

}  // namespace mpcvr
