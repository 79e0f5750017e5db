// vp_sharpen.h — EXTENSION (include/mpcvr.h: mpcvr_sharpen_pass / mpcvr_render_sharpen / mpcvr_process_batch_sharpen): binomial unsharp
// mask of a surface of 32-bit RGB texels, in integers.  The reference has no sharpener, so there is no reference line to cite: the
// definition is the text of include/mpcvr.h, the arithmetic vp_sharpen_core.h, modelled bit for bit by tests/sharpen_model.py.
// The kernel's parameters and its launcher; nothing here is shared with the frame path's kernels.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "vp_sharpen_core.h"

namespace mpcvr {

// The tile of one workgroup: kSharpenWaves wavefronts, each kSharpenWaveRows consecutive rows of kSharpenTileCols columns (16 lanes x 4
// columns per row, 4 rows per step) — k_deband's launch shape.
constexpr int kSharpenTileCols = 64;
constexpr int kSharpenWaves = 8;
constexpr int kSharpenWaveRows = 8;
constexpr int kSharpenTileRows = kSharpenWaves * kSharpenWaveRows;
// The staged image in LDS: the tile's rows plus r above and below, and kSharpenImageCols columns: the tile's 64 with 4 to the left and 4 to
// the right (of which r are used), so that the tile's first column sits on 16 bytes and a lane reads its four columns and the four on
// either side as three 16-byte LDS reads.
constexpr int kSharpenPad = 4;
constexpr int kSharpenImageCols = kSharpenTileCols + 2 * kSharpenPad;
// LDS of one workgroup: the image, and the horizontal sums of every image row over the tile's columns — two dwords per texel in mode 0
// (R and B ride in one: a sum of a 10-bit code is <= 64 * 1023 = 65,472), one in mode 1 (the luma's)
constexpr int SharpenLdsBytes(int r, int mode)
{
    return (kSharpenTileRows + 2 * r) * (kSharpenImageCols + kSharpenTileCols * (mode == SHARPEN_LUMA ? 1 : 2)) * 4;
}
static_assert(SharpenLdsBytes(kSharpenMaxRadius, SHARPEN_RGB) <= 64 * 1024 && 2 * SharpenLdsBytes(kSharpenMaxRadius, SHARPEN_RGB) <= 160 * 1024, "two workgroups in a CU's LDS at the largest radius");

// radius 1 .. 3, amount 0 .. 256, threshold 0 .. 4 maxin (quarter codes of the source), overshoot 0 .. maxin, mode 0 / 1, dither 0 / 1
constexpr bool SharpenArgsValid(const SharpenArgs &a, bool in10)
{
    return a.radius >= 1 && a.radius <= kSharpenMaxRadius && a.amount >= 0 && a.amount <= kSharpenMaxAmount && a.threshold >= 0 &&
           a.threshold <= 4 * (in10 ? 1023 : 255) && a.overshoot >= 0 && a.overshoot <= (in10 ? 1023 : 255) &&
           (a.mode == SHARPEN_RGB || a.mode == SHARPEN_LUMA) && (a.dither == 0 || a.dither == 1);
}

// one frame of a launch with a frame dimension: its source, its destination and its seed (pitches, size, formats and parameters are the launch's)
struct SharpenFrame { const uint8_t *src; uint8_t *dst; uint32_t seed, pad; };

struct SharpenParams {
    const uint8_t *src; int64_t src_pitch;             // w x h texels of 4 bytes
    uint8_t *dst; int64_t dst_pitch;                   // never over src: workgroups read texels other workgroups write
    int w, h;
    SharpenArgs a; uint32_t seed;
    int src16, dst16;                                  // surface and its pitch on 16 bytes: four columns inside the surface are one 16-byte load / store
    // DEVICE table of n_frames {src, dst, seed} rows (the EncodeFrame convention, vp_encode.h); null: one frame, src / dst / seed above.
    // With a table src16 and dst16 hold only if EVERY frame of the launch allows them
    const SharpenFrame *frames;
};
// pointers and pitches multiples of 4, valid parameters, no overlap (the caller checks: SharpenSurface, hip_video_processor_ext.cpp).
// One launch for a chunk of a batch; further launches only beyond 65535 frames (the grid's z extent)
hipError_t LaunchSharpen(const SharpenParams &p, bool in10, bool out10, hipStream_t stream, int n_frames = 1);

// ---- host only, no device work (vp_plan.cpp) ----
// the defaults for a source format (mpcvr_sharpen_params_default).  false: another format
bool PlanSharpenDefaults(int src_fmt, SharpenArgs *a);
// the whole pass over surfaces in host memory (mpcvr_sharpen_host).  false: whatever mpcvr_sharpen_pass refuses with MPCVR_E_INVALIDARG
bool PlanSharpenHost(const void *src, int64_t src_pitch, int src_fmt, int w, int h, const SharpenArgs &a, uint32_t seed, void *dst, int64_t dst_pitch, int dst_fmt);

}  // namespace mpcvr
