// vp_measure.h — EXTENSION (include/mpcvr.h: mpcvr_measure_pass / mpcvr_measure_backbuffer / mpcvr_process_batch_yuv_stats): the histogram of
// max(R, G, B) over a rectangle of a rendered frame of 32-bit RGB texels, and what a host derives from it (MaxCLL / MaxFALL of CTA-861.3,
// percentiles).  The reference's statistics are an on-screen overlay, so there is no reference line to cite: the definition is
// the integer text of include/mpcvr.h, modelled bit for bit by tests/measure_model.py.
// The kernel's parameters and its launcher, and the two host functions (vp_plan.cpp); nothing here is shared with the frame path's kernels.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

struct mpcvr_light_level;                              // include/mpcvr.h

namespace mpcvr {

constexpr int kHistBins = 1024;                        // MPCVR_HIST_BINS (mpcvr_capi.cpp asserts they agree)
// The tile of one workgroup: kMeasureWaves wavefronts walk a band of kMeasureBandRows rows (wavefront v takes rows v, v + kMeasureWaves, ...
// of the band: kMeasureBandRows / kMeasureWaves rows, all loaded before the first is counted) over `wg_cols` columns, 256 per step.
constexpr int kMeasureBandRows = 64;
constexpr int kMeasureWaves = 8;
constexpr int kMeasureWaveCols = 256;                  // 64 lanes x 4 columns

struct MeasureParams {
    const uint8_t *src; int src_pitch;                 // frame 0: w x h texels of 4 bytes
    size_t frame_stride;                               // bytes from frame z to frame z + 1 (blockIdx.z); unused for one frame
    uint32_t *hist;                                    // frame z counts into hist + kHistBins * z
    int w;                                             // the surface's width (no load reaches past column w - 1)
    int left, top, right, bottom;                      // the rectangle, inside the surface
    int src16;                                         // surface, pitch and frame stride on 16 bytes: a lane with four columns inside the surface takes one 16-byte load per row
    int wg_cols;                                       // columns per workgroup, a multiple of kMeasureWaveCols (0: LaunchMeasure chooses)
};
// The columns one workgroup walks: the widest of 1024 / 512 / 256 that still leaves the launch `kMeasureMinGroups` workgroups, one per
// compute unit (the flush of a workgroup is up to 4 KiB of atomics whatever its tile, so the tile is as large as the
// parallelism lets it be — measured: 4K runs fastest at 512 columns = 272 workgroups, 8K alike at 512 and 1024, both worse at 256).
// MPCVR_MEASURE_WG_COLS=<256 | 512 | 1024 | ...> in the environment overrides it (tools/bench_measure.py sweeps it).
constexpr int kMeasureMaxGroupCols = 1024, kMeasureMinGroups = 256;
int MeasureGroupCols(int rect_w, int rect_h, int n_frames);

// Clears the n_frames x kHistBins words (one hipMemsetAsync on `stream`) and counts behind it: one launch for up to 65535 frames.  An empty
// rectangle leaves the cleared words and launches nothing.  *launches (may be null): kernel launches queued.  The caller checks pointers,
// pitch and that the rectangle lies inside the surface (MeasureSurface, hip_video_processor_ext.cpp).
hipError_t LaunchMeasure(const MeasureParams &p, bool in10, hipStream_t stream, int n_frames = 1, int *launches = nullptr);

// ---- host only, no device work (vp_plan.cpp) ----
// 10000 * EOTF_ST2084(code / maxin) in double, the constants of Shaders/convert/st2084.hlsl
double PqCodeToNits(int code, int maxin);
void LightLevelFromHistogram(const uint32_t *hist, int maxin, ::mpcvr_light_level *out);
// the smallest code whose cumulative count reaches ceil(ppm * pixels / 10^6); -1 for an empty histogram
int HistogramPercentile(const uint32_t *hist, uint32_t ppm);

}  // namespace mpcvr
