// vp_deband.h — EXTENSION (include/mpcvr.h: mpcvr_deband_pass / mpcvr_render_deband / mpcvr_process_batch_deband): hashed four-tap
// debanding of a surface of 32-bit RGB texels, in integers.  The reference has no deband, so there is no reference line to cite: the
// definition is the text of include/mpcvr.h, the arithmetic vp_deband_core.h, modelled bit for bit by tests/deband_model.py.
// The kernel's parameters and its launcher; nothing here is shared with the frame path's kernels.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "vp_deband_core.h"

namespace mpcvr {

// The tile of one workgroup: kDebandWaves wavefronts, each kDebandWaveRows consecutive rows of kDebandTileCols columns (16 lanes x 4
// columns per row, 4 rows per step).
constexpr int kDebandTileCols = 64;
constexpr int kDebandWaves = 8;
constexpr int kDebandWaveRows = 8;
constexpr int kDebandTileRows = kDebandWaves * kDebandWaveRows;

// Where a launch reads the taps from.  DB_LDS: a workgroup stages its tile plus a halo of R = range * iterations texels on every side,
// clamped to the surface, into LDS ((64 + 2 R)^2 dwords) and a tap is one LDS dword read — possible while two workgroups fit the
// 160 KiB of a CU (R <= kDebandLdsFitR).  DB_GLOBAL: every tap is a 4-byte global load at clamped coordinates (the neighbourhood stays in
// the L2).
enum DebandPlace { DB_GLOBAL = 0, DB_LDS = 1 };
constexpr int kDebandLdsFitR = 32;                     // (64 + 64)^2 * 4 = 65,536: the most dynamic LDS a launch gets without a grant; two workgroups per CU
constexpr size_t DebandLdsBytes(int R) { return (size_t)(kDebandTileCols + 2 * R) * (size_t)(kDebandTileRows + 2 * R) * 4; }
static_assert(DebandLdsBytes(kDebandLdsFitR) <= 64 * 1024 && 2 * DebandLdsBytes(kDebandLdsFitR) <= 160 * 1024, "at least two workgroups in a CU's LDS at the largest halo LDS takes");
// The dispatcher's rule: LDS wherever it fits, global above.  Measured (profiles/r19/deband_pass.txt section 2): at
// R = 8, 16 and 32, at 1080p, 4K and 8K, the geometric mean of global / LDS time is 1.29 .. 1.49; LDS is level at worst (0.99 .. 1.02 with
// one iteration at R = 8 at 4K and 8K) and up to 2.03 x ahead with four iterations, where 64 gathers per lane meet one staging
constexpr int kDebandLdsMaxR = 32;
constexpr int DebandPlacement(int R, int /*w*/, int /*h*/) { return R <= kDebandLdsMaxR ? DB_LDS : DB_GLOBAL; }
// ... and what a launch takes: the rule, or what MPCVR_DEBAND_TAPS names in its place (vp_deband.hip)
int DebandPlaceFor(int R, int w, int h);
inline const char *DebandPlaceName(int place) { return place == DB_LDS ? "lds" : "global"; }

// range 1 .. 64, iterations 1 .. 4, range * iterations <= 64, threshold 0 .. 4 maxin (quarter codes of the source), dither 0 / 1
constexpr bool DebandArgsValid(const DebandArgs &a, bool in10)
{
    return a.range >= 1 && a.range <= kDebandMaxRange && a.iterations >= 1 && a.iterations <= kDebandMaxIterations &&
           a.range * a.iterations <= kDebandMaxHalo && a.threshold >= 0 && a.threshold <= 4 * (in10 ? 1023 : 255) && (a.dither == 0 || a.dither == 1);
}

// one frame of a launch with a frame dimension: its source, its destination and its seed (pitches, size, formats and parameters are the launch's)
struct DebandFrame { const uint8_t *src; uint8_t *dst; uint32_t seed, pad; };

struct DebandParams {
    const uint8_t *src; int64_t src_pitch;             // w x h texels of 4 bytes
    uint8_t *dst; int64_t dst_pitch;                   // never over src: lanes read texels other lanes write
    int w, h;
    DebandArgs a; uint32_t seed;
    int src16, dst16;                                  // surface and its pitch on 16 bytes: a lane with four columns inside the surface takes one 16-byte load / store
    // DEVICE table of n_frames {src, dst, seed} rows (the EncodeFrame convention, vp_encode.h); null: one frame, src / dst / seed above.
    // With a table src16 and dst16 hold only if EVERY frame of the launch allows them
    const DebandFrame *frames;
};
// pointers and pitches multiples of 4, valid parameters, no overlap (the caller checks: DebandSurface, hip_video_processor_ext.cpp).
// One launch for a chunk of a batch; further launches only beyond 65535 frames (the grid's z extent)
hipError_t LaunchDeband(const DebandParams &p, bool in10, bool out10, hipStream_t stream, int n_frames = 1);

// ---- host only, no device work (vp_plan.cpp) ----
// the defaults for a source format (mpcvr_deband_params_default).  false: another format
bool PlanDebandDefaults(int src_fmt, DebandArgs *a);
// the whole pass over surfaces in host memory (mpcvr_deband_host).  false: whatever mpcvr_deband_pass refuses with MPCVR_E_INVALIDARG
bool PlanDebandHost(const void *src, int64_t src_pitch, int src_fmt, int w, int h, const DebandArgs &a, uint32_t seed, void *dst, int64_t dst_pitch, int dst_fmt);

}  // namespace mpcvr
