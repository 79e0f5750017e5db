// vp_deint.h — EXTENSION (include/mpcvr.h: mpcvr_deint_pass / mpcvr_copy_sample_fields / mpcvr_process_batch_deint): motion-adaptive
// deinterlacing of a sample at field rate, plane by plane — the edge-directed spatial prediction held inside a temporal band, in integers.
// The reference leaves deinterlacing to the fixed-function video processor, so there is no reference line to cite: the
// definition is the text of include/mpcvr.h, the arithmetic vp_deint_core.h (DeintComponent), modelled bit for bit by tests/deint_model.py.
// The kernel's parameters and its launcher; nothing here is shared with the frame path's kernels.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "vp_plan.h"
#include "vp_deint_core.h"

namespace mpcvr {

// The tile.  Columns are counted in CHANNEL STEPS: a step is cs components (1, or one U,V pair of a bi-planar chroma plane).  A lane owns
// kDeintLaneSteps consecutive steps of a row, a wavefront kDeintWaveCols; it walks down a strip of kDeintStripRows rows (whole row pairs).
// A workgroup is kDeintWaves wavefronts, one strip below the other.
constexpr int kDeintLaneSteps = 4;
constexpr int kDeintWaveCols = 64 * kDeintLaneSteps;
constexpr int kDeintStripRows = 4;
constexpr int kDeintWaves = 4;
constexpr int kDeintGroupCols = kDeintWaveCols;
constexpr int kDeintGroupRows = kDeintWaves * kDeintStripRows;
constexpr int kDeintMaxPlanes = 3;

// one plane as the host describes it (mpcvr_deint_plane, include/mpcvr.h)
struct DeintPlane { size_t offset; int32_t pitch, comps, lines, bytes, cs, mask; };
// the planes of a sample of (cformat, w, h, pitch) by mpcvr_set_input's rules (pitch 0: the default pitch); false: a format the pass does
// not take, a size or pitch outside the rules, a plane of fewer than 2 lines.  Host only (vp_plan.cpp)
bool PlanDeintPlanes(int cformat, int w, int h, int pitch, int *planes, DeintPlane out[kDeintMaxPlanes]);
// the context-owned sample surface of mpcvr_process_batch_deint: output frame i of a chunk at i * frameStride (pitch * lines bytes rounded
// up to 256), chunks by PlanChunks (vp_plan.h) under `budget`
bool PlanBatchDeint(int pitch, int lines, int nOut, size_t budget, ChunkLayout *out);

// one output frame of a launch with a frame dimension: three samples, the sample to write, the shown field
struct DeintFrame { const uint8_t *prev, *cur, *next; uint8_t *dst; int32_t keep, first; };

// one plane of a launch: where it lies in a sample (the same in prev, cur and next) and in the destination
struct DeintLaunchPlane { int64_t src_off, dst_off, src_pitch, dst_pitch; int32_t steps, lines; };

struct DeintParams {
    DeintFrame one;                                    // the frame, by value, of a launch without a table
    const DeintFrame *frames;                          // DEVICE table of n_frames rows (frame = blockIdx.z / n_planes); null: `one`
    DeintLaunchPlane plane[kDeintMaxPlanes];           // the planes of one (bytes, cs): plane = blockIdx.z % n_planes
    int32_t n_planes;
    int32_t mask;                                      // applied to every component on load: 0xff, 0x3ff (planar 10-bit) or 0xffff
    int32_t srcvec;                                    // every source plane of the launch and its pitch on 4 * cs * bytes: one vector load per lane and row
    int32_t dstvec;                                    // ... every destination plane: one vector store per lane and row
};
// bytes 1 / 2, cs 1 / 2, mode DI_ADAPTIVE / DI_ADAPTIVE_NOCHECK.  The caller has checked sizes, pitches and overlaps (DeintSurface,
// hip_video_processor_ext.cpp); one launch for as many frames as the grid's z extent holds, one more per further such lot
hipError_t LaunchDeint(const DeintParams &p, int bytes, int cs, int mode, hipStream_t stream, int n_frames = 1);

}  // namespace mpcvr
