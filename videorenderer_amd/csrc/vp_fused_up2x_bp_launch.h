// vp_fused_up2x_bp_launch.h — k_fused_up2x_bp, the bi-planar twin of the fused exact-2x kernel (fused_up2x_body with BP set: see
// vp_fused_up2x_bp.h), and its per-tap-count launcher; vp_fused_up2x_bp_nt{4,5,6}.hip instantiate one tap count each (seven kernels).
// -DMPCVR_UP2X_BP_HEADLINE_ONLY (tests/test_up2x_bp_loop.py): only the headline instantiation <5, PQ table, P01x, integer dither>.
#pragma once
#include "vp_fused_up2x.h"

namespace mpcvr {

namespace {

template <int NT, int TAIL, int SRC, int EPI>
__global__ __launch_bounds__(256, MPCVR_UP2X_WAVES) void k_fused_up2x_bp(FusedArgs P, const FusedFrame *__restrict__ frames, const unsigned char *__restrict__ baked,
                                                                         FrameTable32 tab)
{
    fused_up2x_body<NT, TAIL, SRC, EPI, XC_NEVER, 1>(P, frames, baked, tab);
}

}  // namespace

template <int NT>
void LaunchFusedUp2xBpNT(const FusedArgs &a, dim3 grid, size_t lds, int tailk, int srck, int epik, const FusedFrame *frames_dev, const unsigned char *baked,
                         const FrameTable32 &tab, hipStream_t s)
{
    const dim3 block(256, 1, 1);
#define MPCVR_LAUNCH_BP(TK, SK, EK) hipLaunchKernelGGL((k_fused_up2x_bp<NT, TK, SK, EK>), grid, block, lds, s, a, frames_dev, baked, tab)
#ifdef MPCVR_UP2X_BP_HEADLINE_ONLY
    MPCVR_LAUNCH_BP(TAILK_PQ_LUT, SRC_P01X, EPI_DITHER8);
#else
    // every (tail, source, epilogue) of bp_planned(): FusedUp2xBpTakes lets nothing else through
    if (srck == SRC_NV12) MPCVR_LAUNCH_BP(TAILK_NONE, SRC_NV12, EPI_DIRECT8);
    else if (epik == EPI_DITHER8) {
        if (tailk == TAILK_PQ_LUT) MPCVR_LAUNCH_BP(TAILK_PQ_LUT, SRC_P01X, EPI_DITHER8);
        else if (tailk == TAILK_HLG) MPCVR_LAUNCH_BP(TAILK_HLG, SRC_P01X, EPI_DITHER8);
        else MPCVR_LAUNCH_BP(TAILK_NONE, SRC_P01X, EPI_DITHER8);
    } else {
        if (tailk == TAILK_PQ_LUT) MPCVR_LAUNCH_BP(TAILK_PQ_LUT, SRC_P01X, EPI_DIRECT8);
        else if (tailk == TAILK_HLG) MPCVR_LAUNCH_BP(TAILK_HLG, SRC_P01X, EPI_DIRECT8);
        else MPCVR_LAUNCH_BP(TAILK_NONE, SRC_P01X, EPI_DIRECT8);
    }
#endif
#undef MPCVR_LAUNCH_BP
}

}  // namespace mpcvr
