// vp_fused_up2x_bp.hip — host side of the bi-planar twin of the fused exact-2x kernel (vp_fused_up2x_bp.h): which launches may take it.
#include "vp_fused_up2x_bp.h"

#include "../../include/mpcvr.h"

namespace mpcvr {

bool FusedUp2xRowCarryHolds(int vk1, int vk2, int vk3, int rect_t, int H, int ch)
{
    if (H < 1 || ch < 1) return false;
    // segments start on even rows (LaunchFusedUp2x), so every iteration's first virtual row is odd: a = -3, -1, .. and the last one of
    // a frame's last segment is at most H + 1.  A segment's first convert loads both rows; every later one relies on the pair (a - 2, a).
    int prev_a, prev_b;
    FusedUp2xChromaRows(vk1, vk2, vk3, rect_t, H, ch, -3, &prev_a, &prev_b);
    for (int a = -1; a <= H + 3; a += 2) {
        int row_a, row_b;
        FusedUp2xChromaRows(vk1, vk2, vk3, rect_t, H, ch, a, &row_a, &row_b);
        if (row_a != prev_b) return false;
        prev_b = row_b;
    }
    return true;
}

bool FusedUp2xBpTakes(const FusedArgs &a, int srck, int epik, int tailk)
{
    // an instantiation that exists (bp_planned), in the fast form of the convert stage
    const bool planned = (srck == SRC_P01X && (epik == EPI_DITHER8 || epik == EPI_DIRECT8) && (tailk == TAILK_PQ_LUT || tailk == TAILK_HLG || tailk == TAILK_NONE)) ||
                         (srck == SRC_NV12 && epik == EPI_DIRECT8 && tailk == TAILK_NONE);
    if (!planned || a.exact_cv) return false;
    // 4:2:0 with the bilinear chroma filter, not centred: the odd luma column is the mean of texels c0 and c0 + 1
    if (a.sub422 || a.sub444 || a.packed422 || a.packed444 || a.gray || a.nearest || a.center_h || a.cw_own != 0.5f || a.cw_next != 0.5f) return false;
    // the matrix' structural zeros (every non-constant-luminance YCbCr matrix; a hue-rotated ProcAmp matrix has none)
    if (a.m[1] != 0.0f || a.m[8] != 0.0f) return false;
    // the odd column's chroma coefficients are used halved (HH, fused_up2x_body): halving must be exact — it is unless m is subnormal-small
    for (int i : {2, 4, 5, 7})
        if (a.m[i] != 0.0f && (0.5f * a.m[i]) * 2.0f != a.m[i]) return false;
    // the lane identity: lane j + 1's texel c0 is lane j's c0 + 1.  Inside the rect that takes even W and rect_l (blocks start on even
    // columns); at the left edge the clamped lanes' odd columns are patched over (stage C's edge branch); at the right edge the lanes
    // clamped to block W - 2 all hold texel c0 = (rect_l + W - 2) / 2, which is their c0 + 1 only where the frame's chroma ends there
    if ((a.W & 1) || (a.rect_l & 1) || a.W < 2) return false;
    if (((a.rect_l + a.W - 2) >> 1) < a.cw - 1) return false;
    // the row identity: rect_t even and a siting whose chroma row advances by one per iteration — enumerated over the launch's rows
    // (H / 2 + 4 scalar steps per launch), the clamped rows above and below the rect included
    if (a.rect_t & 1) return false;
    return FusedUp2xRowCarryHolds(a.vk1, a.vk2, a.vk3, a.rect_t, a.H, a.ch);
}

int &FusedUp2xLastForm()
{
    static thread_local int form = -1;
    return form;
}

}  // namespace mpcvr

extern "C" int32_t mpcvr_plan_up2x_row_carry(int32_t vk1, int32_t vk2, int32_t vk3, int32_t rect_t, int32_t h, int32_t ch)
{
    return mpcvr::FusedUp2xRowCarryHolds(vk1, vk2, vk3, rect_t, h, ch) ? 1 : 0;
}
