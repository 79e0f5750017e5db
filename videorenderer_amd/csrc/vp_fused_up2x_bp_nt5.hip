// the bi-planar twin of the fused exact-2x kernel with 5 taps per axis (Lanczos3 as Direct3D 11 draws it, quirk Q1): see vp_fused_up2x_bp.h / vp_fused_up2x_bp_launch.h
#include "vp_fused_up2x_bp_launch.h"

namespace mpcvr {
template void LaunchFusedUp2xBpNT<5>(const FusedArgs &, dim3, size_t, int, int, int, const FusedFrame *, const unsigned char *, const FrameTable32 &, hipStream_t);
}
