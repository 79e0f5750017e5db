// vp_fused_prefetch.h — load_raw's row-pair prefetch (vp_fused_dev.h), issued so that the compiler's wait-count pass does not see it,
// and the hand-counted wait that goes with it.  Used by the fused exact-2x kernel (vp_fused_up2x.h) alone and kept out of
// vp_fused_dev.h, which every fused kernel includes: the traffic records of profiles/hbm_traffic.json are tied to the digest of the
// sources a workload's kernels are built from, and the other kernels' binaries do not change with this file.
#pragma once
#include "vp_fused_dev.h"

namespace mpcvr {

namespace {

// On the gfx9 family vector loads AND stores share one counter (vmcnt) that retires in issue order — the compiler's own model of
// this target.  Where paths with different numbers of memory operations meet (the loads behind `t + 1 < n_iter`, the row stores
// behind `t >= 3 && store_ok`), its s_waitcnt pass assumes the fewest, so in front of every convert stage it wrote vmcnt(3..0):
// wait until every output row this wave has stored so far is acknowledged, and until the prefetch of the previous iteration has
// landed.  For the fixed-count sources the row pair is therefore loaded by ONE inline-assembly statement (saddr form: wave-uniform
// row base in an SGPR pair + the lane's 32-bit offset) and waited for by hand, with the number of vector memory operations the wave
// has certainly issued since (raw_unseen_arrived).  The compiler takes an assembly output for valid at once, so
//   * the raw load results stay untouched in RawUnseen until the wait; what load_raw does to them (the NV12 unpack, U | V << 16 of
//     the planar formats) happens in raw_unseen_finish, behind it;
//   * the outputs are early-clobber: a destination that shared a register with a lane offset could land before a later load of the
//     statement has read the offset;
//   * the statement opens with s_nop 4: a row base restored from a spill lane (v_readlane_b32) just in front of it is a VALU write
//     of an SGPR a vector memory instruction reads, five wait states the compiler pads only for instructions of its own.
// SRC_GENERIC (plane count and sample size known at run time only) keeps load_raw and the compiler's waits.
template <int SRC>
__host__ __device__ constexpr int raw_unseen_loads() { return (SRC == SRC_P01X || SRC == SRC_NV12) ? 6 : (SRC == SRC_PLANAR16 || SRC == SRC_PLANAR8) ? 10 : 0; }
template <int N> struct RawUnseen { uint32_t v[N]; };     // luma rows 0, 1; then chroma as [plane][column c0, c0+1][row n, n+1]

#define MPCVR_LD_(op, d, o, b) "\n\t" op " %[" d "], %[" o "], %[" b "]"
// bi-planar: 2 luma + 4 interleaved-chroma loads
#define MPCVR_UNSEEN6(YOP, COP) \
    asm volatile("s_nop 4" MPCVR_LD_(YOP, "d0", "yo", "r0") MPCVR_LD_(YOP, "d1", "yo", "r1") \
                 MPCVR_LD_(COP, "d2", "c1", "ua") MPCVR_LD_(COP, "d3", "c1", "ub") MPCVR_LD_(COP, "d4", "c2", "ua") MPCVR_LD_(COP, "d5", "c2", "ub") \
                 : [d0] "=&v"(r.v[0]), [d1] "=&v"(r.v[1]), [d2] "=&v"(r.v[2]), [d3] "=&v"(r.v[3]), [d4] "=&v"(r.v[4]), [d5] "=&v"(r.v[5]) \
                 : [yo] "v"(ra.yoff), [c1] "v"(ra.coff[1]), [c2] "v"(ra.coff[2]), [r0] "s"(ry0), [r1] "s"(ry1), [ua] "s"(pu + oA), [ub] "s"(pu + oB))
// three planes: 2 luma + 4 U + 4 V loads
#define MPCVR_UNSEEN10(YOP, COP) \
    asm volatile("s_nop 4" MPCVR_LD_(YOP, "d0", "yo", "r0") MPCVR_LD_(YOP, "d1", "yo", "r1") \
                 MPCVR_LD_(COP, "d2", "c1", "ua") MPCVR_LD_(COP, "d3", "c1", "ub") MPCVR_LD_(COP, "d4", "c2", "ua") MPCVR_LD_(COP, "d5", "c2", "ub") \
                 MPCVR_LD_(COP, "d6", "c1", "va") MPCVR_LD_(COP, "d7", "c1", "vb") MPCVR_LD_(COP, "d8", "c2", "va") MPCVR_LD_(COP, "d9", "c2", "vb") \
                 : [d0] "=&v"(r.v[0]), [d1] "=&v"(r.v[1]), [d2] "=&v"(r.v[2]), [d3] "=&v"(r.v[3]), [d4] "=&v"(r.v[4]), [d5] "=&v"(r.v[5]), \
                   [d6] "=&v"(r.v[6]), [d7] "=&v"(r.v[7]), [d8] "=&v"(r.v[8]), [d9] "=&v"(r.v[9]) \
                 : [yo] "v"(ra.yoff), [c1] "v"(ra.coff[1]), [c2] "v"(ra.coff[2]), [r0] "s"(ry0), [r1] "s"(ry1), \
                   [ua] "s"(pu + oA), [ub] "s"(pu + oB), [va] "s"(pv + oA), [vb] "s"(pv + oB))
template <int SRC>
__device__ __forceinline__ void load_raw_unseen(const FusedArgs &P, gcptr py, const RawAddr &ra, int y0, int y1, RawUnseen<raw_unseen_loads<SRC>()> &r)
{
    const int sy0 = P.rect_t + y0, sy1 = P.rect_t + y1;
    const gcptr ry0 = py + (uint32_t)sy0 * (uint32_t)P.pitch_y, ry1 = py + (uint32_t)sy1 * (uint32_t)P.pitch_y;
    const int n = chroma_v4(P, sy0) >> 2;
    const uint32_t oA = (uint32_t)clampi(n, 0, P.ch - 1) * (uint32_t)P.pitch_c, oB = (uint32_t)clampi(n + 1, 0, P.ch - 1) * (uint32_t)P.pitch_c;
    const gcptr pu = py + P.off_u;
    if constexpr (SRC == SRC_P01X) MPCVR_UNSEEN6("global_load_dword", "global_load_dword");
    else if constexpr (SRC == SRC_NV12) MPCVR_UNSEEN6("global_load_ushort", "global_load_ushort");
    else {
        const gcptr pv = py + P.off_v;
        if constexpr (SRC == SRC_PLANAR16) MPCVR_UNSEEN10("global_load_dword", "global_load_ushort");
        else MPCVR_UNSEEN10("global_load_ushort", "global_load_ubyte");
    }
}
#undef MPCVR_UNSEEN10
#undef MPCVR_UNSEEN6
#undef MPCVR_LD_
// Wait for a group of L loads.  `t` = the loop iteration the wait stands in (wave-uniform).  The group was issued in iteration
// t - 2, behind that iteration's convert; since then the wave has certainly issued the 4 row stores of iteration t - 2 (if
// t - 2 >= 3: lane 0 of every wave that got this far stores), the L loads of iteration t - 1 and the 4 row stores of iteration
// t - 1 (if t - 1 >= 3): vmcnt(L + 8) from t = 5 on, L + 4 at t = 4, L during the run-in (and for the first convert, in front
// of the loop, which has only the second prologue group behind it).  The unaligned generic epilogue issues 16 stores per
// iteration instead of 4: counted as 4, a count that is too low only waits longer.  One too high reads registers before the
// data is there — wrong pixels, not a fault.  s_waitcnt takes an immediate only, hence the ladder of scalar branches; the
// statement names no register (tying the destinations to it made the compiler copy them in front of the wait), so a
// scheduling barrier keeps their readers behind it.
template <int L>
__device__ __forceinline__ void raw_unseen_arrived(int t)
{
    asm volatile("s_cmp_lt_i32 %0, 5\n\t"
                 "s_cbranch_scc1 1f\n\t"
                 "s_waitcnt vmcnt(%1)\n\t"
                 "s_branch 3f\n"
                 "1:\n\t"
                 "s_cmp_lt_i32 %0, 4\n\t"
                 "s_cbranch_scc1 2f\n\t"
                 "s_waitcnt vmcnt(%2)\n\t"
                 "s_branch 3f\n"
                 "2:\n\t"
                 "s_waitcnt vmcnt(%3)\n"
                 "3:" : : "s"(t), "n"(L + 8), "n"(L + 4), "n"(L) : "memory", "scc");
    __builtin_amdgcn_sched_barrier(0);
}
// what load_raw does with the loaded codes, behind the wait (raw_codes: the three-plane 16-bit loader alone cuts its dwords to P.raw_mask)
template <int SRC>
__device__ __forceinline__ void raw_unseen_finish(const FusedArgs &P, const RawUnseen<raw_unseen_loads<SRC>()> &u, Raw &r)
{
    r.y[0] = raw_codes<SRC>(P, u.v[0]); r.y[1] = raw_codes<SRC>(P, u.v[1]);
    r.c[0][0] = r.c[1][0] = 0;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int rr = 0; rr < 2; rr++) {
            const uint32_t d = u.v[2 + 2 * i + rr];
            if constexpr (SRC == SRC_P01X) r.c[rr][1 + i] = d;
            else if constexpr (SRC == SRC_NV12) r.c[rr][1 + i] = (d & 0xffu) | ((d >> 8) << 16);
            else r.c[rr][1 + i] = raw_codes<SRC>(P, d | (u.v[6 + 2 * i + rr] << 16));
        }
}

}  // namespace

}  // namespace mpcvr
