// vp_fused_up2x_bp.h — the bi-planar twin of the fused exact-2x kernel's convert stage (k_fused_up2x_bp, vp_fused_up2x_bp_launch.h).
//
// The generic stage C (convert_block + load_raw_unseen) repeats three things in every iteration of every wave of a 4:2:0 bi-planar launch:
//   * lane j loads and converts the chroma texels of columns c0 and c0 + 1, lane j + 1 loads column c0 + 1 again as its own c0 and
//     repeats its vertical interpolation;
//   * an iteration reads chroma rows n and n + 1, the next one n + 1 and n + 2: row n + 1 is loaded and converted twice;
//   * every non-constant-luminance YCbCr matrix has m[1] == 0 and m[8] == 0, and all nine matrix FMAs are issued.
// The twin loads ONE chroma dword per iteration (column c0, row n + 1), keeps its two converted floats for the next iteration (where
// they are row n), takes the vertically interpolated pairs of column c0 + 1 from lane j + 1 with a wave-wide shift by one lane (DPP:
// no LDS round trip) and drops the two matrix FMAs whose coefficient is a structural zero.  Everything else of the loop — stage X,
// stage Y, the epilogues, the software pipeline, the counted wait — is fused_up2x_body's own text (vp_fused_up2x.h), which reads this header's pieces where its BP argument is set.
// Same values, same operations on them, in the same order as the generic stage — but for two rescalings that are exact and sit inside
// a neighbouring FMA here (the odd column's halved chroma: HH below; the convert output's read-back: nbc2, vp_fused_up2x.h; both
// identities are checked in tests/test_up2x_bp_folds.py): the two kernels agree bit for bit
// (tests/test_up2x_bp_gpu.py, tests/test_up2x_bp_folds_gpu.py), and LaunchFusedUp2xNT takes the twin only where FusedUp2xBpTakes says the identities above hold for
// the whole launch — anything else runs the generic kernel, so a disagreement costs the fast path, never a pixel.
// New device code lives here and not in vp_fused_dev.h, which every fused kernel's traffic record is tied to (profiles/hbm_traffic.json).
#pragma once
#include "vp_fused_dev.h"
#include "vp_fused_prefetch.h"

namespace mpcvr {

// ---- host side (vp_fused_up2x_bp.hip) ----
// Chroma rows (n, n + 1), clamped, of the iteration that converts virtual rows a, a + 1 — load_raw_unseen's own expressions.
inline void FusedUp2xChromaRows(int vk1, int vk2, int vk3, int rect_t, int H, int ch, int a, int *rowA, int *rowB)
{
    const int y0 = a < 0 ? 0 : a > H - 1 ? H - 1 : a;
    const int sy0 = rect_t + y0;
    const int n = (vk1 * sy0 + vk2 * (sy0 & ~1) + vk3) >> 2;          // chroma_v4(P, sy0) >> 2
    *rowA = n < 0 ? 0 : n > ch - 1 ? ch - 1 : n;
    *rowB = n + 1 < 0 ? 0 : n + 1 > ch - 1 ? ch - 1 : n + 1;
}
// The row identity the twin's carried row stands on: chroma row n of every iteration is row n + 1 of the iteration before it, for every
// iteration of every segment (virtual rows a = -3, -1, .. H + 1: the run-in above the rect and the clamped rows below it included).
bool FusedUp2xRowCarryHolds(int vk1, int vk2, int vk3, int rect_t, int H, int ch);
// May this launch take the twin?  (srck / epik / tailk: the launcher's source, epilogue and tail kinds)
bool FusedUp2xBpTakes(const FusedArgs &a, int srck, int epik, int tailk);
// (FusedUp2xLastForm, vp_launch.h: which of the two the calling thread's last launch took)
// vp_fused_up2x_bp_launch.h, instantiated by vp_fused_up2x_bp_nt{4,5,6}.hip: the twin for one tap count, with the grid, LDS size, table
// image and frame table LaunchFusedUp2xNT has worked out (its own launch, another kernel); the launch must pass FusedUp2xBpTakes
template <int NT>
void LaunchFusedUp2xBpNT(const FusedArgs &a, dim3 grid, size_t lds, int tailk, int srck, int epik, const FusedFrame *frames_dev, const unsigned char *baked,
                         const FrameTable32 &tab, hipStream_t s);

namespace {

// plans the twin is instantiated for: P01x with both specialised epilogues behind the table tails and without a tail, NV12 with the straight store
template <int TAIL, int SRC, int EPI>
__host__ __device__ constexpr bool bp_planned()
{
    return (SRC == SRC_P01X && (EPI == EPI_DITHER8 || EPI == EPI_DIRECT8) && (TAIL == TAILK_PQ_LUT || TAIL == TAILK_HLG || TAIL == TAILK_NONE)) ||
           (SRC == SRC_NV12 && EPI == EPI_DIRECT8 && TAIL == TAILK_NONE);
}

// the twin's loads of a row pair: v[0], v[1] luma rows; v[2] chroma column c0 of row n + 1; v[3] the same column of row n — loaded
// by a segment's first group only (BOTH), every later iteration has it from the iteration before
constexpr int BP_LOADS = 3;
struct RawUnseenBp { uint32_t v[4]; };
struct ChromaCarry { float u, v; };        // the converted (U, V) of column c0, chroma row n + 1 of the last convert stage

#define MPCVR_LD_(op, d, o, b) "\n\t" op " %[" d "], %[" o "], %[" b "]"
#define MPCVR_UNSEEN3(YOP, COP) \
    asm volatile("s_nop 4" MPCVR_LD_(YOP, "d0", "yo", "r0") MPCVR_LD_(YOP, "d1", "yo", "r1") MPCVR_LD_(COP, "d2", "c1", "ub") \
                 : [d0] "=&v"(r.v[0]), [d1] "=&v"(r.v[1]), [d2] "=&v"(r.v[2]) \
                 : [yo] "v"(ra.yoff), [c1] "v"(ra.coff[1]), [r0] "s"(ry0), [r1] "s"(ry1), [ub] "s"(pu + oB))
#define MPCVR_UNSEEN4(YOP, COP) \
    asm volatile("s_nop 4" MPCVR_LD_(YOP, "d0", "yo", "r0") MPCVR_LD_(YOP, "d1", "yo", "r1") MPCVR_LD_(COP, "d2", "c1", "ub") MPCVR_LD_(COP, "d3", "c1", "ua") \
                 : [d0] "=&v"(r.v[0]), [d1] "=&v"(r.v[1]), [d2] "=&v"(r.v[2]), [d3] "=&v"(r.v[3]) \
                 : [yo] "v"(ra.yoff), [c1] "v"(ra.coff[1]), [r0] "s"(ry0), [r1] "s"(ry1), [ua] "s"(pu + oA), [ub] "s"(pu + oB))
// load_raw_unseen (vp_fused_prefetch.h: one statement, early-clobber outputs, s_nop 4 — for the reasons given there) with the
// twin's loads: BP_LOADS of them, or one more in front of the loop
template <int SRC, bool BOTH>
__device__ __forceinline__ void load_raw_unseen_bp(const FusedArgs &P, gcptr py, const RawAddr &ra, int y0, int y1, RawUnseenBp &r)
{
    static_assert(SRC == SRC_P01X || SRC == SRC_NV12, "bi-planar sources");
    const int sy0 = P.rect_t + y0, sy1 = P.rect_t + y1;
    const gcptr ry0 = py + (uint32_t)sy0 * (uint32_t)P.pitch_y, ry1 = py + (uint32_t)sy1 * (uint32_t)P.pitch_y;
    const int n = chroma_v4(P, sy0) >> 2;
    const uint32_t oA = (uint32_t)clampi(n, 0, P.ch - 1) * (uint32_t)P.pitch_c, oB = (uint32_t)clampi(n + 1, 0, P.ch - 1) * (uint32_t)P.pitch_c;
    const gcptr pu = py + P.off_u;
    if constexpr (BOTH) {
        if constexpr (SRC == SRC_P01X) MPCVR_UNSEEN4("global_load_dword", "global_load_dword");
        else MPCVR_UNSEEN4("global_load_ushort", "global_load_ushort");
    } else {
        (void)oA;
        if constexpr (SRC == SRC_P01X) MPCVR_UNSEEN3("global_load_dword", "global_load_dword");
        else MPCVR_UNSEEN3("global_load_ushort", "global_load_ushort");
    }
}
#undef MPCVR_UNSEEN4
#undef MPCVR_UNSEEN3
#undef MPCVR_LD_

// (U, V) of an interleaved chroma texel as floats: two 16-bit words (P01x) or two bytes (NV12)
template <int SRC>
__device__ __forceinline__ ChromaCarry chroma_floats(uint32_t d)
{
    if constexpr (SRC == SRC_P01X) return ChromaCarry{(float)(d & 0xffffu), (float)(d >> 16)};
    else return ChromaCarry{(float)(d & 0xffu), (float)((d >> 8) & 0xffu)};
}
// lane j's copy of lane j + 1's value: a wave-wide shift by one lane (DPP wave_shl:1), no LDS.  Lane 63 has no neighbour and reads
// 0.0 (bound_ctrl); its block is rect columns x0 + 122, x0 + 123, and of those stage X reads the even one alone (A column 126 is the
// last its taps reach, from lane 59), which takes its chroma from the lane's own texel — inside the rect no active lane reaches what
// lane 63 gets here.  At the rect's right edge a lane clamped to the last block hands its ODD column to stage X: stage C's edge patch
// (vp_fused_up2x.h) therefore takes that column from the lane in front of it, never from lane 63.
__device__ __forceinline__ float from_next_lane(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130 /* wave_shl:1 */, 0xf, 0xf, true));
}
__device__ __forceinline__ f2 from_next_lane(f2 v) { return f2{from_next_lane(v.x), from_next_lane(v.y)}; }

// convert_block_yuv (vp_fused_dev.h) for the plans of bp_planned(): no Dolby Vision, the table tails or none — its text with
// the matrix FMAs of m[1] (R from U) and m[8] (B from V) left out: 0 * x added to a sum (FusedUp2xBpTakes checks both are 0).
template <int TAIL>
__device__ __forceinline__ void convert_block_yuv_bp(const FusedArgs &P, const f2 (&MM)[5], const f2 (&HH)[2], const f2 (&GG)[5], const f2 (&CC)[3], const f2 (&Ycol)[2], const f2 (&Ucol)[2],
                                                     const f2 (&Vcol)[2], const f2 *T, f2 out[2][3])
{
    static_assert(TAIL == TAILK_PQ_LUT || TAIL == TAILK_HLG || TAIL == TAILK_NONE, "tails the twin is planned for");
    f2 rgbc[2][3];
#pragma unroll
    for (int rr = 0; rr < 2; rr++) {              // rr = luma column of the block
        // the odd column's Ucol / Vcol are twice its chroma (convert_block_bp) and meet the halved coefficients HH = {m2, m4, m5, m7} / 2:
        // fma(m / 2, 2x, acc) is fma(m, x, acc) bit for bit, halving and doubling being exact
        const f2 *KK = rr ? HH : MM;
        const int k2 = rr ? 0 : 2, k4 = rr ? 1 : 4, k5 = rr ? 2 : 5, k7 = rr ? 3 : 7;
        rgbc[rr][0] = fma_k<true>(MM, 0, Ycol[rr], fma_k<false>(KK, k2, Vcol[rr], CC[0]));
        rgbc[rr][1] = fma_k<true>(MM, 3, Ycol[rr], fma_k<false>(KK, k4, Ucol[rr], fma_k<false>(KK, k5, Vcol[rr], CC[1])));
        rgbc[rr][2] = fma_k<true>(MM, 6, Ycol[rr], fma_k<false>(KK, k7, Ucol[rr], CC[2]));
    }
    if constexpr (!tail_has_table(TAIL)) {
#pragma unroll
        for (int rr = 0; rr < 2; rr++)
#pragma unroll
            for (int ch = 0; ch < 3; ch++) out[rr][ch] = rgbc[rr][ch];
        return;
    } else {
        // all twelve table reads of the block are issued together (their addresses depend only on the matrix results)
        f2 linc[2][3];
        f2 ent[2][3][2]; float frc[2][3][2];
#pragma unroll
        for (int rr = 0; rr < 2; rr++)
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const float t = rgbc[rr][ch][e] * (float)(LUT_N - 1);
                    frc[rr][ch][e] = __builtin_amdgcn_fractf(t);
                    ent[rr][ch][e] = T[(int)t];
                }
#pragma unroll
        for (int rr = 0; rr < 2; rr++)
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    // {value, slope} entry: VOP3 v_fma_f32 as in convert_block_yuv.  VOP2 v_fmac_f32 accumulates onto the value's own
                    // register, the low half of the pair its ds_read_b64 filled, and the results have to stand in pairs of their own for
                    // the packed matrix behind them: tried, it compiled to one v_mov_b32 per lerp (12 per iteration) and was taken back
                    float r;
                    asm("v_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(ent[rr][ch][e].y), "v"(frc[rr][ch][e]), "v"(ent[rr][ch][e].x));
                    linc[rr][ch][e] = r;
                }
#pragma unroll
        for (int rr = 0; rr < 2; rr++) {
            const f2 *lin = linc[rr];
            if constexpr (TAIL == TAILK_PQ_LUT) {
                // hable(ST2084ToLinear(x) * scale) / hable(4.8) came from the table; 2020 -> 709, saturate and pow 1/2.2 in ALU
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const f2 g = fma_k<true>(GG, 3 * ch, lin[0], fma_k<false>(GG, 3 * ch + 1, lin[1], mul_k(GG, 3 * ch + 2, lin[2])));
                    out[rr][ch] = f2{hlsl_pow(g.x, 1.0f / 2.2f), hlsl_pow(g.y, 1.0f / 2.2f)};
                }
            } else {
                // HLG: inverse_HLG per channel came from the table; the rest as convert_block_yuv's TAILK_HLG branch has it
                const f2 ys = splat(2000.0f) * pk_fma(splat(0.2627f), lin[0], pk_fma(splat(0.6780f), lin[1], splat(0.0593f) * lin[2]));
                const float ks = P.lum_scale * (1.0f / 1000.0f);
                const f2 gain = f2{hlsl_pow(ys.x, 0.2f) * ks, hlsl_pow(ys.y, 0.2f) * ks};
                const float A_ = 0.15f, B_ = 0.50f, CB = 0.10f * 0.50f, DE = 0.20f * 0.02f, DF = 0.20f * 0.30f, EF = 0.02f / 0.30f;
                const float inv_div = 1.0f / (((4.8f * (A_ * 4.8f + CB) + DE) / (4.8f * (A_ * 4.8f + B_) + DF)) - EF);
                f2 tm[3];
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const f2 x = lin[ch] * gain;
                    const f2 num = pk_fma(x, pk_fma(splat(A_), x, splat(CB)), splat(DE));
                    const f2 den = pk_fma(x, pk_fma(splat(A_), x, splat(B_)), splat(DF));
                    const f2 q = f2{num.x * __builtin_amdgcn_rcpf(den.x), num.y * __builtin_amdgcn_rcpf(den.y)};
                    tm[ch] = (q - splat(EF)) * splat(inv_div);
                }
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const f2 g = fma_k<true>(GG, 3 * ch, tm[0], fma_k<false>(GG, 3 * ch + 1, tm[1], mul_k(GG, 3 * ch + 2, tm[2])));
                    out[rr][ch] = f2{hlsl_pow(g.x, 1.0f / 2.2f), hlsl_pow(g.y, 1.0f / 2.2f)};
                }
            }
        }
    }
}

// convert_block (vp_fused_dev.h) for the twin: the block's luma and ONE new chroma texel (column c0, row n + 1) from `u`, row n from
// `keep` (FIRST: from u.v[3], a segment's first convert), column c0 + 1 from the next lane.  sy0 / sy1 as convert_block takes them.
template <int TAIL, int SRC, bool FIRST>
__device__ __forceinline__ void convert_block_bp(const FusedArgs &P, const f2 (&MM)[5], const f2 (&HH)[2], const f2 (&GG)[5], const f2 (&CC)[3], const RawUnseenBp &u, ChromaCarry &keep,
                                                 int sy0, int sy1, const f2 *T, f2 out[2][3])
{
    // vertical weights of chroma rows n (w0) and n+1 (w1) for (row 0, row 1): wave-uniform, one SGPR pair each
    const int n4 = chroma_v4(P, sy0) & ~3;
    const int fr0 = chroma_v4(P, sy0) - n4, fr1 = chroma_v4(P, sy1) - n4;
    const f2 w1 = f2{quarter(fr0), quarter(fr1)}, w0 = f2{quarter(4 - fr0), quarter(4 - fr1)};
    const ChromaCarry bot = chroma_floats<SRC>(u.v[2]);
    ChromaCarry top = keep;
    if constexpr (FIRST) top = chroma_floats<SRC>(u.v[3]);
    keep = bot;
    f2 Ucol[2], Vcol[2], Ycol[2];
    Ucol[0] = pk_fma(splat(bot.u), w1, splat(top.u) * w0);       // column c0 as (row 0, row 1) pairs: the even luma column's chroma
    Vcol[0] = pk_fma(splat(bot.v), w1, splat(top.v) * w0);
    const f2 Un = from_next_lane(Ucol[0]), Vn = from_next_lane(Vcol[0]);      // column c0 + 1: the next lane's c0
    if constexpr (SRC == SRC_P01X) {
        Ycol[0] = f2{(float)(u.v[0] & 0xffffu), (float)(u.v[1] & 0xffffu)};
        Ycol[1] = f2{(float)(u.v[0] >> 16), (float)(u.v[1] >> 16)};
    } else {
        Ycol[0] = f2{(float)(u.v[0] & 0xffu), (float)(u.v[1] & 0xffu)};
        Ycol[1] = f2{(float)((u.v[0] >> 8) & 0xffu), (float)((u.v[1] >> 8) & 0xffu)};
    }
    // the odd luma column's chroma is fma(Un, 0.5, Ucol[0] * 0.5) (cw_own == cw_next == 0.5: FusedUp2xBpTakes) = 0.5 * RNE(Un + Ucol[0]),
    // scaling by a half being exact: the sum goes on as it is and the halving into the matrix coefficients it meets (HH)
    Ucol[1] = Un + Ucol[0];
    Vcol[1] = Vn + Vcol[0];
    convert_block_yuv_bp<TAIL>(P, MM, HH, GG, CC, Ycol, Ucol, Vcol, T, out);
}

}  // namespace

}  // namespace mpcvr
