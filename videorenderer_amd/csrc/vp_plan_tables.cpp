// vp_plan_tables.cpp — see vp_plan_tables.h.  Built with -ffp-contract=off like vp_plan.cpp: the fp32 steps below feed the tap tables.
#include "vp_plan_tables.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace mpcvr {

// hint for the folded resize kernels: the smallest source index of every block of `block` outputs, and the widest block's window
static std::vector<int32_t> BlockLows(const HostAxisTaps &h, size_t nOut, size_t block, int *span)
{
    std::vector<int32_t> lo((nOut + block - 1) / block);
    *span = 0;
    for (size_t b = 0; b < lo.size(); b++) {
        const size_t first = b * block * (size_t)h.ntaps, last = std::min(nOut, (b + 1) * block) * (size_t)h.ntaps;
        const auto mm = std::minmax_element(h.idx.begin() + first, h.idx.begin() + last);
        lo[b] = *mm.first;
        *span = std::max(*span, *mm.second - *mm.first + 1);
    }
    return lo;
}

AxisPack PackAxisTaps(const HostAxisTaps &h, const std::vector<int32_t> &other)
{
    AxisPack p;
    p.ntaps = h.ntaps; p.normalise = h.normalise;
    const size_t cnt = h.idx.size(), nOut = h.ntaps > 0 ? cnt / (size_t)h.ntaps : 0;
    // a sub-table of `words` words at the next 256-byte boundary; returns its offset
    auto place = [&p](const void *src, size_t words) {
        const size_t at = (p.words.size() + kPackAlignWords - 1) / kPackAlignWords * kPackAlignWords;
        p.words.resize(at + words);
        if (words) std::memcpy(p.words.data() + at, src, words * 4);
        return at;
    };
    p.offIdx = place(h.idx.data(), cnt);
    p.offW = place(h.w.data(), h.w.size());
    if (h.normalise) p.offWsum = place(h.wsum.data(), h.wsum.size());
    p.nOther = other.size();
    p.offOther = place(other.data(), other.size());
    if (nOut > 0) {
        const std::vector<int32_t> lo = BlockLows(h, nOut, 64, &p.blk_span), lo8 = BlockLows(h, nOut, 8, &p.blk8_span),
                                   lo32 = BlockLows(h, nOut, 32, &p.blk32_span);
        // tap-major copies of both tables and the 8- / 32-output block tables behind the block table
        const size_t off = (lo.size() + 63) / 64 * 64;
        std::vector<int32_t> blk(off + 2 * cnt + lo8.size() + lo32.size());
        std::copy(lo8.begin(), lo8.end(), blk.begin() + off + 2 * cnt);
        std::copy(lo32.begin(), lo32.end(), blk.begin() + off + 2 * cnt + lo8.size());
        std::copy(lo.begin(), lo.end(), blk.begin());
        for (size_t f = 0; f < nOut; f++)
            for (int k = 0; k < h.ntaps; k++) {
                blk[off + (size_t)k * nOut + f] = h.idx[f * h.ntaps + k];
                std::memcpy(&blk[off + cnt + (size_t)k * nOut + f], &h.w[f * h.ntaps + k], sizeof(float));
            }
        p.offBlk = place(blk.data(), blk.size());
        p.n_out = (int)nOut;
    }
    p.other_identity = 1;
    for (size_t i = 0; i < other.size(); i++)
        if (other[i] != (int32_t)i) { p.other_identity = 0; break; }
    return p;
}

AxisTaps AxisPack::View(const void *devBase) const
{
    AxisTaps t{};
    t.other_identity = other_identity;
    if (words.empty() || !devBase) return t;
    const int32_t *base = (const int32_t *)devBase;
    t.idx = base + offIdx; t.w = (const float *)(base + offW);
    t.wsum = normalise ? (const float *)(base + offWsum) : nullptr;
    t.ntaps = ntaps; t.normalise = normalise;
    if (n_out > 0) {
        const size_t cnt = (size_t)n_out * ntaps, nLo = ((size_t)n_out + 63) / 64, nLo8 = ((size_t)n_out + 7) / 8;
        t.blk_lo = base + offBlk; t.blk_span = blk_span;
        t.idx_t = t.blk_lo + (nLo + 63) / 64 * 64; t.w_t = (const float *)(t.idx_t + cnt); t.n_out = n_out;
        t.blk8_lo = t.idx_t + 2 * cnt; t.blk8_span = blk8_span;
        t.blk32_lo = t.blk8_lo + nLo8; t.blk32_span = blk32_span;
    }
    return t;
}

StripPack PackStripTables(const StripPlan &sp, const PeriodPlan *pp)
{
    StripPack s;
    std::vector<int32_t> &pack = s.words;
    auto put = [&pack](const void *src, size_t words) {
        const size_t at = pack.size();
        pack.resize(at + words);
        if (words) std::memcpy(pack.data() + at, src, words * 4);
        return at;
    };
    s.stripOff[0] = put(sp.yrange.data(), sp.yrange.size());
    s.stripOff[1] = put(sp.xstrip.data(), sp.xstrip.size());
    s.stripOff[2] = put(sp.xi_t.data(), sp.xi_t.size());
    s.stripOff[3] = put(sp.xw_t.data(), sp.xw_t.size());
    s.stripOff[4] = put(sp.yi.data(), sp.yi.size());
    s.stripOff[5] = put(sp.yw.data(), sp.yw.size());
    if (pp) {
        s.periodOff[0] = put(pp->xi_t.data(), pp->xi_t.size());
        s.periodOff[1] = put(pp->xw_t.data(), pp->xw_t.size());
        while (pack.size() & 7) pack.push_back(0);                      // the weight rows (32 bytes each) are read with scalar multi-dword loads
        s.periodOff[2] = put(pp->yw.data(), pp->yw.size());
        s.periodOff[3] = put(pp->xstrip.data(), pp->xstrip.size());
    }
    return s;
}

bool ConvertDrawEnabled(const FmtConvParams &f, const ProcAmp &pa, bool dovi)
{
    if (dovi) return true;
    if (f.CSType == CST_YUV || f.CSType == CST_GRAY || (f.CSType == CST_RGB && f.planes == 3)) return true;
    return std::fabs(pa.brightness / 255) > 1e-4f || std::fabs(pa.contrast - 1.0f) > 1e-4f;
}

bool BuildPlanTables(const PassPlan &plan, const PlanTablesInput &in, PlanTables *out, std::string *why)
{
    *out = PlanTables{};
    PlanTables &t = *out;
    const int w1 = in.srcRectW, h1 = in.srcRectH, w2 = in.outW, h2 = in.outH;
    HostAxisTaps hx, hy;
    std::vector<int32_t> ox, oy;
    if (plan.two_pass || plan.one_pass) {
        // The rotation-carrying draw (TextureResizeShader / TextureCopyRect with FillVertices' rotation and flip,
        // :130-179): which texture coordinate runs along which screen axis, and in which direction
        //     rot   0: U = l + a(r-l)  V = t + b(bm-t)      rot  90: U = l + b(r-l)  V = bm - a(bm-t)
        //     rot 180: U = r - a(r-l)  V = bm - b(bm-t)     rot 270: U = r - b(r-l)  V = t + a(bm-t)     flip: l <-> r
        const int rot = plan.rotation;
        const bool swap = rot == 90 || rot == 270;
        const int tax = swap ? 1 : 0;                               // texture axis run through by screen x
        bool rev_u = rot == 180 || rot == 270;
        const bool rev_v = rot == 90 || rot == 180;
        if (plan.flip) rev_u = !rev_u;
        const bool rev_x = tax == 0 ? rev_u : rev_v, rev_y = tax == 0 ? rev_v : rev_u;
        const int len_x = tax == 0 ? w1 : h1, len_y = tax == 0 ? h1 : w1;       // extent of the source rect along x / y
        // source of the draw: the convert output (rect at the origin) or, with the convert draw disabled, the source
        // texture itself with rSrc = srcRect (:3321-3323); clamp addressing covers the whole texture
        const bool fromTex = !plan.convert;
        const int ol = fromTex ? in.srcLeft : 0, ot = fromTex ? in.srcTop : 0;
        const int tw = fromTex ? in.texW : w1, th = fromTex ? in.texH : h1;
        const int org_x = tax == 0 ? ol : ot, org_y = tax == 0 ? ot : ol;
        const int tex_x = tax == 0 ? tw : th, tex_y = tax == 0 ? th : tw;
        const int outW = w2, outH = plan.two_pass ? plan.mid_h : h2;
        const int a = plan.first_tex_axis;
        // scale[AXIS] as TextureResizeShader sets it: srcRect/dstRect of the same-named screen dimension (:351-354)
        const float cscale = a == 0 ? (float)w1 / (float)outW : (float)h1 / (float)outH;
        const bool taps_on_x = (a < 0) || (tax == a);               // ps_simple: a 1-tap table along x
        const Resizer rs = a < 0 ? Resizer{RS_NONE, 0} : plan.first_rs;
        t.firstJinc = rs.kind == RS_UP && rs.method == MPCVR_UPSCALE_Jinc2;
        t.firstCoords = DrawCoords{org_x, len_x, rev_x ? 1 : 0, (float)len_x / (float)outW,
                                   org_y, len_y, rev_y ? 1 : 0, (float)len_y / (float)outH, swap ? 1 : 0, tex_x, tex_y, outW, outH};
        bool ok = true;
        if (t.firstJinc) {
            // the 2-D shader needs no tables
        } else
        if (taps_on_x) {
            ok = BuildAxisTaps(rs, org_x, len_x, outW, tex_x, in.flags, &hx, rev_x, a < 0 ? 0.0f : cscale);
            BuildPointIndex(org_y, len_y, outH, tex_y, &ox, rev_y);
        } else {
            ok = BuildAxisTaps(rs, org_y, len_y, outH, tex_y, in.flags, &hx, rev_y, cscale);
            BuildPointIndex(org_x, len_x, outW, tex_x, &ox, rev_x);
        }
        if (!ok) { *why = "resize ratio outside the supported range"; return false; }
        t.firstAxis = taps_on_x ? 0 : 1;
        t.firstSwap = swap;
        if (!t.firstJinc) t.x = PackAxisTaps(hx, ox);
    }
    if (plan.two_pass) {
        // m_TexResize: fp16, dst width x (source extent along screen y) (:3143-3160); the second draw is unrotated
        const int mh = plan.mid_h;
        t.secondJinc = plan.ry.kind == RS_UP && plan.ry.method == MPCVR_UPSCALE_Jinc2;
        t.secondCoords = DrawCoords{0, w2, 0, 1.0f, 0, mh, 0, (float)mh / (float)h2, 0, w2, mh, w2, h2};
        if (!t.secondJinc) {
            if (!BuildAxisTaps(plan.ry, 0, mh, h2, mh, in.flags, &hy)) { *why = "resize ratio outside the supported range"; return false; }
            BuildPointIndex(0, w2, w2, w2, &oy);     // Y pass: columns map 1:1
            t.y = PackAxisTaps(hy, oy);
        }
    }

    // the arbitrary-ratio fused kernel takes an unrotated two-pass resize whose tables fit it.  A horizontal flip (FillVertices swaps
    // src_l and src_r, DX11VideoProcessor.cpp:167-169) is the X draw's table read from the other end — per-column tap indices and
    // weights are what these kernels read anyway — so a flipped frame stays on the fused path.  Rotation 180 also reverses the first
    // draw's ROW map (the pack's `other`), which the surface variant reads row by row.  90 / 270 turn the first draw into a Y shader
    // and stay per draw
    if (!in.noStrip && plan.two_pass && !t.firstJinc && !t.secondJinc && t.firstAxis == 0 && !t.firstSwap && (plan.rotation == 0 || plan.rotation == 180) &&
        !(in.flags & (MPCVR_FLAG_NO_FUSED | MPCVR_FLAG_NO_FAST_CONVERT | MPCVR_FLAG_NO_STRIP)) &&
        PlanFusedStrip(hx, hy, w2, h2, plan.convert ? w1 : in.texW, plan.mid_h, &t.strip)) {
        // periodic vertical ratio (1080p -> 1440p, 720p -> 1080p, 4K -> 1440p, 4K -> 1080p ...): the register-window kernel's tables
        const bool q1 = plan.rx.kind == RS_UP && plan.ry.kind == RS_UP && in.iUpscaling == MPCVR_UPSCALE_Lanczos3 && !(in.flags & MPCVR_FLAG_LANCZOS3_FIXED);
        // (an interleaved RGB sample without a convert draw is read in place: the X tables then index the whole texture's columns)
        const bool periodic = plan.rx.kind == RS_UP && plan.ry.kind == RS_UP &&
                              PlanFusedPeriod(hx, hy, w2, h2, plan.convert ? w1 : in.texW, plan.mid_h, q1, &t.period, in.heavyConvert);
        if (!periodic) t.period = PeriodPlan{};
        t.stripPack = PackStripTables(t.strip, periodic ? &t.period : nullptr);
        t.stripPlanned = true;
    } else {
        t.strip = StripPlan{};
    }
    return true;
}

}  // namespace mpcvr
