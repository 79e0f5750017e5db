// vp_plan_tables.h — the tables of one plan as host values: what lies between DecidePlan and the first upload.  The geometry of the
// rotation-carrying draw, the tap tables of both draws packed one buffer per axis, and the strip / periodic kernels' tables.  No device
// work and no HIP header: the processor uploads a pack with one copy and reads it through a view; the C-ABI hands the same packs to the
// CPU tests (mpcvr_plan_draw_tables).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "vp_plan.h"

namespace mpcvr {

// every sub-table of an axis pack starts on a 256-byte boundary of the pack (what each had as an allocation of its own)
enum { kPackAlignWords = 64 };

// One axis' tap tables in one buffer of 4-byte words: idx | w | wsum | other | block pack, word offsets below.
// Block pack: blk_lo | pad to 64 words | idx_t | w_t | blk8_lo | blk32_lo.
struct AxisPack {
    std::vector<int32_t> words;                                  // empty: the draw has no tap tables (none planned, or the 2-D Jinc2m shader)
    size_t offIdx = 0, offW = 0, offWsum = 0, offOther = 0, offBlk = 0;
    size_t nOther = 0;                                           // entries of the unfiltered axis' index map
    int ntaps = 0, normalise = 0, n_out = 0;
    int blk_span = 0, blk8_span = 0, blk32_span = 0;
    int other_identity = 1;
    size_t Bytes() const { return words.size() * sizeof(int32_t); }
    // the kernel-side struct over the pack's copy at devBase; an empty pack gives nulls and zeros whatever devBase is
    AxisTaps View(const void *devBase) const;
    const int32_t *Other(const void *devBase) const { return words.empty() || !devBase ? nullptr : (const int32_t *)devBase + offOther; }
};
AxisPack PackAxisTaps(const HostAxisTaps &h, const std::vector<int32_t> &other);

// the strip kernel's tables, and behind them the periodic kernel's (none: its offsets stay 0), in one buffer of 4-byte words
struct StripPack {
    std::vector<int32_t> words;
    size_t stripOff[6] = {0, 0, 0, 0, 0, 0};      // yrange | xstrip | xi_t | xw_t | yi | yw
    size_t periodOff[4] = {0, 0, 0, 0};           // xi_t | xw_t | yw | xstrip
};
StripPack PackStripTables(const StripPlan &sp, const PeriodPlan *pp);

struct PlanTables {
    DrawCoords firstCoords{}, secondCoords{};
    int firstAxis = 0;             // screen axis the first draw's tap table runs along
    bool firstSwap = false;        // rotation 90/270: taps address the other texture axis
    bool firstJinc = false, secondJinc = false;    // the draw runs the 2-D Jinc2m shader
    AxisPack x, y;                 // first and second draw
    bool stripPlanned = false;     // the arbitrary-ratio fused kernel's tables exist (strip, stripPack)
    StripPlan strip;
    PeriodPlan period;             // P == 0: not a periodic geometry
    StripPack stripPack;
};

// m_PSConvColorData.bEnable — DX11VideoProcessor.cpp:849-853: interleaved RGB skips the convert draw unless brightness
// or contrast are set (hue / saturation do not count); Dolby Vision always converts (:834)
bool ConvertDrawEnabled(const FmtConvParams &f, const ProcAmp &pa, bool dovi);

struct PlanTablesInput {
    int srcLeft = 0, srcTop = 0, srcRectW = 0, srcRectH = 0;     // source rect
    int texW = 0, texH = 0;        // the whole source texture
    int outW = 0, outH = 0;        // video rect size
    int iUpscaling = 0;            // Settings_t fields the tables depend on
    uint32_t flags = 0;
    bool heavyConvert = false;     // the convert stage carries a table tail (PQ / HLG -> SDR)
    bool noStrip = false;          // MPCVR_NO_STRIP
};
// false + *why: a resize ratio outside what the tap tables support
bool BuildPlanTables(const PassPlan &plan, const PlanTablesInput &in, PlanTables *out, std::string *why);

}  // namespace mpcvr
