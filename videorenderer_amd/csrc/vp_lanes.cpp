// vp_lanes.cpp — FrameLanes (vp_lanes.h): which lane a frame or a batch takes, what it waits for, and what it leaves behind
#include "vp_lanes.h"

#include <cstdlib>
#include <utility>

namespace mpcvr {

// Four lanes: measured on MI355X with 4K P010 -> 8K frames (bench.py process_per_frame) — one lane 14.4 k frames/s, two 18.2 k, four
// 19.3 k; the kernels size their segments for that many frames side by side (FusedParams::inflight).
int FrameLanes::Count()
{
    static const int n = [] { const char *e = std::getenv("MPCVR_FRAME_LANES"); const int v = e && *e ? std::atoi(e) : 4; return v < 1 ? 1 : v > kFrameLanes ? kFrameLanes : v; }();
    return n;
}

int FrameLanes::PickFrameLane(const RtSpan &rt)
{
    Lane *pick = nullptr;
    hipEvent_t also[kFrameLanes];
    int n_also = 0;
    for (int li = 0; li < Count(); li++) {
        Lane &fl = m_lanes[li];
        hipEvent_t latest = nullptr;                 // the lane's most recent unfinished frame into rt's bytes (the ring is walked oldest first)
        for (int i = 0; i < kLaneDepth; i++) {
            Frame &f = fl.ring[(fl.head + i) % kLaneDepth];
            if (!f.pending || !f.rt.Overlaps(rt)) continue;  // (only a frame into the same memory is worth a driver call)
            if (hipEventQuery(f.done) == hipSuccess) { f.pending = false; continue; }
            latest = f.done;
        }
        if (!latest) continue;
        if (!pick) pick = &fl; else also[n_also++] = latest;
    }
    if (!pick) { pick = &m_lanes[m_frameNext]; m_frameNext = (m_frameNext + 1) % Count(); }
    if (!pick->stream && hipStreamCreateWithFlags(&pick->stream, hipStreamDefault) != hipSuccess) { pick->stream = nullptr; return -1; }
    for (int i = 0; i < n_also; i++) (void)hipStreamWaitEvent(pick->stream, also[i], 0);
    // ... and behind a whole batch still in flight on another lane that writes into this target's bytes (the pick's own batches: stream order)
    for (int li = 0; li < kFrameLanes; li++) {
        Lane &bl = m_lanes[li];
        if (!bl.batchPending || &bl == pick) continue;
        if (hipEventQuery(bl.batchDone) == hipSuccess) { bl.batchPending = false; bl.batchSpans.clear(); continue; }
        if (SpansOverlap(bl.batchSpans, rt)) (void)hipStreamWaitEvent(pick->stream, bl.batchDone, 0);
    }
    return (int)(pick - m_lanes);
}

int FrameLanes::PickBatchLane(std::vector<RtSpan> &&written, int *waits)
{
    Lane *pick = &m_lanes[m_batchNext];
    if (!pick->stream && hipStreamCreateWithFlags(&pick->stream, hipStreamDefault) != hipSuccess) { pick->stream = nullptr; return -1; }
    // (two lanes: MPCVR_BATCH_LANE_COUNT = 2 .. 8 for the A/B — profiles/r06/batch_lane_count_call34.txt)
    static const int count = [] { const char *e = std::getenv("MPCVR_BATCH_LANE_COUNT"); const int v = e && *e ? std::atoi(e) : kBatchLanes; return v < 2 ? 2 : v > kFrameLanes ? kFrameLanes : v; }();
    m_batchNext = (m_batchNext + 1) % count;
    std::vector<RtSpan> &spans = m_batchSpans;
    spans = std::move(written);
    SortAndMergeSpans(spans);
    for (Lane &fl : m_lanes) {
        if (&fl == pick || !fl.stream) continue;
        for (Frame &f : fl.ring) {
            if (!f.pending) continue;
            if (hipEventQuery(f.done) == hipSuccess) { f.pending = false; continue; }
            if (SpansOverlap(spans, f.rt)) { (void)hipStreamWaitEvent(pick->stream, f.done, 0); ++*waits; }
        }
        if (!fl.batchPending) continue;
        if (hipEventQuery(fl.batchDone) == hipSuccess) { fl.batchPending = false; fl.batchSpans.clear(); continue; }
        if (SpanListsOverlap(spans, fl.batchSpans)) { (void)hipStreamWaitEvent(pick->stream, fl.batchDone, 0); ++*waits; }
    }
    return (int)(pick - m_lanes);
}

// its completion event, and its spans (m_batchSpans, from PickBatchLane) joined to those of the lane's batches still in flight
void FrameLanes::NoteLaneBatch(int lane)
{
    Lane *fl = &m_lanes[lane];
    if (!fl->batchDone && hipEventCreateWithFlags(&fl->batchDone, hipEventDisableTiming) != hipSuccess) { fl->batchDone = nullptr; (void)hipStreamSynchronize(fl->stream); return; }
    if (fl->batchPending && hipEventQuery(fl->batchDone) == hipSuccess) fl->batchPending = false;
    if (!fl->batchPending) fl->batchSpans.clear();
    fl->batchSpans.insert(fl->batchSpans.end(), m_batchSpans.begin(), m_batchSpans.end());
    SortAndMergeSpans(fl->batchSpans);
    (void)hipEventRecord(fl->batchDone, fl->stream);
    fl->batchPending = true;
    fl->last = fl->batchDone;
}

// its completion event takes the ring's oldest slot (whose frame must have completed)
void FrameLanes::NoteLaneFrame(int lane, const RtSpan &rt)
{
    Lane *fl = &m_lanes[lane];
    Frame &f = fl->ring[fl->head];
    fl->head = (fl->head + 1) % kLaneDepth;
    if (!f.done && hipEventCreateWithFlags(&f.done, hipEventDisableTiming) != hipSuccess) { f.done = nullptr; (void)hipStreamSynchronize(fl->stream); return; }
    if (f.pending) (void)hipEventSynchronize(f.done);
    f.rt = rt; f.pending = true;
    (void)hipEventRecord(f.done, fl->stream);
    fl->last = f.done;
}

// the context stream -> lane edge (see NoteStreamWork): one event record per generation of context-stream work, one wait per lane
void FrameLanes::LaneWaitsForStream(int lane, hipStream_t ctx)
{
    Lane *fl = &m_lanes[lane];
    if (fl->seenGen == m_streamGen || !ctx) return;
    if (m_markGen != m_streamGen) {
        if (!m_evStreamMark && hipEventCreateWithFlags(&m_evStreamMark, hipEventDisableTiming) != hipSuccess) m_evStreamMark = nullptr;
        if (!m_evStreamMark || hipEventRecord(m_evStreamMark, ctx) != hipSuccess) {       // no event: the host waits instead
            (void)hipStreamSynchronize(ctx);
            for (Lane &l : m_lanes) l.seenGen = m_streamGen;
            return;
        }
        m_markGen = m_streamGen;
    }
    (void)hipStreamWaitEvent(fl->stream, m_evStreamMark, 0);
    fl->seenGen = m_streamGen;
}

hipError_t FrameLanes::Join(bool host_wait, hipStream_t ctx)
{
    hipError_t err = hipSuccess;
    for (Lane &fl : m_lanes) {
        if (!fl.stream || !fl.last) continue;
        if (host_wait) {
            const hipError_t e = hipStreamSynchronize(fl.stream);
            if (e != hipSuccess) err = e;
            for (Frame &f : fl.ring) f.pending = false;
            fl.batchPending = false; fl.batchSpans.clear();
            fl.last = nullptr;
        } else if (ctx) (void)hipStreamWaitEvent(ctx, fl.last, 0);
    }
    return err;
}

void FrameLanes::Release()
{
    if (m_evStreamMark) (void)hipEventDestroy(m_evStreamMark);
    for (Lane &fl : m_lanes) {
        if (fl.stream) { (void)hipStreamSynchronize(fl.stream); (void)hipStreamDestroy(fl.stream); }
        for (Frame &f : fl.ring) if (f.done) (void)hipEventDestroy(f.done);
        if (fl.batchDone) (void)hipEventDestroy(fl.batchDone);
    }
}

}  // namespace mpcvr
