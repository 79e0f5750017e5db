// vp_lanes.h — FrameLanes: the streams beside the context stream that frames and whole batches of one context overlap on, and the
// bookkeeping that keeps writes into the same memory in order.  WHICH frames and batches may take a lane is the processor's decision
// (CHipVideoProcessor::FrameLanesUsable, BatchLaneEligible: it depends on the plan); this class only answers where and behind what.
//
// mpcvr_process frame after frame (the reference's own call pattern, Render -> Process, DX11VideoProcessor.cpp:2730): a single 4K
// frame is one round of waves on this part, so a kernel's ramp-up and drain cost a third of its time when frames run strictly one
// after the other.  Frames are independent (a D3D11 driver overlaps draws into different render targets as well): a context that
// owns its stream deals consecutive frames to four lanes whose kernels overlap; everything that can observe a result
// (mpcvr_synchronize, the snapshot, a batch, a plan change, a new stream) joins them first.  The lane streams are BLOCKING streams
// like the context's own (CHipVideoProcessor::Init), so work on the legacy default stream stays ordered against them.
#pragma once
#include <hip/hip_runtime_api.h>

#include <vector>

#include "vp_spans.h"

namespace mpcvr {

class FrameLanes {
public:
    static constexpr int kFrameLanes = 8;         // built; Count() of them are used (4 unless MPCVR_FRAME_LANES says otherwise)
    static int Count();
    // every frame queued on a lane leaves (render target, completion event) in the lane's ring; a slot is reused only after its frame has
    // completed, which also bounds how far the host runs ahead (kFrameLanes x kLaneDepth frames)
    static constexpr int kLaneDepth = 8;
    // (round 6) WHOLE BATCHES take turns on the first two lanes as well (ProcessBatch on a context that owns its stream, a plan that is one
    // launch per batch with no intermediate surface): two launches in flight fill each other's ramp-up and tail — same box, 32-frame batches:
    // 4K -> 8K 22.6 k -> 23.5 k frames/s, 1080p -> 1440p 99.4 k -> 115.6 k (profiles/r06/final4/bench_workloads.jsonl).
    static constexpr int kBatchLanes = 2;

    // A lane is named by its index (what GetLastBatchInfo reports), -1: none.
    // The lane of the frame about to be queued: one that still holds a frame into memory this one's render target overlaps if there is one
    // (stream order then keeps the two writes apart; further lanes holding such a frame are waited for), else the next in turn.  -1: no stream
    int PickFrameLane(const RtSpan &rt);
    // the lane of the batch about to be queued (the batch lanes take turns), ordered behind everything still in flight on OTHER lanes that
    // writes into the bytes of `spans`: single frames (their ring entries) and batches; *waits grows by the number of such writers.  -1: no stream
    // spans (any order, overlaps allowed; taken over): what the batch writes for the caller — the render targets of mpcvr_process_batch; of a chunk of
    // mpcvr_process_batch_yuv the planes it leaves, not the context-owned surface it renders into on the way (the lane's own: stream order covers it)
    int PickBatchLane(std::vector<RtSpan> &&spans, int *waits);
    hipStream_t Stream(int lane) const { return m_lanes[lane].stream; }
    void NoteLaneFrame(int lane, const RtSpan &rt);   // the frame just queued on the lane writes `rt`
    void NoteLaneBatch(int lane);                     // the batch PickBatchLane picked the lane for has been queued on it
    // work queued on the CONTEXT stream (a batch, a frame that ran off the lanes, a sample copy / repack, a read-back) since a lane last
    // waited for it: every such call bumps the generation; a lane whose seenGen is behind waits for an event recorded on the context stream
    // (recorded once per generation) before its next frame — a lane frame into the render target, or out of the sample, that the context
    // stream is still writing or reading can then neither overtake nor overlap it (mpcvr.h: frames into overlapping memory stay in order)
    void NoteStreamWork() { m_streamGen++; }
    void LaneWaitsForStream(int lane, hipStream_t ctx);
    // host_wait: block until the lanes are idle (the last failure, if any, is returned); otherwise the context stream waits for them
    // (work queued on it afterwards runs behind every frame in flight)
    hipError_t Join(bool host_wait, hipStream_t ctx);
    void Release();            // waits for the lanes and destroys their streams and events: once, the lanes are not used afterwards

private:
    struct Frame { RtSpan rt; hipEvent_t done = nullptr; bool pending = false; };
    // last: the event behind the frame or batch queued last (Join); seenGen: the generation of context-stream work the lane last waited for (trails
    // m_streamGen); batchSpans: the bytes the render targets of the lane's batches still in flight cover (sorted, disjoint: spans that touch are
    // merged), batchDone: the event behind the last of them
    struct Lane { hipStream_t stream = nullptr; Frame ring[kLaneDepth]; int head = 0; hipEvent_t last = nullptr; unsigned seenGen = 0;
                  std::vector<RtSpan> batchSpans; hipEvent_t batchDone = nullptr; bool batchPending = false; };
    Lane m_lanes[kFrameLanes];
    int m_frameNext = 0, m_batchNext = 0;         // whose turn it is
    std::vector<RtSpan> m_batchSpans;             // the batch being queued (PickBatchLane fills it, NoteLaneBatch files it)
    unsigned m_streamGen = 0, m_markGen = ~0u;
    hipEvent_t m_evStreamMark = nullptr;
};

}  // namespace mpcvr
