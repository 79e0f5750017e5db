// hip_video_processor_ext.cpp — the EXTENSIONS of CHipVideoProcessor (no reference line anywhere in this file): frames as NV12 / P010, their
// histograms, frames as float tensors, float tensors as samples, deinterlacing at field rate, frames through a 3D LUT.  Each is a free function that checks and launches
// one pass (EncodeSurface, MeasureSurface, TensorSurface, SampleSurface, DeintSurface, Lut3dSurface), a per-sample call and a batch call; the batch calls share
// two chunk loops (RunSurfaceChunks, RunSampleChunks), the per-sample calls CopySample's upload slots (AcquireUploadSlot / PublishUploadSlot).
#include "hip_video_processor.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace mpcvr {

// ------------------------------------------------------------------------------------------------
// EXTENSION — the frame as NV12 / P010 for an encoder (include/mpcvr.h: mpcvr_encode_pass, mpcvr_render_yuv; kernel: vp_encode.hip).
// No reference line: the reference has no RGB -> YUV path.
// ------------------------------------------------------------------------------------------------
// What a k_encode420 launch is given, but for its pointers: the caller adds src / y / uv or the frame table, and takes src16 / dst8 back
// where a pointer of the launch is off 16 / 8 bytes (here they say what the pitches allow)
static EncodeParams EncodeLaunchParams(const EncodePlan &plan, int w, int h, int srcPitch, int yPitch, int uvPitch)
{
    EncodeParams p{};
    p.src_pitch = srcPitch; p.y_pitch = yPitch; p.uv_pitch = uvPitch;
    p.w = w; p.h = h;
    std::memcpy(p.coef, plan.coef, sizeof(p.coef));
    std::memcpy(p.off, plan.off, sizeof(p.off));
    p.src16 = (srcPitch & 15) == 0;
    p.dst8 = ((yPitch | uvPitch) & 7) == 0;
    return p;
}

HRESULT EncodeSurface(const void *src, int srcPitch, int srcFmt, int w, int h, int outCformat, uint32_t extfmt, void *yPlane, int yPitch,
                      void *uvPlane, int uvPitch, hipStream_t stream, bool checkOnly, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    if ((!src && !checkOnly) || !yPlane || !uvPlane) { *why = "null surface or plane"; return MPCVR_E_POINTER; }      // (checkOnly: a source still to be allocated)
    if (w < 2 || h < 2 || ((w | h) & 1) || w > 32768 || h > 32768) { *why = "width and height must be even, 2 .. 32768"; return MPCVR_E_INVALIDARG; }
    EncodePlan plan;
    if (!PlanEncode(outCformat, srcFmt, extfmt, w, h, &plan)) { *why = "output NV12 or P010 with a YCbCr description, source BGRA8 or RGB10A2"; return MPCVR_E_INVALIDARG; }
    const int rowBytes = plan.out10 ? 2 * w : w;        // of the Y plane and of the UV plane alike (w / 2 pairs)
    if (srcPitch < 4 * w || yPitch < rowBytes || uvPitch < rowBytes) { *why = "pitch smaller than a row"; return MPCVR_E_INVALIDARG; }
    if (((uintptr_t)src | (uintptr_t)yPlane | (uintptr_t)uvPlane | (uintptr_t)srcPitch | (uintptr_t)yPitch | (uintptr_t)uvPitch) & 3) {
        *why = "surface, planes and pitches must be multiples of 4"; return MPCVR_E_INVALIDARG;
    }
    const RtSpan s = RowsSpan(src, (size_t)srcPitch, h, (size_t)4 * w);
    const RtSpan y = RowsSpan(yPlane, (size_t)yPitch, h, (size_t)rowBytes), c = RowsSpan(uvPlane, (size_t)uvPitch, h / 2, (size_t)rowBytes);
    if (y.Overlaps(c) || (src && (y.Overlaps(s) || c.Overlaps(s)))) { *why = "the planes overlap each other or the source"; return MPCVR_E_INVALIDARG; }
    if (checkOnly) return MPCVR_S_OK;
    EncodeParams p = EncodeLaunchParams(plan, w, h, srcPitch, yPitch, uvPitch);
    p.src = (const uint8_t *)src; p.y = (uint8_t *)yPlane; p.uv = (uint8_t *)uvPlane;
    p.src16 &= (s.lo & 15) == 0;
    p.dst8 &= ((y.lo | c.lo) & 7) == 0;
    if (LaunchEncode420(p, plan.in10, plan.out10, plan.siting, stream) != hipSuccess) { *why = "k_encode420 launch failed"; return MPCVR_E_FAIL; }
    return MPCVR_S_OK;
}

// Render, then the pass over the whole window behind it.  The frame stays off the lanes (like the snapshot's): the pass reads the back
// buffer, and the lanes' bookkeeping orders WRITES into the same memory — a following Render on another lane would not wait for a reader.
// On the context stream everything queued later, lanes included (NoteStreamWork), runs behind the pass.
HRESULT CHipVideoProcessor::RenderYuv(int /*field*/, int outCformat, uint32_t extfmt, void *yPlane, int yPitch, void *uvPlane, int uvPitch)
{
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    (void)hipSetDevice(m_device);
    const int w = m_windowRect.Width(), h = m_windowRect.Height();
    if (w < 2 || h < 2 || ((w | h) & 1)) return Fail(MPCVR_E_INVALIDARG, "a 4:2:0 frame needs an even window width and height");
    if (!m_curSample) return MPCVR_S_FALSE;          // nothing to draw, as Render
    // everything about the planes is answered before anything is drawn (a back buffer Render has yet to allocate cannot overlap them)
    const bool have = m_BackBuffer.ptr && m_BackBuffer.size >= (size_t)w * 4 * h;
    HRESULT hr;
    const char *why = "";
    if ((hr = EncodeSurface(have ? m_BackBuffer.ptr : nullptr, w * 4, m_cfg.output_format, w, h, outCformat, extfmt, yPlane, yPitch, uvPlane, uvPitch, nullptr, true, &why)))
        return Fail(hr, why);
    if ((hr = RenderBackBuffer(true)) != MPCVR_S_OK) return hr;
    hr = EncodeSurface(m_BackBuffer.ptr, w * 4, m_cfg.output_format, w, h, outCformat, extfmt, yPlane, yPitch, uvPlane, uvPitch, m_stream, false, &why);
    m_launches++;
    m_lanes.NoteStreamWork();
    return hr ? Fail(hr, why) : MPCVR_S_OK;
}

// ------------------------------------------------------------------------------------------------
// EXTENSION — measuring a rendered frame: the histogram of max(R, G, B) (include/mpcvr.h: mpcvr_measure_pass, mpcvr_measure_backbuffer;
// kernel: vp_measure.hip).  No reference line: the reference's statistics are an overlay.
// ------------------------------------------------------------------------------------------------
// What a k_measure_maxrgb launch is given, but for its pointers: src / hist and the frame stride are the caller's, as in EncodeLaunchParams
static MeasureParams MeasureLaunchParams(int srcPitch, int w, const mpcvr_rect &r)
{
    MeasureParams p{};
    p.src_pitch = srcPitch; p.w = w;
    p.left = r.left; p.top = r.top; p.right = r.right; p.bottom = r.bottom;
    p.src16 = (srcPitch & 15) == 0;
    return p;
}

HRESULT MeasureSurface(const void *src, int srcPitch, int srcFmt, int w, int h, const mpcvr_rect *rect, uint32_t *histDev, hipStream_t stream,
                       bool checkOnly, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    if (!src || !histDev) { *why = "null surface or histogram"; return MPCVR_E_POINTER; }
    if (srcFmt != MPCVR_OUT_BGRA8 && srcFmt != MPCVR_OUT_RGB10A2) { *why = "source BGRA8 or RGB10A2"; return MPCVR_E_INVALIDARG; }
    if (w < 1 || h < 1 || w > 32768 || h > 32768) { *why = "width and height must be 1 .. 32768"; return MPCVR_E_INVALIDARG; }
    if (srcPitch < 4 * w) { *why = "pitch smaller than a row"; return MPCVR_E_INVALIDARG; }
    if (((uintptr_t)src | (uintptr_t)histDev | (uintptr_t)srcPitch) & 3) { *why = "surface, pitch and histogram must be multiples of 4"; return MPCVR_E_INVALIDARG; }
    const mpcvr_rect whole{0, 0, w, h};
    const mpcvr_rect r = rect ? *rect : whole;
    if (r.left < 0 || r.top < 0 || r.right > w || r.bottom > h || r.left >= r.right || r.top >= r.bottom) {
        *why = "the rectangle is empty or leaves the surface"; return MPCVR_E_INVALIDARG;
    }
    const RtSpan s = RowsSpan(src, (size_t)srcPitch, h, (size_t)4 * w), bins{(uintptr_t)histDev, (uintptr_t)histDev + sizeof(uint32_t) * kHistBins};
    if (bins.Overlaps(s)) { *why = "the histogram overlaps the surface"; return MPCVR_E_INVALIDARG; }
    if (checkOnly) return MPCVR_S_OK;
    MeasureParams p = MeasureLaunchParams(srcPitch, w, r);
    p.src = (const uint8_t *)src; p.hist = histDev;
    p.src16 &= (s.lo & 15) == 0;
    if (LaunchMeasure(p, srcFmt == MPCVR_OUT_RGB10A2, stream) != hipSuccess) { *why = "k_measure_maxrgb launch failed"; return MPCVR_E_FAIL; }
    return MPCVR_S_OK;
}

mpcvr_rect CHipVideoProcessor::ActiveRect() const
{
    mpcvr_rect a{std::max(m_videoRect.left, 0), std::max(m_videoRect.top, 0), std::min(m_videoRect.right, m_windowRect.Width()),
                 std::min(m_videoRect.bottom, m_windowRect.Height())};
    if (a.right <= a.left || a.bottom <= a.top) a = mpcvr_rect{0, 0, 0, 0};
    return a;
}

// The pass over the back buffer as the last Render / RenderYuv left it.  It READS memory the frame lanes may still be writing and a later
// Render on a lane may overwrite, and the lanes order writers only — so, as RenderYuv: behind the lanes on the context stream
// (OrderOnContextStream), and everything queued later, lanes included, behind the pass (NoteStreamWork).
HRESULT CHipVideoProcessor::MeasureBackBuffer(uint32_t *histDev)
{
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (!histDev) return Fail(MPCVR_E_POINTER, "null histogram");
    const int w = m_windowRect.Width(), h = m_windowRect.Height();
    // no frame yet, or none of this window's size and format (the back buffer is addressed by the window)
    if (!m_BackBuffer.ptr || m_backW != w || m_backH != h || m_backFmt != m_cfg.output_format || w < 1 || h < 1) return MPCVR_S_FALSE;
    (void)hipSetDevice(m_device);
    const mpcvr_rect r = ActiveRect();
    const bool empty = r.right <= r.left;
    const char *why = "";
    HRESULT hr;
    // (an empty active area: the checks run against the whole window, then only the clear is queued)
    if ((hr = MeasureSurface(m_BackBuffer.ptr, w * 4, m_backFmt, w, h, empty ? nullptr : &r, histDev, nullptr, true, &why))) return Fail(hr, why);
    OrderOnContextStream();
    if (empty) hr = CheckHip(hipMemsetAsync(histDev, 0, sizeof(uint32_t) * kHistBins, m_stream), "clear histogram");
    else {
        hr = MeasureSurface(m_BackBuffer.ptr, w * 4, m_backFmt, w, h, &r, histDev, m_stream, false, &why);
        if (hr) hr = Fail(hr, why); else m_launches++;
    }
    m_lanes.NoteStreamWork();
    return hr;
}

// A batch as NV12 / P010 (include/mpcvr.h: mpcvr_process_batch_yuv).  Everything about the arguments is answered first; then the call is cut
// into chunks of PlanBatchYuv's size, and each chunk is: the batch machinery into frames of a context-owned surface, ONE k_encode420 launch
// with a frame dimension behind it on the same stream.  A chunk whose route may take a batch lane (BatchLaneEligible) takes the next lane in
// turn and that lane's own surface — the lane's stream order covers the surface's write, read and reuse, and the render of the next chunk
// runs beside this one's pass on the other lane; the lanes order the chunk on the bytes it WRITES for the caller, its planes.  Every other
// chunk runs on the context stream into the first surface, behind whatever the lanes hold (OrderOnContextStream), the lanes' next work behind it.
// With histograms (mpcvr_process_batch_yuv_stats): ONE k_measure_maxrgb launch behind the chunk's pass on the same stream, its frame dimension
// over the chunk's frames in the surface (they sit at frameStride: a base, a stride and the chunk's first row are all it needs).  The rows
// are one more span the chunk writes for the caller: the lanes order on them as on the planes.
HRESULT CHipVideoProcessor::ProcessBatchYuv(int n, const void *const *srcs, int outCformat, uint32_t extfmt, void *const *yPlanes, int yPitch,
                                            void *const *uvPlanes, int uvPitch, uint32_t *histDev)
{
    const BatchRecord record(*this, n > 0 ? n : 0);
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (n <= 0) return Fail(MPCVR_E_INVALIDARG, "empty batch");
    if (!srcs || !yPlanes || !uvPlanes) return Fail(MPCVR_E_POINTER, "null array of frames or planes");
    for (int i = 0; i < n; i++)
        if (!srcs[i] || !yPlanes[i] || !uvPlanes[i]) return Fail(MPCVR_E_POINTER, "null frame or plane in batch");
    if ((uintptr_t)histDev & 3) return Fail(MPCVR_E_INVALIDARG, "the histogram must be 4-byte aligned");
    const int w = m_windowRect.Width(), h = m_windowRect.Height();
    BatchYuvLayout lay;
    if (!PlanBatchYuv(w, h, n, m_yuvBudget, &lay)) return Fail(MPCVR_E_INVALIDARG, "a 4:2:0 frame needs an even window width and height, 2 .. 32768");
    // what the pass refuses, per frame (the surface is still to be allocated: it cannot overlap a plane) ...
    const char *why = "";
    for (int i = 0; i < n; i++)
        if (HRESULT bad = EncodeSurface(nullptr, lay.surfacePitch, m_cfg.output_format, w, h, outCformat, extfmt, yPlanes[i], yPitch, uvPlanes[i], uvPitch, nullptr, true, &why))
            return Fail(bad, why);
    EncodePlan plan;
    if (!PlanEncode(outCformat, m_cfg.output_format, extfmt, w, h, &plan)) return Fail(MPCVR_E_INVALIDARG, "output NV12 or P010 with a YCbCr description");
    // ... and the 2n planes against each other: a plane counts as the bytes from its first pixel to the last pixel of its last row
    const size_t rowBytes = plan.out10 ? (size_t)2 * w : (size_t)w;
    const std::vector<RtSpan> planes = BatchPlaneSpans(n, yPlanes, yPitch, uvPlanes, uvPitch, h, rowBytes);
    if (AnyTwoSpansOverlap(planes)) return Fail(MPCVR_E_INVALIDARG, "two planes of the batch overlap");
    constexpr size_t kHistRow = sizeof(uint32_t) * kHistBins;
    if (histDev) {
        const RtSpan rows{(uintptr_t)histDev, (uintptr_t)histDev + kHistRow * (size_t)n};
        for (const RtSpan &pl : planes)
            if (pl.Overlaps(rows)) return Fail(MPCVR_E_INVALIDARG, "the histogram rows overlap a plane of the batch");
    }

    (void)hipSetDevice(m_device);
    HRESULT hr = MPCVR_S_OK;
    if (m_planDirty && (hr = UpdatePlan())) return hr;
    const EncodeParams ep = EncodeLaunchParams(plan, w, h, lay.surfacePitch, yPitch, uvPitch);      // (src16 holds for every chunk: every frame of a surface starts on 256 bytes)
    return RunSurfaceChunks(n, srcs, lay, "yuv",
        [&](int at, int m) {
            std::vector<RtSpan> writes(planes.begin() + 2 * (size_t)at, planes.begin() + 2 * (size_t)(at + m));
            if (histDev) writes.push_back(RtSpan{(uintptr_t)histDev + kHistRow * (size_t)at, (uintptr_t)histDev + kHistRow * (size_t)(at + m)});
            return writes;
        },
        [&](BatchRun &run, int at) { return EncodeChunk(run, ep, plan, yPlanes + at, uvPlanes + at, histDev ? histDev + (size_t)kHistBins * (size_t)at : nullptr); });
}

// The chunk loop of the batch calls that render into a context-owned surface and run one pass per chunk behind it (ProcessBatchYuv,
// ProcessBatchTensor): writesOf(at, m) names the bytes the chunk of frames [at, at + m) writes for the caller, pass(run, at) queues the
// chunk's pass on run.on.stream (run.dsts: the chunk's frames in the surface).  `tag` names the call in GetLastBatchInfo.
template <class WritesOf, class Pass>
HRESULT CHipVideoProcessor::RunSurfaceChunks(int n, const void *const *srcs, const BatchYuvLayout &lay, const char *tag, WritesOf writesOf, Pass pass)
{
    HRESULT hr = MPCVR_S_OK;
    const int most = lay.framesPerChunk;
    std::vector<void *> frames((size_t)most);
    auto surfaceFrames = [&](YuvSurface &s) -> HRESULT {       // the surface for `most` frames, and their addresses
        const size_t had = s.buf.ptr ? s.buf.size : 0;
        if (HRESULT bad = CheckHip(s.buf.CheckCreate(lay.frameStride * (size_t)most), "batch RGB surface")) return bad;
        if (s.buf.size != had) s.cleared = false;
        for (int i = 0; i < most; i++) frames[i] = (uint8_t *)s.buf.ptr + (size_t)i * lay.frameStride;
        return MPCVR_S_OK;
    };
    std::string lanes;
    int chunks = 0;
    for (int at = 0; at < n && !hr; at += most, chunks++) {
        const int m = std::min(most, n - at);
        BatchRun run{m, srcs + at, frames.data(), lay.surfacePitch};
        YuvSurface *surf = &m_yuvSurf[0];
        if ((hr = surfaceFrames(*surf))) break;
        BatchRoutePlan rp = m_plan.errdiff ? BatchRoutePlan{} : ClassifyBatch(run);     // (an error-diffusion plan classifies its own chunks: the default is no lane route)
        const int bl = PlaceBatch(rp, run, writesOf(at, m));
        if (bl > 0) {                                   // another lane, another surface: the route is planned for the targets it draws into
            surf = &m_yuvSurf[bl];
            if ((hr = surfaceFrames(*surf))) break;
            rp = ClassifyBatch(run);
        }
        if (chunks < 64) lanes += (chunks ? "," : "") + std::to_string(bl);
        if (!(hr = RenderChunk(rp, run, *surf))) hr = pass(run, at);
        NoteBatchQueued(bl);
    }
    m_yuvLastInfo = std::string(";") + tag + "_chunks=" + std::to_string(chunks) + ";" + tag + "_lanes=" + lanes;
    return hr;
}

// Its mirror, the chunk loop of the batch calls that draw from the context-owned sample surface (ProcessBatchFromTensors, ProcessBatchDeint):
// pass(at, m, samples, stream) queues the pass that writes samples[0 .. m) for output frames [at, at + m), the batch machinery draws them into
// dsts + at behind it.  Both on the context stream: stream order covers the surface's write, read and reuse by the next chunk.
template <class Pass>
HRESULT CHipVideoProcessor::RunSampleChunks(int n, const ChunkLayout &lay, void *const *dsts, int rtPitch, const char *tag, Pass pass)
{
    const int most = lay.framesPerChunk;
    HRESULT hr;
    if ((hr = CheckHip(m_sampleSurf.CheckCreate(lay.frameStride * (size_t)most), "batch sample surface"))) return hr;
    std::vector<const void *> samples((size_t)most);
    for (int i = 0; i < most; i++) samples[i] = (const uint8_t *)m_sampleSurf.ptr + (size_t)i * lay.frameStride;
    int chunks = 0;
    for (int at = 0; at < n && !hr; at += most, chunks++) {
        const int m = std::min(most, n - at);
        BatchRun run{m, samples.data(), dsts + at, rtPitch};
        run.on = RunOn{m_stream};
        OrderOnContextStream();          // behind every frame and batch the lanes hold (the last chunk's readers of the surface are on this stream already)
        if ((hr = pass(at, m, samples.data(), m_stream))) break;
        BatchRoutePlan rp = m_plan.errdiff ? BatchRoutePlan{} : ClassifyBatch(run);     // (an error-diffusion plan classifies its own chunks)
        hr = m_plan.errdiff ? ProcessBatchErrDiff(run) : RunBatchRoute(rp, run);
    }
    m_yuvLastInfo = std::string(";") + tag + "_chunks=" + std::to_string(chunks);
    return hr;
}

// the chunk's frames into the surface: the batch machinery on run.on.stream
HRESULT CHipVideoProcessor::RenderChunk(BatchRoutePlan &rp, BatchRun &run, YuvSurface &surf)
{
    hipStream_t const stream = run.on.stream;
    // Process never writes the letterbox: black once per allocation and per window / video rect, in front of the first chunk that draws there
    if (!surf.cleared || surf.window != m_windowRect || surf.video != m_videoRect) {
        if (HRESULT hr = CheckHip(hipMemsetAsync(surf.buf.ptr, 0, surf.buf.size, stream), "clear batch RGB surface")) return hr;
        surf.cleared = true; surf.window = m_windowRect; surf.video = m_videoRect;
    }
    // (the error-diffusion plan runs its own chunks and its pass on the context stream: `run` is on it, BatchLaneEligible refuses such a plan)
    return m_plan.errdiff ? ProcessBatchErrDiff(run) : RunBatchRoute(rp, run);
}

HRESULT CHipVideoProcessor::EncodeChunk(BatchRun &run, const EncodeParams &encode, const EncodePlan &plan, void *const *yPlanes, void *const *uvPlanes,
                                        uint32_t *histRows)
{
    hipStream_t const stream = run.on.stream;
    HRESULT hr;
    // the planes' table through the frame tables' ring; the lease ends behind the pass
    SlotLease table;
    EncodeParams ep = encode;
    if ((hr = m_tableRing.SendRows<EncodeFrame>(run.n, stream, "plane table", &table, [&](EncodeFrame *fr) {
            for (int i = 0; i < run.n; i++) {
                fr[i] = EncodeFrame{(const uint8_t *)run.dsts[i], (uint8_t *)yPlanes[i], (uint8_t *)uvPlanes[i]};
                ep.dst8 &= (((uintptr_t)yPlanes[i] | (uintptr_t)uvPlanes[i]) & 7) == 0;       // the 8-byte stores only if every plane of the launch allows them
            }
        }))) return hr;
    ep.frames = (const EncodeFrame *)table.dev;
    if ((hr = CheckHip(LaunchEncode420(ep, plan.in10, plan.out10, plan.siting, stream, run.n), "k_encode420")) || !histRows) return hr;
    // the chunk's histograms: the frames of the surface are run.dsts[0] + i * frame stride (RunSurfaceChunks lays them out so: on 256 bytes)
    MeasureParams mp = MeasureLaunchParams(encode.src_pitch, encode.w, ActiveRect());
    mp.src = (const uint8_t *)run.dsts[0]; mp.hist = histRows;
    mp.frame_stride = run.n > 1 ? (size_t)((const uint8_t *)run.dsts[1] - (const uint8_t *)run.dsts[0]) : 0;
    int launched = 0;
    const hipError_t e = LaunchMeasure(mp, plan.in10, stream, run.n, &launched);
    // (counted as the kernel launches it was: none for an empty active area, whose rows are only cleared)
    return launched ? CheckHip(e, "k_measure_maxrgb") : CheckHip(e, "clear histogram rows");
}

// ------------------------------------------------------------------------------------------------
// EXTENSION — the frame as the float tensor a model takes (include/mpcvr.h: mpcvr_tensor_pass, mpcvr_render_tensor,
// mpcvr_process_batch_tensor; kernel: vp_tensor.hip).  No reference line: the reference has no float output.
// ------------------------------------------------------------------------------------------------
// the planes of one tensor (first element to last element of the last row): three for C,H,W, the whole tensor for H,W,C; returns how many
static int TensorPlaneSpans(const mpcvr_tensor_desc &d, const void *dst, int w, int h, RtSpan out[3])
{
    const size_t es = (size_t)TensorElementSize(d.dtype);
    if (d.layout == TN_INTERLEAVED) { out[0] = RowsSpan(dst, (size_t)d.row_pitch, h, 3 * es * (size_t)w); return 1; }
    for (int k = 0; k < 3; k++) out[k] = RowsSpan((const uint8_t *)dst + (size_t)k * (size_t)d.plane_pitch, (size_t)d.row_pitch, h, es * (size_t)w);
    return 3;
}

// what TensorSurface and SampleSurface ask of a description and of the tensor at `base` it describes (w: the elements of a row, per channel)
static HRESULT CheckTensorDesc(const mpcvr_tensor_desc &d, const void *base, int w, const char **why)
{
    if (d.dtype < TN_F32 || d.dtype > TN_BF16 || (d.layout != TN_PLANAR && d.layout != TN_INTERLEAVED) ||
        (d.channel_order != MPCVR_TENSOR_RGB && d.channel_order != MPCVR_TENSOR_BGR) || d.reserved != 0) {
        *why = "unknown dtype, layout or channel order, or reserved is not 0"; return MPCVR_E_INVALIDARG;
    }
    for (int k = 0; k < 3; k++)
        if (!TensorFactorOk(d.scale[k]) || !TensorFactorOk(d.bias[k])) { *why = "scale and bias must be finite, and 0 or of magnitude 2^-100 .. 2^100"; return MPCVR_E_INVALIDARG; }
    const bool planar = d.layout == TN_PLANAR;
    const int64_t es = TensorElementSize(d.dtype), kMaxPitch = (int64_t)1 << 47;      // (h rows and three planes of that stay far inside 64 bits)
    if (d.row_pitch < es * (planar ? 1 : 3) * w || d.row_pitch > kMaxPitch || (planar && (d.plane_pitch < 1 || d.plane_pitch > kMaxPitch))) {
        *why = "row pitch smaller than a row, or a pitch that is not positive or beyond 2^47"; return MPCVR_E_INVALIDARG;
    }
    if (((uintptr_t)base | (uintptr_t)d.row_pitch | (planar ? (uintptr_t)d.plane_pitch : 0)) & (uintptr_t)(es - 1)) {
        *why = "tensor and pitches must be multiples of the element size"; return MPCVR_E_INVALIDARG;
    }
    return MPCVR_S_OK;
}

// What a k_tensor launch is given, but for its pointers: src / dst or the frame table are the caller's, who takes src16 / dstvec back where
// a pointer of the launch is off the grid (here they say what the pitches allow), as in EncodeLaunchParams
static TensorParams TensorLaunchParams(const mpcvr_tensor_desc &d, int w, int h, int srcPitch)
{
    TensorParams p{};
    p.src_pitch = srcPitch; p.w = w; p.h = h;
    p.row_pitch = d.row_pitch; p.plane_pitch = d.layout == TN_PLANAR ? d.plane_pitch : 0;
    std::memcpy(p.scale, d.scale, sizeof(p.scale));
    std::memcpy(p.bias, d.bias, sizeof(p.bias));
    p.bgr = d.channel_order == MPCVR_TENSOR_BGR;
    p.src16 = (srcPitch & 15) == 0;
    p.dstvec = ((p.row_pitch | p.plane_pitch) & (TensorVectorBytes(d.dtype) - 1)) == 0;
    return p;
}

HRESULT TensorSurface(const void *src, int srcPitch, int srcFmt, int w, int h, const mpcvr_tensor_desc *desc, void *dst, hipStream_t stream,
                      bool checkOnly, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    if ((!src && !checkOnly) || !desc || !dst) { *why = "null surface, description or tensor"; return MPCVR_E_POINTER; }      // (checkOnly: a source still to be allocated)
    if (srcFmt != MPCVR_OUT_BGRA8 && srcFmt != MPCVR_OUT_RGB10A2) { *why = "source BGRA8 or RGB10A2"; return MPCVR_E_INVALIDARG; }
    if (w < 1 || h < 1 || w > 32768 || h > 32768) { *why = "width and height must be 1 .. 32768"; return MPCVR_E_INVALIDARG; }
    if (srcPitch < 4 * w) { *why = "pitch smaller than a row"; return MPCVR_E_INVALIDARG; }
    if (((uintptr_t)src | (uintptr_t)srcPitch) & 3) { *why = "surface and pitch must be multiples of 4"; return MPCVR_E_INVALIDARG; }
    const mpcvr_tensor_desc &d = *desc;
    if (HRESULT bad = CheckTensorDesc(d, dst, w, why)) return bad;
    const RtSpan s = RowsSpan(src, (size_t)srcPitch, h, (size_t)4 * w);
    RtSpan pl[3];
    const int np = TensorPlaneSpans(d, dst, w, h, pl);
    for (int a = 0; a < np; a++) {
        if (src && pl[a].Overlaps(s)) { *why = "a plane overlaps the source"; return MPCVR_E_INVALIDARG; }
        for (int b = a + 1; b < np; b++)
            if (pl[a].Overlaps(pl[b])) { *why = "two planes of the tensor overlap"; return MPCVR_E_INVALIDARG; }
    }
    if (checkOnly) return MPCVR_S_OK;
    TensorParams p = TensorLaunchParams(d, w, h, srcPitch);
    p.src = (const uint8_t *)src; p.dst = (uint8_t *)dst;
    p.src16 &= (s.lo & 15) == 0;
    p.dstvec &= ((uintptr_t)dst & (uintptr_t)(TensorVectorBytes(d.dtype) - 1)) == 0;
    if (LaunchTensor(p, srcFmt == MPCVR_OUT_RGB10A2, d.dtype, d.layout, stream) != hipSuccess) { *why = "k_tensor launch failed"; return MPCVR_E_FAIL; }
    return MPCVR_S_OK;
}

// Render, then the pass over the whole window behind it, ordered as RenderYuv (the comment there): on the context stream, the lanes' next
// work behind the pass.
HRESULT CHipVideoProcessor::RenderTensor(int /*field*/, const mpcvr_tensor_desc &desc, void *dst)
{
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    (void)hipSetDevice(m_device);
    const int w = m_windowRect.Width(), h = m_windowRect.Height();
    // everything about the tensor is answered before anything is drawn (a back buffer Render has yet to allocate cannot overlap it)
    const bool have = m_BackBuffer.ptr && m_BackBuffer.size >= (size_t)w * 4 * h;
    HRESULT hr;
    const char *why = "";
    if ((hr = TensorSurface(have ? m_BackBuffer.ptr : nullptr, w * 4, m_cfg.output_format, w, h, &desc, dst, nullptr, true, &why))) return Fail(hr, why);
    if (!m_curSample) return MPCVR_S_FALSE;          // nothing to draw, as Render
    if ((hr = RenderBackBuffer(true)) != MPCVR_S_OK) return hr;
    hr = TensorSurface(m_BackBuffer.ptr, w * 4, m_cfg.output_format, w, h, &desc, dst, m_stream, false, &why);
    m_launches++;
    m_lanes.NoteStreamWork();
    return hr ? Fail(hr, why) : MPCVR_S_OK;
}

// A batch as tensors (include/mpcvr.h: mpcvr_process_batch_tensor): ProcessBatchYuv with k_tensor as the chunk's pass.  Everything about
// the arguments is answered first; the chunks, their surfaces, lanes and order are RunSurfaceChunks'.  Every plane of every frame is a
// span the chunk writes.
HRESULT CHipVideoProcessor::ProcessBatchTensor(int n, const void *const *srcs, const mpcvr_tensor_desc *desc, void *const *dsts)
{
    const BatchRecord record(*this, n > 0 ? n : 0);
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (n <= 0) return Fail(MPCVR_E_INVALIDARG, "empty batch");
    if (!srcs || !dsts || !desc) return Fail(MPCVR_E_POINTER, "null array of frames or tensors, or null description");
    for (int i = 0; i < n; i++)
        if (!srcs[i] || !dsts[i]) return Fail(MPCVR_E_POINTER, "null frame or tensor in batch");
    const int w = m_windowRect.Width(), h = m_windowRect.Height();
    BatchYuvLayout lay;
    if (!PlanBatchTensor(w, h, n, m_yuvBudget, &lay)) return Fail(MPCVR_E_INVALIDARG, "a tensor needs a window width and height of 1 .. 32768");
    // what the pass refuses, per frame (the surface is still to be allocated: it cannot overlap a plane) ...
    const char *why = "";
    for (int i = 0; i < n; i++)
        if (HRESULT bad = TensorSurface(nullptr, lay.surfacePitch, m_cfg.output_format, w, h, desc, dsts[i], nullptr, true, &why)) return Fail(bad, why);
    // ... and the planes of all frames against each other
    const int np = desc->layout == TN_PLANAR ? 3 : 1;
    std::vector<RtSpan> planes((size_t)np * (size_t)n);
    for (int i = 0; i < n; i++) TensorPlaneSpans(*desc, dsts[i], w, h, &planes[(size_t)np * (size_t)i]);
    if (AnyTwoSpansOverlap(planes)) return Fail(MPCVR_E_INVALIDARG, "two planes of the batch overlap");

    (void)hipSetDevice(m_device);
    if (HRESULT bad = m_planDirty ? UpdatePlan() : MPCVR_S_OK) return bad;
    const TensorParams tp = TensorLaunchParams(*desc, w, h, lay.surfacePitch);      // (src16 holds for every chunk: every frame of a surface starts on 256 bytes)
    const bool in10 = m_cfg.output_format == MPCVR_OUT_RGB10A2;
    return RunSurfaceChunks(n, srcs, lay, "tensor",
        [&](int at, int m) { return std::vector<RtSpan>(planes.begin() + (size_t)np * (size_t)at, planes.begin() + (size_t)np * (size_t)(at + m)); },
        [&](BatchRun &run, int at) {
            // the tensors' table through the frame tables' ring; the lease ends behind the pass
            SlotLease table;
            TensorParams p = tp;
            if (HRESULT bad = m_tableRing.SendRows<TensorFrame>(run.n, run.on.stream, "tensor table", &table, [&](TensorFrame *fr) {
                    for (int i = 0; i < run.n; i++) {
                        fr[i] = TensorFrame{(const uint8_t *)run.dsts[i], (uint8_t *)dsts[at + i]};
                        p.dstvec &= ((uintptr_t)dsts[at + i] & (uintptr_t)(TensorVectorBytes(desc->dtype) - 1)) == 0;      // the vector stores only if every tensor of the launch allows them
                    }
                })) return bad;
            p.frames = (const TensorFrame *)table.dev;
            return CheckHip(LaunchTensor(p, in10, desc->dtype, desc->layout, run.on.stream, run.n), "k_tensor");
        });
}

// ------------------------------------------------------------------------------------------------
// EXTENSION — the way back: the float tensor a model leaves as a planar RGB sample (include/mpcvr.h: mpcvr_sample_pass,
// mpcvr_copy_sample_tensor, mpcvr_process_batch_from_tensors; kernel: vp_tensor_in.hip).  No reference line: the reference has no float input.
// ------------------------------------------------------------------------------------------------
// What a k_sample_from_tensor launch is given, but for its pointers: src / dst or the frame table are the caller's, who takes srcvec / dstvec
// back where a pointer of the launch is off the grid (here they say what the pitches allow), as in TensorLaunchParams
static SampleParams SampleLaunchParams(const mpcvr_tensor_desc &d, int w, int h, int bytes, int maxcode, int pitch)
{
    SampleParams p{};
    p.w = w; p.h = h;
    p.row_pitch = d.row_pitch; p.plane_pitch = d.layout == TN_PLANAR ? d.plane_pitch : 0;
    p.dst_pitch = pitch; p.dst_plane = (int64_t)pitch * h;
    std::memcpy(p.scale, d.scale, sizeof(p.scale));
    std::memcpy(p.bias, d.bias, sizeof(p.bias));
    p.maxcode = (float)maxcode;
    p.bgr = d.channel_order == MPCVR_TENSOR_BGR;
    p.srcvec = ((p.row_pitch | p.plane_pitch) & (TensorVectorBytes(d.dtype) - 1)) == 0;
    p.dstvec = (pitch & (4 * bytes - 1)) == 0;
    return p;
}

HRESULT SampleSurface(const void *tensor, const mpcvr_tensor_desc *desc, int w, int h, int cformat, void *sample, int pitch, hipStream_t stream,
                      bool checkOnly, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    if (!tensor || !desc || (!sample && !checkOnly)) { *why = "null tensor, description or sample"; return MPCVR_E_POINTER; }      // (checkOnly: a sample still to be allocated)
    int bytes, maxcode;
    if (!SampleFormat(cformat, &bytes, &maxcode)) { *why = "sample GBRP8, GBRP10 or GBRP16"; return MPCVR_E_INVALIDARG; }
    if (w < 1 || h < 1 || w > 32768 || h > 32768) { *why = "width and height must be 1 .. 32768"; return MPCVR_E_INVALIDARG; }
    const mpcvr_tensor_desc &d = *desc;
    if (HRESULT bad = CheckTensorDesc(d, tensor, w, why)) return bad;
    if (pitch < w * bytes || (pitch & (bytes - 1)) || ((uintptr_t)sample & (uintptr_t)(bytes - 1))) {
        *why = "sample pitch smaller than a row, or sample or pitch no multiple of the component size"; return MPCVR_E_INVALIDARG;
    }
    // the tensor is only read: its planes may share bytes with each other, not with a plane of the sample
    RtSpan tp[3], sp[3];
    const int np = TensorPlaneSpans(d, tensor, w, h, tp);
    for (int k = 0; k < 3; k++) sp[k] = RowsSpan((const uint8_t *)sample + (size_t)k * (size_t)pitch * (size_t)h, (size_t)pitch, h, (size_t)w * bytes);
    if (sample) {
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < np; b++)
                if (sp[a].Overlaps(tp[b])) { *why = "a plane of the tensor overlaps a plane of the sample"; return MPCVR_E_INVALIDARG; }
            for (int b = a + 1; b < 3; b++)      // (cannot happen while pitch >= a row and the planes lie pitch * h apart: checked, not assumed)
                if (sp[a].Overlaps(sp[b])) { *why = "two planes of the sample overlap"; return MPCVR_E_INVALIDARG; }
        }
    }
    if (checkOnly) return MPCVR_S_OK;
    SampleParams p = SampleLaunchParams(d, w, h, bytes, maxcode, pitch);
    p.src = (const uint8_t *)tensor; p.dst = (uint8_t *)sample;
    p.srcvec &= ((uintptr_t)tensor & (uintptr_t)(TensorVectorBytes(d.dtype) - 1)) == 0;
    p.dstvec &= ((uintptr_t)sample & (uintptr_t)(4 * bytes - 1)) == 0;
    if (LaunchSampleFromTensor(p, d.dtype, d.layout, bytes, stream) != hipSuccess) { *why = "k_sample_from_tensor launch failed"; return MPCVR_E_FAIL; }
    return MPCVR_S_OK;
}

// CopySample(MPCVR_MEM_HOST) with the pass in place of the host-to-device copy: the same slot ring, device buffers and events.  The pass is
// queued on the context stream (the caller's tensor is free in stream order behind the call); `uploaded` is recorded behind it there, so a
// frame lane waits for the pass exactly as it waits for an upload (ProcessFrame).
HRESULT CHipVideoProcessor::CopySampleTensor(const void *tensor, const mpcvr_tensor_desc *desc)
{
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (!tensor || !desc) return Fail(MPCVR_E_POINTER, "null tensor or description");
    // (every refusal comes before anything is touched: the current sample, its upload slot and the stream it was last drawn on stay as they are)
    const char *why = "";
    if (HRESULT bad = SampleSurface(tensor, desc, m_srcWidth, m_srcHeight, m_srcParams->cformat, nullptr, m_srcPitch, nullptr, true, &why)) return Fail(bad, why);
    (void)hipSetDevice(m_device);
    HRESULT hr;
    MarkConsumed();                                  // the previous sample is done with as far as the host is concerned
    m_curSlot = -1;
    m_lastRun = nullptr;
    m_curSample = nullptr;                           // (a failure below leaves no sample rather than a slot half written)
    int si;
    if ((hr = AcquireUploadSlot((size_t)m_srcPitch * m_srcLines, &si))) return hr;
    if ((hr = SampleSurface(tensor, desc, m_srcWidth, m_srcHeight, m_srcParams->cformat, m_up[si].dev.ptr, m_srcPitch, m_stream, false, &why))) return Fail(hr, why);
    m_launches++;
    m_lanes.NoteStreamWork();
    return PublishUploadSlot(si, m_stream);
}

// A batch from tensors (include/mpcvr.h: mpcvr_process_batch_from_tensors).  Everything about the arguments is answered first; then the
// call is cut into chunks of PlanBatchSamples' size, and each chunk is ONE k_sample_from_tensor launch with a frame dimension into the
// context-owned sample surface and the batch machinery behind it (RunSampleChunks).
HRESULT CHipVideoProcessor::ProcessBatchFromTensors(int n, const void *const *tensors, const mpcvr_tensor_desc *desc, void *const *dsts, int rtPitch)
{
    const BatchRecord record(*this, n > 0 ? n : 0);
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (n <= 0) return Fail(MPCVR_E_INVALIDARG, "empty batch");
    if (!tensors || !dsts || !desc) return Fail(MPCVR_E_POINTER, "null array of tensors or frames, or null description");
    for (int i = 0; i < n; i++)
        if (!tensors[i] || !dsts[i]) return Fail(MPCVR_E_POINTER, "null tensor or frame in batch");
    int bytes, maxcode;
    if (!SampleFormat(m_srcParams->cformat, &bytes, &maxcode)) return Fail(MPCVR_E_INVALIDARG, "the input must be GBRP8, GBRP10 or GBRP16");
    if (HRESULT bad = CheckBatchArgs(n, tensors, dsts, rtPitch)) return bad;
    const int w = m_srcWidth, h = m_srcHeight;
    const char *why = "";
    for (int i = 0; i < n; i++)
        if (HRESULT bad = SampleSurface(tensors[i], desc, w, h, m_srcParams->cformat, nullptr, m_srcPitch, nullptr, true, &why)) return Fail(bad, why);
    ChunkLayout lay;
    if (!PlanBatchSamples(m_srcPitch, h, n, m_yuvBudget, &lay)) return Fail(MPCVR_E_INVALIDARG, "sample layout");

    (void)hipSetDevice(m_device);
    if (HRESULT bad = m_planDirty ? UpdatePlan() : MPCVR_S_OK) return bad;
    // (dstvec holds for every chunk: every frame of the surface starts on 256 bytes)
    const SampleParams sp = SampleLaunchParams(*desc, w, h, bytes, maxcode, m_srcPitch);
    return RunSampleChunks(n, lay, dsts, rtPitch, "sample", [&](int at, int m, const void *const *samples, hipStream_t stream) {
        // the tensors' table through the frame tables' ring; the lease ends behind the pass
        SlotLease table;
        SampleParams p = sp;
        if (HRESULT bad = m_tableRing.SendRows<SampleFrame>(m, stream, "sample table", &table, [&](SampleFrame *fr) {
                for (int i = 0; i < m; i++) {
                    fr[i] = SampleFrame{(const uint8_t *)tensors[at + i], (uint8_t *)const_cast<void *>(samples[i])};
                    p.srcvec &= ((uintptr_t)tensors[at + i] & (uintptr_t)(TensorVectorBytes(desc->dtype) - 1)) == 0;      // the vector loads only if every tensor of the launch allows them
                }
            })) return bad;
        p.frames = (const SampleFrame *)table.dev;
        return CheckHip(LaunchSampleFromTensor(p, desc->dtype, desc->layout, bytes, stream, m), "k_sample_from_tensor");
    });
}

// ------------------------------------------------------------------------------------------------
// EXTENSION — motion-adaptive deinterlacing at field rate (include/mpcvr.h: mpcvr_deint_pass, mpcvr_copy_sample_fields,
// mpcvr_process_batch_deint; kernel: vp_deint.hip).  No reference line: the reference hands deinterlacing to the fixed-function video processor.
// ------------------------------------------------------------------------------------------------
// What the k_deint launches of one sample are given, but for their pointers: one DeintParams per distinct (bytes, cs) among the planes (cs[g]
// says which), srcvec / dstvec as far as plane offsets and pitches decide them — the caller takes them back where a pointer is off the grid
static int DeintGroupParams(const DeintPlane *sp, const DeintPlane *dp, int np, DeintParams out[2], int cs[2])
{
    int n = 0;
    for (int want = 1; want <= 2; want++) {
        DeintParams p{};
        p.srcvec = p.dstvec = 1;
        for (int i = 0; i < np; i++) {
            if (sp[i].cs != want) continue;
            const size_t grid = (size_t)(kDeintLaneSteps * want * sp[i].bytes) - 1;
            p.plane[p.n_planes++] = DeintLaunchPlane{(int64_t)sp[i].offset, (int64_t)dp[i].offset, sp[i].pitch, dp[i].pitch, sp[i].comps / want, sp[i].lines};
            p.srcvec &= ((sp[i].offset | (size_t)sp[i].pitch) & grid) == 0;
            p.dstvec &= ((dp[i].offset | (size_t)dp[i].pitch) & grid) == 0;
            p.mask = sp[i].mask;
        }
        if (p.n_planes) { out[n] = p; cs[n++] = want; }
    }
    return n;
}

HRESULT DeintSurface(const void *prev, const void *cur, const void *next, int cformat, int w, int h, int pitch, int keep, int first, int mode,
                     void *dst, int dstPitch, hipStream_t stream, bool checkOnly, const char **why, int *launches)
{
    const char *dummy;
    if (!why) why = &dummy;
    if (launches) *launches = 0;
    if (!prev || !cur || !next || (!dst && !checkOnly)) { *why = "null sample"; return MPCVR_E_POINTER; }      // (checkOnly: a destination still to be allocated)
    DeintPlane sp[kDeintMaxPlanes], dp[kDeintMaxPlanes];
    int np = 0, npd = 0;
    if (!PlanDeintPlanes(cformat, w, h, pitch, &np, sp) || !PlanDeintPlanes(cformat, w, h, dstPitch, &npd, dp)) {
        *why = "a planar or bi-planar format, a size and pitches by the rules of mpcvr_set_input, at least 2 lines per plane"; return MPCVR_E_INVALIDARG;
    }
    if ((keep != 0 && keep != 1) || (first != 0 && first != 1) || (mode != DI_ADAPTIVE && mode != DI_ADAPTIVE_NOCHECK)) {
        *why = "keep and first are 0 or 1, mode MPCVR_DEINT_ADAPTIVE_EXT or MPCVR_DEINT_ADAPTIVE_NOCHECK_EXT"; return MPCVR_E_INVALIDARG;
    }
    const int bytes = sp[0].bytes;
    if (((uintptr_t)prev | (uintptr_t)cur | (uintptr_t)next | (uintptr_t)dst) & (uintptr_t)(bytes - 1)) {
        *why = "samples must be multiples of the component size"; return MPCVR_E_INVALIDARG;
    }
    // the sources are only read: they may share bytes with each other, not with a plane of the destination
    if (dst) {
        const void *const srcs[3] = {prev, cur, next};
        for (int a = 0; a < np; a++) {
            const RtSpan d = RowsSpan((const uint8_t *)dst + dp[a].offset, (size_t)dp[a].pitch, dp[a].lines, (size_t)dp[a].comps * bytes);
            for (int s = 0; s < 3; s++)
                for (int b = 0; b < np; b++)
                    if (d.Overlaps(RowsSpan((const uint8_t *)srcs[s] + sp[b].offset, (size_t)sp[b].pitch, sp[b].lines, (size_t)sp[b].comps * bytes))) {
                        *why = "a plane of the destination overlaps a plane of a source"; return MPCVR_E_INVALIDARG;
                    }
            for (int b = a + 1; b < np; b++)
                if (d.Overlaps(RowsSpan((const uint8_t *)dst + dp[b].offset, (size_t)dp[b].pitch, dp[b].lines, (size_t)dp[b].comps * bytes))) {
                    *why = "two planes of the destination overlap"; return MPCVR_E_INVALIDARG;
                }
        }
    }
    if (checkOnly) return MPCVR_S_OK;
    DeintParams g[2];
    int cs[2];
    const int ng = DeintGroupParams(sp, dp, np, g, cs);
    for (int i = 0; i < ng; i++) {
        DeintParams &p = g[i];
        const uintptr_t grid = (uintptr_t)(kDeintLaneSteps * cs[i] * bytes) - 1;
        p.one = DeintFrame{(const uint8_t *)prev, (const uint8_t *)cur, (const uint8_t *)next, (uint8_t *)dst, keep, first};
        p.srcvec &= (((uintptr_t)prev | (uintptr_t)cur | (uintptr_t)next) & grid) == 0;
        p.dstvec &= ((uintptr_t)dst & grid) == 0;
        if (LaunchDeint(p, bytes, cs[i], mode, stream) != hipSuccess) { *why = "k_deint launch failed"; return MPCVR_E_FAIL; }
        if (launches) ++*launches;
    }
    return MPCVR_S_OK;
}

// keep and first of field `field` (0 the first, 1 the second) of a frame of `fieldOrder` (1 top field first, 2 bottom field first)
static void FieldParity(int fieldOrder, int field, int *keep, int *first)
{
    *first = field == 0;
    *keep = fieldOrder == 1 ? field : 1 - field;
}

// CopySampleTensor with k_deint as the pass: the same slot ring, device buffers and events, on the context stream.
HRESULT CHipVideoProcessor::CopySampleFields(const void *prev, const void *cur, const void *next, int fieldOrder, int field, int mode)
{
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (!prev || !cur || !next) return Fail(MPCVR_E_POINTER, "null sample");
    if ((fieldOrder != 1 && fieldOrder != 2) || (field != 0 && field != 1)) return Fail(MPCVR_E_INVALIDARG, "field_order is 1 or 2, field 0 or 1");
    int keep, first;
    FieldParity(fieldOrder, field, &keep, &first);
    // (every refusal comes before anything is touched: the current sample, its upload slot and the stream it was last drawn on stay as they are)
    const char *why = "";
    const int cf = m_srcParams->cformat;
    if (HRESULT bad = DeintSurface(prev, cur, next, cf, m_srcWidth, m_srcHeight, m_srcPitch, keep, first, mode, nullptr, m_srcPitch, nullptr, true, &why)) return Fail(bad, why);
    (void)hipSetDevice(m_device);
    HRESULT hr;
    MarkConsumed();                                  // the previous sample is done with as far as the host is concerned
    m_curSlot = -1;
    m_lastRun = nullptr;
    m_curSample = nullptr;                           // (a failure below leaves no sample rather than a slot half written)
    int si, launched = 0;
    if ((hr = AcquireUploadSlot((size_t)m_srcPitch * m_srcLines, &si))) return hr;
    // (the slot's buffer may be one a caller was handed as a sample address long ago: the overlap rule is asked again with the real destination)
    if ((hr = DeintSurface(prev, cur, next, cf, m_srcWidth, m_srcHeight, m_srcPitch, keep, first, mode, m_up[si].dev.ptr, m_srcPitch, m_stream, false, &why, &launched))) return Fail(hr, why);
    m_launches += launched;
    m_lanes.NoteStreamWork();
    return PublishUploadSlot(si, m_stream);
}

// A batch at field rate (include/mpcvr.h: mpcvr_process_batch_deint).  Everything about the arguments is answered first; then the output
// frames are cut into chunks of PlanBatchDeint's size, and each chunk is the pass with a frame dimension (one launch per distinct (bytes,
// cs) among the planes) into the context-owned sample surface and the batch machinery behind it (RunSampleChunks).
HRESULT CHipVideoProcessor::ProcessBatchDeint(int n, const void *const *frames, int fieldOrder, int fieldsPerFrame, int mode, void *const *dsts, int rtPitch)
{
    const bool fpfOk = fieldsPerFrame == 1 || fieldsPerFrame == 2;
    const int nOut = n > 0 && n <= (1 << 24) && fpfOk ? n * fieldsPerFrame : 0;
    const BatchRecord record(*this, nOut);
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (n <= 0 || n > (1 << 24)) return Fail(MPCVR_E_INVALIDARG, "empty batch");
    if (!frames || !dsts) return Fail(MPCVR_E_POINTER, "null array of samples or frames");
    if (!fpfOk || (fieldOrder != 1 && fieldOrder != 2) || (mode != DI_ADAPTIVE && mode != DI_ADAPTIVE_NOCHECK))
        return Fail(MPCVR_E_INVALIDARG, "fields_per_frame is 1 or 2, field_order 1 or 2, mode MPCVR_DEINT_ADAPTIVE_EXT or MPCVR_DEINT_ADAPTIVE_NOCHECK_EXT");
    for (int i = 0; i < n + 2; i++)
        if (!frames[i]) return Fail(MPCVR_E_POINTER, "null sample in batch");
    for (int k = 0; k < nOut; k++)
        if (!dsts[k]) return Fail(MPCVR_E_POINTER, "null frame in batch");
    DeintPlane sp[kDeintMaxPlanes];
    int np = 0;
    if (!PlanDeintPlanes(m_srcParams->cformat, m_srcWidth, m_srcHeight, m_srcPitch, &np, sp))
        return Fail(MPCVR_E_INVALIDARG, "the input must be a planar or bi-planar format of at least 2 lines per plane");
    const int bytes = sp[0].bytes;
    std::vector<const void *> curs((size_t)nOut);
    for (int k = 0; k < nOut; k++) curs[k] = frames[1 + k / fieldsPerFrame];
    if (HRESULT bad = CheckBatchArgs(nOut, curs.data(), dsts, rtPitch)) return bad;
    uintptr_t bits = 0;
    for (int i = 0; i < n + 2; i++) bits |= (uintptr_t)frames[i];
    if (bits & (uintptr_t)(bytes - 1)) return Fail(MPCVR_E_INVALIDARG, "samples must be multiples of the component size");
    ChunkLayout lay;
    if (!PlanBatchDeint(m_srcPitch, m_srcLines, nOut, m_yuvBudget, &lay)) return Fail(MPCVR_E_INVALIDARG, "sample layout");

    (void)hipSetDevice(m_device);
    if (HRESULT bad = m_planDirty ? UpdatePlan() : MPCVR_S_OK) return bad;
    // (dstvec holds for every chunk: every frame of the surface starts on 256 bytes; srcvec only if every sample of the call allows it)
    DeintParams g[2];
    int cs[2];
    const int ng = DeintGroupParams(sp, sp, np, g, cs);
    for (int i = 0; i < ng; i++) g[i].srcvec &= (bits & ((uintptr_t)(kDeintLaneSteps * cs[i] * bytes) - 1)) == 0;
    return RunSampleChunks(nOut, lay, dsts, rtPitch, "deint", [&](int at, int m, const void *const *samples, hipStream_t stream) {
        // the frames' table through the frame tables' ring; the lease ends behind the pass
        SlotLease table;
        HRESULT hr = m_tableRing.SendRows<DeintFrame>(m, stream, "deint table", &table, [&](DeintFrame *fr) {
            for (int i = 0; i < m; i++) {
                const int k = at + i, f = 1 + k / fieldsPerFrame;
                int keep, first;
                FieldParity(fieldOrder, k % fieldsPerFrame, &keep, &first);
                fr[i] = DeintFrame{(const uint8_t *)frames[f - 1], (const uint8_t *)frames[f], (const uint8_t *)frames[f + 1],
                                   (uint8_t *)const_cast<void *>(samples[i]), keep, first};
            }
        });
        for (int i = 0; i < ng && !hr; i++) {
            DeintParams p = g[i];
            p.frames = (const DeintFrame *)table.dev;
            hr = CheckHip(LaunchDeint(p, bytes, cs[i], mode, stream, m), "k_deint");
        }
        return hr;
    });
}

// ------------------------------------------------------------------------------------------------
// EXTENSION — a 3D colour LUT over rendered frames (include/mpcvr.h: mpcvr_lut3d_pass, mpcvr_render_lut3d, mpcvr_process_batch_lut3d;
// kernel: vp_lut3d.hip).  No reference line: the reference has no LUT.
// ------------------------------------------------------------------------------------------------
// What a k_lut3d launch is given, but for its surfaces: src / dst or the frame table are the caller's, who takes src16 / dst16 back where a
// pointer of the launch is off 16 bytes (here they say what the pitches allow), as in TensorLaunchParams
static Lut3dParams Lut3dLaunchParams(int w, int h, int srcPitch, int dstPitch, const void *lutDev, int n)
{
    Lut3dParams p{};
    p.src_pitch = srcPitch; p.dst_pitch = dstPitch; p.w = w; p.h = h;
    p.lut = (const Lut3dEntry *)lutDev; p.n = n;
    p.src16 = (srcPitch & 15) == 0;
    p.dst16 = (dstPitch & 15) == 0;
    return p;
}

HRESULT Lut3dSurface(const void *src, int srcPitch, int srcFmt, int w, int h, const void *lutDev, int n, void *dst, int dstPitch, int dstFmt,
                     hipStream_t stream, bool checkOnly, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    if ((!src && !checkOnly) || !lutDev || !dst) { *why = "null surface, table or destination"; return MPCVR_E_POINTER; }      // (checkOnly: a source still to be allocated)
    if ((srcFmt != MPCVR_OUT_BGRA8 && srcFmt != MPCVR_OUT_RGB10A2) || (dstFmt != MPCVR_OUT_BGRA8 && dstFmt != MPCVR_OUT_RGB10A2)) {
        *why = "source and destination BGRA8 or RGB10A2"; return MPCVR_E_INVALIDARG;
    }
    if (w < 1 || h < 1 || w > 32768 || h > 32768) { *why = "width and height must be 1 .. 32768"; return MPCVR_E_INVALIDARG; }
    if (n < kLut3dMinN || n > kLut3dMaxN) { *why = "the table's size must be 2 .. 65"; return MPCVR_E_INVALIDARG; }
    if (srcPitch < 4 * w || dstPitch < 4 * w) { *why = "pitch smaller than a row"; return MPCVR_E_INVALIDARG; }
    if (((uintptr_t)src | (uintptr_t)srcPitch | (uintptr_t)dst | (uintptr_t)dstPitch) & 3) { *why = "surfaces and pitches must be multiples of 4"; return MPCVR_E_INVALIDARG; }
    if ((uintptr_t)lutDev & 7) { *why = "the table must be 8-byte aligned"; return MPCVR_E_INVALIDARG; }
    const RtSpan s = RowsSpan(src, (size_t)srcPitch, h, (size_t)4 * w), d = RowsSpan(dst, (size_t)dstPitch, h, (size_t)4 * w);
    const RtSpan t{(uintptr_t)lutDev, (uintptr_t)lutDev + Lut3dTableBytes(n)};
    // in place — the same first pixel and the same pitch — is the one overlap of the two surfaces a lane's read-then-write order covers
    if (src && d.Overlaps(s) && !(dst == src && dstPitch == srcPitch)) { *why = "the destination overlaps the source without being the source"; return MPCVR_E_INVALIDARG; }
    if (t.Overlaps(d)) { *why = "the table overlaps the destination"; return MPCVR_E_INVALIDARG; }
    if (checkOnly) return MPCVR_S_OK;
    Lut3dParams p = Lut3dLaunchParams(w, h, srcPitch, dstPitch, lutDev, n);
    p.src = (const uint8_t *)src; p.dst = (uint8_t *)dst;
    p.src16 &= (s.lo & 15) == 0;
    p.dst16 &= (d.lo & 15) == 0;
    if (LaunchLut3d(p, srcFmt == MPCVR_OUT_RGB10A2, dstFmt == MPCVR_OUT_RGB10A2, stream) != hipSuccess) { *why = "k_lut3d launch failed"; return MPCVR_E_FAIL; }
    return MPCVR_S_OK;
}

// Render, then the pass from the back buffer over the whole window into the caller's target, ordered as RenderYuv (the comment there): on
// the context stream, the lanes' next work behind the pass.  The back buffer is only read: it stays the frame a plain Render leaves.
HRESULT CHipVideoProcessor::RenderLut3d(int /*field*/, const void *lutDev, int n, void *dst, int dstPitch, int dstFmt)
{
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    (void)hipSetDevice(m_device);
    const int w = m_windowRect.Width(), h = m_windowRect.Height();
    // everything about the table and the target is answered before anything is drawn (a back buffer Render has yet to allocate cannot overlap them)
    const bool have = m_BackBuffer.ptr && m_BackBuffer.size >= (size_t)w * 4 * h;
    HRESULT hr;
    const char *why = "";
    if ((hr = Lut3dSurface(have ? m_BackBuffer.ptr : nullptr, w * 4, m_cfg.output_format, w, h, lutDev, n, dst, dstPitch, dstFmt, nullptr, true, &why))) return Fail(hr, why);
    if (!m_curSample) return MPCVR_S_FALSE;          // nothing to draw, as Render
    if ((hr = RenderBackBuffer(true)) != MPCVR_S_OK) return hr;
    hr = Lut3dSurface(m_BackBuffer.ptr, w * 4, m_cfg.output_format, w, h, lutDev, n, dst, dstPitch, dstFmt, m_stream, false, &why);
    m_launches++;
    m_lanes.NoteStreamWork();
    return hr ? Fail(hr, why) : MPCVR_S_OK;
}

// A batch through the table (include/mpcvr.h: mpcvr_process_batch_lut3d): ProcessBatchTensor with k_lut3d as the chunk's pass and the
// caller's render targets as what it writes.  Everything about the arguments is answered first; the chunks, their surfaces, lanes and order
// are RunSurfaceChunks'.
HRESULT CHipVideoProcessor::ProcessBatchLut3d(int n, const void *const *srcs, const void *lutDev, int lutN, void *const *dsts, int dstPitch, int dstFmt)
{
    const BatchRecord record(*this, n > 0 ? n : 0);
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (n <= 0) return Fail(MPCVR_E_INVALIDARG, "empty batch");
    if (!srcs || !dsts || !lutDev) return Fail(MPCVR_E_POINTER, "null array of frames or targets, or null table");
    for (int i = 0; i < n; i++)
        if (!srcs[i] || !dsts[i]) return Fail(MPCVR_E_POINTER, "null frame or target in batch");
    const int w = m_windowRect.Width(), h = m_windowRect.Height();
    BatchYuvLayout lay;
    if (!PlanBatchTensor(w, h, n, m_yuvBudget, &lay)) return Fail(MPCVR_E_INVALIDARG, "the pass needs a window width and height of 1 .. 32768");
    // what the pass refuses, per frame, the table against the target included (the surface is still to be allocated: it cannot overlap either) ...
    const char *why = "";
    for (int i = 0; i < n; i++)
        if (HRESULT bad = Lut3dSurface(nullptr, lay.surfacePitch, m_cfg.output_format, w, h, lutDev, lutN, dsts[i], dstPitch, dstFmt, nullptr, true, &why)) return Fail(bad, why);
    // ... and the targets against each other
    std::vector<RtSpan> targets((size_t)n);
    for (int i = 0; i < n; i++) targets[i] = RowsSpan(dsts[i], (size_t)dstPitch, h, (size_t)4 * w);
    if (AnyTwoSpansOverlap(targets)) return Fail(MPCVR_E_INVALIDARG, "two targets of the batch overlap");

    (void)hipSetDevice(m_device);
    if (HRESULT bad = m_planDirty ? UpdatePlan() : MPCVR_S_OK) return bad;
    const Lut3dParams lp = Lut3dLaunchParams(w, h, lay.surfacePitch, dstPitch, lutDev, lutN);      // (src16 holds for every chunk: every frame of a surface starts on 256 bytes)
    const bool in10 = m_cfg.output_format == MPCVR_OUT_RGB10A2, out10 = dstFmt == MPCVR_OUT_RGB10A2;
    const HRESULT hr = RunSurfaceChunks(n, srcs, lay, "lut3d",
        [&](int at, int m) { return std::vector<RtSpan>(targets.begin() + (size_t)at, targets.begin() + (size_t)(at + m)); },
        [&](BatchRun &run, int at) {
            // the targets' table through the frame tables' ring; the lease ends behind the pass
            SlotLease table;
            Lut3dParams p = lp;
            if (HRESULT bad = m_tableRing.SendRows<Lut3dFrame>(run.n, run.on.stream, "lut3d frame table", &table, [&](Lut3dFrame *fr) {
                    for (int i = 0; i < run.n; i++) {
                        fr[i] = Lut3dFrame{(const uint8_t *)run.dsts[i], (uint8_t *)dsts[at + i]};
                        p.dst16 &= ((uintptr_t)dsts[at + i] & 15) == 0;      // the 16-byte stores only if every target of the launch allows them
                    }
                })) return bad;
            p.frames = (const Lut3dFrame *)table.dev;
            return CheckHip(LaunchLut3d(p, in10, out10, run.on.stream, run.n), "k_lut3d");
        });
    m_yuvLastInfo += std::string(";lut3d_table=") + Lut3dPlaceName(Lut3dPlaceFor(lutN));
    return hr;
}

// ------------------------------------------------------------------------------------------------
// EXTENSION — debanding of rendered frames (include/mpcvr.h: mpcvr_deband_pass, mpcvr_render_deband, mpcvr_process_batch_deband;
// kernel: vp_deband.hip).  No reference line: the reference has no deband.
// ------------------------------------------------------------------------------------------------
// What a k_deband launch is given, but for its surfaces and seed(s), as Lut3dLaunchParams
static DebandParams DebandLaunchParams(int w, int h, int srcPitch, int dstPitch, const mpcvr_deband_params &params)
{
    DebandParams p{};
    p.src_pitch = srcPitch; p.dst_pitch = dstPitch; p.w = w; p.h = h;
    p.a = DebandArgs{params.range, params.iterations, params.threshold, params.dither};
    p.src16 = (srcPitch & 15) == 0;
    p.dst16 = (dstPitch & 15) == 0;
    return p;
}

HRESULT DebandSurface(const void *src, int srcPitch, int srcFmt, int w, int h, const mpcvr_deband_params *params, uint32_t seed, void *dst, int dstPitch,
                      int dstFmt, hipStream_t stream, bool checkOnly, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    if ((!src && !checkOnly) || !params || !dst) { *why = "null surface, parameters or destination"; return MPCVR_E_POINTER; }      // (checkOnly: a source still to be allocated)
    if ((srcFmt != MPCVR_OUT_BGRA8 && srcFmt != MPCVR_OUT_RGB10A2) || (dstFmt != MPCVR_OUT_BGRA8 && dstFmt != MPCVR_OUT_RGB10A2)) {
        *why = "source and destination BGRA8 or RGB10A2"; return MPCVR_E_INVALIDARG;
    }
    if (w < 1 || h < 1 || w > 32768 || h > 32768) { *why = "width and height must be 1 .. 32768"; return MPCVR_E_INVALIDARG; }
    const DebandArgs a{params->range, params->iterations, params->threshold, params->dither};
    if (!DebandArgsValid(a, srcFmt == MPCVR_OUT_RGB10A2)) { *why = "range 1 .. 64, iterations 1 .. 4, range * iterations <= 64, threshold 0 .. 4 maxin, dither 0 / 1"; return MPCVR_E_INVALIDARG; }
    if (srcPitch < 4 * w || dstPitch < 4 * w) { *why = "pitch smaller than a row"; return MPCVR_E_INVALIDARG; }
    if (((uintptr_t)src | (uintptr_t)srcPitch | (uintptr_t)dst | (uintptr_t)dstPitch) & 3) { *why = "surfaces and pitches must be multiples of 4"; return MPCVR_E_INVALIDARG; }
    const RtSpan s = RowsSpan(src, (size_t)srcPitch, h, (size_t)4 * w), d = RowsSpan(dst, (size_t)dstPitch, h, (size_t)4 * w);
    // the pass reads neighbours: no overlap at all, in place included
    if (src && d.Overlaps(s)) { *why = "the destination overlaps the source"; return MPCVR_E_INVALIDARG; }
    if (checkOnly) return MPCVR_S_OK;
    DebandParams p = DebandLaunchParams(w, h, srcPitch, dstPitch, *params);
    p.src = (const uint8_t *)src; p.dst = (uint8_t *)dst; p.seed = seed;
    p.src16 &= (s.lo & 15) == 0;
    p.dst16 &= (d.lo & 15) == 0;
    if (LaunchDeband(p, srcFmt == MPCVR_OUT_RGB10A2, dstFmt == MPCVR_OUT_RGB10A2, stream) != hipSuccess) { *why = "k_deband launch failed"; return MPCVR_E_FAIL; }
    return MPCVR_S_OK;
}

// Render, then the pass from the back buffer over the whole window into the caller's target, ordered as RenderLut3d
HRESULT CHipVideoProcessor::RenderDeband(int /*field*/, const mpcvr_deband_params *params, uint32_t seed, void *dst, int dstPitch, int dstFmt)
{
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    (void)hipSetDevice(m_device);
    const int w = m_windowRect.Width(), h = m_windowRect.Height();
    // everything about the parameters and the target is answered before anything is drawn (a back buffer Render has yet to allocate cannot overlap it)
    const bool have = m_BackBuffer.ptr && m_BackBuffer.size >= (size_t)w * 4 * h;
    HRESULT hr;
    const char *why = "";
    if ((hr = DebandSurface(have ? m_BackBuffer.ptr : nullptr, w * 4, m_cfg.output_format, w, h, params, seed, dst, dstPitch, dstFmt, nullptr, true, &why))) return Fail(hr, why);
    if (!m_curSample) return MPCVR_S_FALSE;          // nothing to draw, as Render
    if ((hr = RenderBackBuffer(true)) != MPCVR_S_OK) return hr;
    hr = DebandSurface(m_BackBuffer.ptr, w * 4, m_cfg.output_format, w, h, params, seed, dst, dstPitch, dstFmt, m_stream, false, &why);
    m_launches++;
    m_lanes.NoteStreamWork();
    return hr ? Fail(hr, why) : MPCVR_S_OK;
}

// A batch through the pass (include/mpcvr.h: mpcvr_process_batch_deband): ProcessBatchLut3d with k_deband as the chunk's pass and a seed
// per frame.  Everything about the arguments is answered first; the chunks, their surfaces, lanes and order are RunSurfaceChunks'.
HRESULT CHipVideoProcessor::ProcessBatchDeband(int n, const void *const *srcs, const mpcvr_deband_params *params, uint32_t seed, void *const *dsts, int dstPitch, int dstFmt)
{
    const BatchRecord record(*this, n > 0 ? n : 0);
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (n <= 0) return Fail(MPCVR_E_INVALIDARG, "empty batch");
    if (!srcs || !dsts || !params) return Fail(MPCVR_E_POINTER, "null array of frames or targets, or null parameters");
    for (int i = 0; i < n; i++)
        if (!srcs[i] || !dsts[i]) return Fail(MPCVR_E_POINTER, "null frame or target in batch");
    const int w = m_windowRect.Width(), h = m_windowRect.Height();
    BatchYuvLayout lay;
    if (!PlanBatchTensor(w, h, n, m_yuvBudget, &lay)) return Fail(MPCVR_E_INVALIDARG, "the pass needs a window width and height of 1 .. 32768");
    // what the pass refuses, per frame (the surface is still to be allocated: it cannot overlap a target) ...
    const char *why = "";
    for (int i = 0; i < n; i++)
        if (HRESULT bad = DebandSurface(nullptr, lay.surfacePitch, m_cfg.output_format, w, h, params, seed, dsts[i], dstPitch, dstFmt, nullptr, true, &why)) return Fail(bad, why);
    // ... and the targets against each other
    std::vector<RtSpan> targets((size_t)n);
    for (int i = 0; i < n; i++) targets[i] = RowsSpan(dsts[i], (size_t)dstPitch, h, (size_t)4 * w);
    if (AnyTwoSpansOverlap(targets)) return Fail(MPCVR_E_INVALIDARG, "two targets of the batch overlap");

    (void)hipSetDevice(m_device);
    if (HRESULT bad = m_planDirty ? UpdatePlan() : MPCVR_S_OK) return bad;
    const DebandParams lp = DebandLaunchParams(w, h, lay.surfacePitch, dstPitch, *params);      // (src16 holds for every chunk: every frame of a surface starts on 256 bytes)
    const bool in10 = m_cfg.output_format == MPCVR_OUT_RGB10A2, out10 = dstFmt == MPCVR_OUT_RGB10A2;
    const HRESULT hr = RunSurfaceChunks(n, srcs, lay, "deband",
        [&](int at, int m) { return std::vector<RtSpan>(targets.begin() + (size_t)at, targets.begin() + (size_t)(at + m)); },
        [&](BatchRun &run, int at) {
            // the targets' and seeds' table through the frame tables' ring; the lease ends behind the pass
            SlotLease table;
            DebandParams p = lp;
            if (HRESULT bad = m_tableRing.SendRows<DebandFrame>(run.n, run.on.stream, "deband frame table", &table, [&](DebandFrame *fr) {
                    for (int i = 0; i < run.n; i++) {
                        fr[i] = DebandFrame{(const uint8_t *)run.dsts[i], (uint8_t *)dsts[at + i], seed + (uint32_t)(at + i), 0u};
                        p.dst16 &= ((uintptr_t)dsts[at + i] & 15) == 0;      // the 16-byte stores only if every target of the launch allows them
                    }
                })) return bad;
            p.frames = (const DebandFrame *)table.dev;
            return CheckHip(LaunchDeband(p, in10, out10, run.on.stream, run.n), "k_deband");
        });
    m_yuvLastInfo += std::string(";deband_taps=") + DebandPlaceName(DebandPlaceFor(params->range * params->iterations, w, h));
    return hr;
}

// ------------------------------------------------------------------------------------------------
// EXTENSION — sharpening of rendered frames (include/mpcvr.h: mpcvr_sharpen_pass, mpcvr_render_sharpen, mpcvr_process_batch_sharpen;
// kernel: vp_sharpen.hip).  No reference line: the reference has no sharpener.
// ------------------------------------------------------------------------------------------------
static SharpenArgs SharpenArgsOf(const mpcvr_sharpen_params &p) { return SharpenArgs{p.radius, p.amount, p.threshold, p.overshoot, p.mode, p.dither}; }

// What a k_sharpen launch is given, but for its surfaces and seed(s), as DebandLaunchParams
static SharpenParams SharpenLaunchParams(int w, int h, int srcPitch, int dstPitch, const mpcvr_sharpen_params &params)
{
    SharpenParams p{};
    p.src_pitch = srcPitch; p.dst_pitch = dstPitch; p.w = w; p.h = h;
    p.a = SharpenArgsOf(params);
    p.src16 = (srcPitch & 15) == 0;
    p.dst16 = (dstPitch & 15) == 0;
    return p;
}

HRESULT SharpenSurface(const void *src, int srcPitch, int srcFmt, int w, int h, const mpcvr_sharpen_params *params, uint32_t seed, void *dst, int dstPitch,
                       int dstFmt, hipStream_t stream, bool checkOnly, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    if ((!src && !checkOnly) || !params || !dst) { *why = "null surface, parameters or destination"; return MPCVR_E_POINTER; }      // (checkOnly: a source still to be allocated)
    if ((srcFmt != MPCVR_OUT_BGRA8 && srcFmt != MPCVR_OUT_RGB10A2) || (dstFmt != MPCVR_OUT_BGRA8 && dstFmt != MPCVR_OUT_RGB10A2)) {
        *why = "source and destination BGRA8 or RGB10A2"; return MPCVR_E_INVALIDARG;
    }
    if (w < 1 || h < 1 || w > 32768 || h > 32768) { *why = "width and height must be 1 .. 32768"; return MPCVR_E_INVALIDARG; }
    if (!SharpenArgsValid(SharpenArgsOf(*params), srcFmt == MPCVR_OUT_RGB10A2)) { *why = "radius 1 .. 3, amount 0 .. 256, threshold 0 .. 4 maxin, overshoot 0 .. maxin, mode 0 / 1, dither 0 / 1"; return MPCVR_E_INVALIDARG; }
    if (srcPitch < 4 * w || dstPitch < 4 * w) { *why = "pitch smaller than a row"; return MPCVR_E_INVALIDARG; }
    if (((uintptr_t)src | (uintptr_t)srcPitch | (uintptr_t)dst | (uintptr_t)dstPitch) & 3) { *why = "surfaces and pitches must be multiples of 4"; return MPCVR_E_INVALIDARG; }
    const RtSpan s = RowsSpan(src, (size_t)srcPitch, h, (size_t)4 * w), d = RowsSpan(dst, (size_t)dstPitch, h, (size_t)4 * w);
    // the pass reads neighbours: no overlap at all, in place included
    if (src && d.Overlaps(s)) { *why = "the destination overlaps the source"; return MPCVR_E_INVALIDARG; }
    if (checkOnly) return MPCVR_S_OK;
    SharpenParams p = SharpenLaunchParams(w, h, srcPitch, dstPitch, *params);
    p.src = (const uint8_t *)src; p.dst = (uint8_t *)dst; p.seed = seed;
    p.src16 &= (s.lo & 15) == 0;
    p.dst16 &= (d.lo & 15) == 0;
    if (LaunchSharpen(p, srcFmt == MPCVR_OUT_RGB10A2, dstFmt == MPCVR_OUT_RGB10A2, stream) != hipSuccess) { *why = "k_sharpen launch failed"; return MPCVR_E_FAIL; }
    return MPCVR_S_OK;
}

// Render, then the pass from the back buffer over the whole window into the caller's target, ordered as RenderDeband
HRESULT CHipVideoProcessor::RenderSharpen(int /*field*/, const mpcvr_sharpen_params *params, uint32_t seed, void *dst, int dstPitch, int dstFmt)
{
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    (void)hipSetDevice(m_device);
    const int w = m_windowRect.Width(), h = m_windowRect.Height();
    // everything about the parameters and the target is answered before anything is drawn (a back buffer Render has yet to allocate cannot overlap it)
    const bool have = m_BackBuffer.ptr && m_BackBuffer.size >= (size_t)w * 4 * h;
    HRESULT hr;
    const char *why = "";
    if ((hr = SharpenSurface(have ? m_BackBuffer.ptr : nullptr, w * 4, m_cfg.output_format, w, h, params, seed, dst, dstPitch, dstFmt, nullptr, true, &why))) return Fail(hr, why);
    if (!m_curSample) return MPCVR_S_FALSE;          // nothing to draw, as Render
    if ((hr = RenderBackBuffer(true)) != MPCVR_S_OK) return hr;
    hr = SharpenSurface(m_BackBuffer.ptr, w * 4, m_cfg.output_format, w, h, params, seed, dst, dstPitch, dstFmt, m_stream, false, &why);
    m_launches++;
    m_lanes.NoteStreamWork();
    return hr ? Fail(hr, why) : MPCVR_S_OK;
}

// A batch through the pass (include/mpcvr.h: mpcvr_process_batch_sharpen): ProcessBatchDeband with k_sharpen as the chunk's pass.
// Everything about the arguments is answered first; the chunks, their surfaces, lanes and order are RunSurfaceChunks'.
HRESULT CHipVideoProcessor::ProcessBatchSharpen(int n, const void *const *srcs, const mpcvr_sharpen_params *params, uint32_t seed, void *const *dsts, int dstPitch, int dstFmt)
{
    const BatchRecord record(*this, n > 0 ? n : 0);
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (n <= 0) return Fail(MPCVR_E_INVALIDARG, "empty batch");
    if (!srcs || !dsts || !params) return Fail(MPCVR_E_POINTER, "null array of frames or targets, or null parameters");
    for (int i = 0; i < n; i++)
        if (!srcs[i] || !dsts[i]) return Fail(MPCVR_E_POINTER, "null frame or target in batch");
    const int w = m_windowRect.Width(), h = m_windowRect.Height();
    BatchYuvLayout lay;
    if (!PlanBatchTensor(w, h, n, m_yuvBudget, &lay)) return Fail(MPCVR_E_INVALIDARG, "the pass needs a window width and height of 1 .. 32768");
    // what the pass refuses, per frame (the surface is still to be allocated: it cannot overlap a target) ...
    const char *why = "";
    for (int i = 0; i < n; i++)
        if (HRESULT bad = SharpenSurface(nullptr, lay.surfacePitch, m_cfg.output_format, w, h, params, seed, dsts[i], dstPitch, dstFmt, nullptr, true, &why)) return Fail(bad, why);
    // ... and the targets against each other
    std::vector<RtSpan> targets((size_t)n);
    for (int i = 0; i < n; i++) targets[i] = RowsSpan(dsts[i], (size_t)dstPitch, h, (size_t)4 * w);
    if (AnyTwoSpansOverlap(targets)) return Fail(MPCVR_E_INVALIDARG, "two targets of the batch overlap");

    (void)hipSetDevice(m_device);
    if (HRESULT bad = m_planDirty ? UpdatePlan() : MPCVR_S_OK) return bad;
    const SharpenParams lp = SharpenLaunchParams(w, h, lay.surfacePitch, dstPitch, *params);      // (src16 holds for every chunk: every frame of a surface starts on 256 bytes)
    const bool in10 = m_cfg.output_format == MPCVR_OUT_RGB10A2, out10 = dstFmt == MPCVR_OUT_RGB10A2;
    return RunSurfaceChunks(n, srcs, lay, "sharpen",
        [&](int at, int m) { return std::vector<RtSpan>(targets.begin() + (size_t)at, targets.begin() + (size_t)(at + m)); },
        [&](BatchRun &run, int at) {
            // the targets' and seeds' table through the frame tables' ring; the lease ends behind the pass
            SlotLease table;
            SharpenParams p = lp;
            if (HRESULT bad = m_tableRing.SendRows<SharpenFrame>(run.n, run.on.stream, "sharpen frame table", &table, [&](SharpenFrame *fr) {
                    for (int i = 0; i < run.n; i++) {
                        fr[i] = SharpenFrame{(const uint8_t *)run.dsts[i], (uint8_t *)dsts[at + i], seed + (uint32_t)(at + i), 0u};
                        p.dst16 &= ((uintptr_t)dsts[at + i] & 15) == 0;      // the 16-byte stores only if every target of the launch allows them
                    }
                })) return bad;
            p.frames = (const SharpenFrame *)table.dev;
            return CheckHip(LaunchSharpen(p, in10, out10, run.on.stream, run.n), "k_sharpen");
        });
}

}  // namespace mpcvr
