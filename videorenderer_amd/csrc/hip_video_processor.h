// hip_video_processor.h — CHipVideoProcessor: the MI355X-native stand-in for the shader path of
// CDX11VideoProcessor (Source/DX11VideoProcessor.h:256-384).  Method names follow the reference's
// so the call sites in CMpcVideoRenderer map one-to-one; the D3D11 device/swap-chain/OSD/subtitle
// members have no counterpart here (out of scope).
#pragma once
#include <hip/hip_runtime_api.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/mpcvr.h"
#include "vp_encode.h"
#include "vp_lanes.h"
#include "vp_measure.h"
#include "vp_tensor.h"
#include "vp_tensor_in.h"
#include "vp_deint.h"
#include "vp_lut3d.h"
#include "vp_deband.h"
#include "vp_sharpen.h"
#include "vp_launch.h"
#include "vp_params.h"
#include "vp_plan.h"
#include "vp_plan_tables.h"

namespace mpcvr {

typedef int32_t HRESULT;

struct CRect {
    int left = 0, top = 0, right = 0, bottom = 0;
    CRect() = default;
    CRect(int l, int t, int r, int b) : left(l), top(t), right(r), bottom(b) {}
    int Width() const { return right - left; }
    int Height() const { return bottom - top; }
    bool IsRectNull() const { return !left && !top && !right && !bottom; }
    bool operator==(const CRect &o) const { return left == o.left && top == o.top && right == o.right && bottom == o.bottom; }
    bool operator!=(const CRect &o) const { return !(*this == o); }
};

// device allocation that only grows (CheckCreate analogue of Tex2D_t, DX11Helper.h:37-90)
struct DevBuffer {
    void *ptr = nullptr;
    size_t size = 0;
    hipError_t CheckCreate(size_t bytes);
    void Release();
};

// EXTENSION (mpcvr_encode_pass, include/mpcvr.h): checks every argument, then — unless checkOnly — launches k_encode420 on `stream`.
// MPCVR_E_POINTER / MPCVR_E_INVALIDARG with nothing launched; *why (optional) names the refusal.  checkOnly takes src = nullptr for a source
// that is still to be allocated (it cannot overlap the planes)
HRESULT EncodeSurface(const void *src, int srcPitch, int srcFmt, int w, int h, int outCformat, uint32_t extfmt, void *yPlane, int yPitch,
                      void *uvPlane, int uvPitch, hipStream_t stream, bool checkOnly, const char **why = nullptr);

// EXTENSION (mpcvr_measure_pass, include/mpcvr.h): checks every argument, then — unless checkOnly — clears the histogram and launches
// k_measure_maxrgb on `stream`.  rect = nullptr: the whole surface.  MPCVR_E_POINTER / MPCVR_E_INVALIDARG with nothing launched or written
HRESULT MeasureSurface(const void *src, int srcPitch, int srcFmt, int w, int h, const mpcvr_rect *rect, uint32_t *histDev, hipStream_t stream,
                       bool checkOnly, const char **why = nullptr);

// EXTENSION (mpcvr_tensor_pass, include/mpcvr.h): checks every argument, then — unless checkOnly — launches k_tensor on `stream`.
// MPCVR_E_POINTER / MPCVR_E_INVALIDARG with nothing launched or written
HRESULT TensorSurface(const void *src, int srcPitch, int srcFmt, int w, int h, const mpcvr_tensor_desc *desc, void *dst, hipStream_t stream,
                      bool checkOnly, const char **why = nullptr);

// EXTENSION (mpcvr_sample_pass, include/mpcvr.h): checks every argument, then — unless checkOnly — launches k_sample_from_tensor on `stream`.
// MPCVR_E_POINTER / MPCVR_E_INVALIDARG with nothing launched or written.  checkOnly takes sample = nullptr for a sample that is still to be
// allocated (it cannot overlap the tensor; its alignment is the allocator's)
HRESULT SampleSurface(const void *tensor, const mpcvr_tensor_desc *desc, int w, int h, int cformat, void *sample, int pitch, hipStream_t stream,
                      bool checkOnly, const char **why = nullptr);

// EXTENSION (mpcvr_deint_pass, include/mpcvr.h): checks every argument, then — unless checkOnly — launches k_deint on `stream`, once per
// distinct (bytes, cs) among the planes; *launches (optional) is told how many.  MPCVR_E_POINTER / MPCVR_E_INVALIDARG with nothing launched
// or written.  checkOnly takes dst = nullptr for a sample that is still to be allocated (it cannot overlap a source)
HRESULT DeintSurface(const void *prev, const void *cur, const void *next, int cformat, int w, int h, int pitch, int keep, int first, int mode,
                     void *dst, int dstPitch, hipStream_t stream, bool checkOnly, const char **why = nullptr, int *launches = nullptr);

// EXTENSION (mpcvr_lut3d_pass, include/mpcvr.h): checks every argument, then — unless checkOnly — launches k_lut3d on `stream`.
// MPCVR_E_POINTER / MPCVR_E_INVALIDARG with nothing launched or written.  checkOnly takes src = nullptr for a source that is still to be
// allocated (it cannot overlap the destination or the table)
HRESULT Lut3dSurface(const void *src, int srcPitch, int srcFmt, int w, int h, const void *lutDev, int n, void *dst, int dstPitch, int dstFmt,
                     hipStream_t stream, bool checkOnly, const char **why = nullptr);

// EXTENSION (mpcvr_deband_pass, include/mpcvr.h): checks every argument, then — unless checkOnly — launches k_deband on `stream`.
// MPCVR_E_POINTER / MPCVR_E_INVALIDARG with nothing launched or written.  checkOnly takes src = nullptr for a source that is still to be
// allocated (it cannot overlap the destination)
HRESULT DebandSurface(const void *src, int srcPitch, int srcFmt, int w, int h, const mpcvr_deband_params *params, uint32_t seed, void *dst, int dstPitch,
                      int dstFmt, hipStream_t stream, bool checkOnly, const char **why = nullptr);

// EXTENSION (mpcvr_sharpen_pass, include/mpcvr.h): checks every argument, then — unless checkOnly — launches k_sharpen on `stream`.
// MPCVR_E_POINTER / MPCVR_E_INVALIDARG with nothing launched or written.  checkOnly takes src = nullptr as DebandSurface does
HRESULT SharpenSurface(const void *src, int srcPitch, int srcFmt, int w, int h, const mpcvr_sharpen_params *params, uint32_t seed, void *dst, int dstPitch,
                       int dstFmt, hipStream_t stream, bool checkOnly, const char **why = nullptr);

class CHipVideoProcessor {
public:
    CHipVideoProcessor();
    ~CHipVideoProcessor();

    HRESULT Init(int device, const mpcvr_settings &settings);                 // ctor + Init (:381,547)
    HRESULT SetStream(hipStream_t s);
    HRESULT Synchronize();

    HRESULT InitMediaType(int cformat, int width, int height, int pitch, const CRect *srcRect, uint32_t extfmt); // :1742
    HRESULT SetVideoRect(const CRect &videoRect);                             // :3426
    HRESULT SetWindowRect(const CRect &windowRect);                           // :3433
    HRESULT SetRotation(int value);                                           // :4052
    // (extension) polls a band of the error-diffusion pass grants the band above before the launch is flagged failed; <= 0: the default (2^21,
    // about two seconds) — a host that shares the GPU, or runs under a debugger, raises it; one that wants a hard deadline lowers it
    HRESULT SetErrorDiffusionPatience(int polls) { m_edPatience = polls > 0 ? polls : 0; return MPCVR_S_OK; }
    HRESULT SetFlip(bool value);                                              // VideoProcessor.h:210
    HRESULT SetSampleFormat(int frameFormat);                                 // m_SampleFormat, :2209-2219
    HRESULT SetHdrOutput(bool enable, int toneMapType, float displayMaxNits);  // m_bHdrPassthrough / m_bHdrLocalToneMapping
    HRESULT SetHdrMetadata(float minMastering, float maxMastering, float maxCLL, float maxFALL);   // SetHDR10ShaderParams :907
    HRESULT SetDoviMetadata(const mpcvr_dovi_metadata *md);                   // CopySample :2270-2520 (IID_MediaSideDataDOVIMetadataV2)
    HRESULT Configure(const mpcvr_settings &config);                          // :3800
    HRESULT SetProcAmpValues(uint32_t flags, float b, float c, float h, float s); // :4506

    HRESULT CopySample(const void *data, int pitch, int memKind);             // :2202 / MemCopyToTexSrcVideo :1213
    HRESULT Process(void *rt, int rtPitch, const CRect *srcRect, const CRect *dstRect, bool /*second*/) { return ProcessFrame(rt, rtPitch, srcRect, dstRect, 0, false); }     // :3285
    HRESULT Render(int field) { return RenderBackBuffer(false); }             // :2599 minus Present
    // EXTENSION (mpcvr_render_yuv): Render, then the back buffer written as NV12 / P010 (vp_encode.h) behind it in stream order
    HRESULT RenderYuv(int field, int outCformat, uint32_t extfmt, void *yPlane, int yPitch, void *uvPlane, int uvPitch);
    // EXTENSION (mpcvr_measure_backbuffer): the histogram of the last rendered frame over video rect ∩ window, on the context stream
    HRESULT MeasureBackBuffer(uint32_t *histDev);
    HRESULT GetBackBuffer(void **ptr, int *pitch, int *w, int *h);
    HRESULT GetCurentImage(void *hostBGRA, size_t *size);                     // :3493
    HRESULT GetDisplayedImage(void *hostPixels, size_t *size, bool deepColor, int *width, int *height, int *bits);     // :3610
    HRESULT ProcessBatch(int n, const void *const *srcs, void *const *dsts, int rtPitch);
    // EXTENSION (mpcvr_process_batch_yuv): the batch in chunks through the batch machinery into a context-owned RGB surface, one k_encode420
    // launch (its frame dimension) behind each chunk on the same stream — the context stream, or a batch lane with a surface of its own
    // histDev (mpcvr_process_batch_yuv_stats; nullptr: none): n rows of kHistBins words, one k_measure_maxrgb launch behind each chunk's pass
    HRESULT ProcessBatchYuv(int n, const void *const *srcs, int outCformat, uint32_t extfmt, void *const *yPlanes, int yPitch, void *const *uvPlanes, int uvPitch,
                            uint32_t *histDev = nullptr);
    // EXTENSION (mpcvr_render_tensor / mpcvr_process_batch_tensor): Render / the batch, then k_tensor (vp_tensor.h) behind it in stream order;
    // the batch shares ProcessBatchYuv's surfaces, budget and chunk loop
    HRESULT RenderTensor(int field, const mpcvr_tensor_desc &desc, void *dst);
    HRESULT ProcessBatchTensor(int n, const void *const *srcs, const mpcvr_tensor_desc *desc, void *const *dsts);
    // EXTENSION (mpcvr_copy_sample_tensor / mpcvr_process_batch_from_tensors): a model's float tensor as the sample of a GBRP8 / 10 / 16
    // input — k_sample_from_tensor (vp_tensor_in.h) into an upload slot in place of the host-to-device copy; a batch through a
    // context-owned sample surface, one pass per chunk in front of the chunk's batch, everything on the context stream
    HRESULT CopySampleTensor(const void *tensor, const mpcvr_tensor_desc *desc);
    HRESULT ProcessBatchFromTensors(int n, const void *const *tensors, const mpcvr_tensor_desc *desc, void *const *dsts, int rtPitch);
    // EXTENSION (mpcvr_copy_sample_fields / mpcvr_process_batch_deint): one field of an interlaced sample, deinterlaced by k_deint (vp_deint.h)
    // into an upload slot in place of the host-to-device copy, as the current sample; a batch at field rate through the context-owned
    // sample surface, the pass (its frame dimension) in front of each chunk's batch, everything on the context stream
    HRESULT CopySampleFields(const void *prev, const void *cur, const void *next, int fieldOrder, int field, int mode);
    HRESULT ProcessBatchDeint(int n, const void *const *frames, int fieldOrder, int fieldsPerFrame, int mode, void *const *dsts, int rtPitch);
    // EXTENSION (mpcvr_render_lut3d / mpcvr_process_batch_lut3d): Render / the batch, then k_lut3d (vp_lut3d.h) behind it in stream order into the
    // caller's targets; the batch shares ProcessBatchYuv's surfaces, budget and chunk loop
    HRESULT RenderLut3d(int field, const void *lutDev, int n, void *dst, int dstPitch, int dstFmt);
    HRESULT ProcessBatchLut3d(int n, const void *const *srcs, const void *lutDev, int lutN, void *const *dsts, int dstPitch, int dstFmt);
    // EXTENSION (mpcvr_render_deband / mpcvr_process_batch_deband): Render / the batch, then k_deband (vp_deband.h) behind it in stream order into
    // the caller's targets; frame i of a batch takes seed + i; the batch shares ProcessBatchYuv's surfaces, budget and chunk loop
    HRESULT RenderDeband(int field, const mpcvr_deband_params *params, uint32_t seed, void *dst, int dstPitch, int dstFmt);
    HRESULT ProcessBatchDeband(int n, const void *const *srcs, const mpcvr_deband_params *params, uint32_t seed, void *const *dsts, int dstPitch, int dstFmt);
    // EXTENSION (mpcvr_render_sharpen / mpcvr_process_batch_sharpen): Render / the batch, then k_sharpen (vp_sharpen.h) behind it in stream order
    // into the caller's targets; frame i of a batch takes seed + i; the batch shares ProcessBatchYuv's surfaces, budget and chunk loop
    HRESULT RenderSharpen(int field, const mpcvr_sharpen_params *params, uint32_t seed, void *dst, int dstPitch, int dstFmt);
    HRESULT ProcessBatchSharpen(int n, const void *const *srcs, const mpcvr_sharpen_params *params, uint32_t seed, void *const *dsts, int dstPitch, int dstFmt);
    HRESULT SetBatchYuvBudget(size_t bytes) { m_yuvBudget = bytes; return MPCVR_S_OK; }
    std::string GetLastBatchInfo() const;
    HRESULT ProcessBatchDovi(int n, const void *const *srcs, void *const *dsts, int rtPitch, const mpcvr_dovi_metadata *rpus);
    void Flush();                                                             // :4074
    HRESULT Reset();                                                          // :3453

    HRESULT GetParamBlob(void *buf, size_t *size);
    HRESULT SetParamBlob(const void *buf, size_t size);
    // the current plan's baked table image for the exact-2x kernel (kBakedTableBytes; two-call size protocol)
    HRESULT GetFusedTables(void *buf, size_t *size);
    // the one collective of the path — rank `root`'s parameter blob to every rank of an RCCL communicator the host created
    // (ncclCommInitRank / ncclCommInitAll), on the context's stream.  Begin queues the broadcast (inside the host's ncclGroupStart /
    // ncclGroupEnd when one process drives several devices), End waits for it and adopts the blob on the other ranks.
    HRESULT BroadcastParamBlobBegin(void *ncclComm, int root, int rank);
    HRESULT BroadcastParamBlobEnd();
    HRESULT GetColorMatrix(float out[12]);
    HRESULT GetExtFmt(uint32_t *v);
    HRESULT GetFrameBytes(size_t *bytes, int *pitch);
    std::string GetPathInfo();
    HRESULT GetLastProcessMs(float *ms);
    HRESULT GetLastTimings(float *copy_host_ms, float *upload_ms, float *process_ms, float *readback_ms);
    const char *LastError() const { return m_lastError.c_str(); }

private:
    HRESULT Fail(HRESULT hr, const std::string &msg);
    HRESULT RenderBackBuffer(bool onContextStream);
    HRESULT CheckHip(hipError_t e, const char *what);

    // mirrors of the reference's private helpers
    void SetShaderConvertColorParams();                  // :813
    void SetShaderLuminanceParams();                     // :889
    HRESULT UpdatePlan();                                // UpdateTexures/UpdatePostScaleTexures/Update*scalingShaders
    // Where a frame or a batch is queued, handed down by value from Process / PlaceBatch to every launch: the stream (the context's,
    // or a frame lane's) and, for single-frame launches, how many frames the host keeps side by side (FusedParams::inflight)
    struct RunOn { hipStream_t stream = nullptr; int inflight = 1; };
    HRESULT ConvertColorPass(const uint8_t *sample, const RunOn &on);     // :3048
    FusedParams ConvertOutputParams(const uint8_t *sample, void *out, int inflight = 1) const;          // the block convert into m_TexConvertOutput
    // what ResizeShaderPass draws through, frame z of each surface at its pointer + z * its stride: one frame (the context's surfaces, no
    // tables, zero strides — what every launcher takes a null ResizeBatch for) or a chunk of a batch (ProcessBatchLaunches)
    struct DrawFrames {
        void *conv = nullptr, *mid = nullptr, *post = nullptr;     // m_TexConvertOutput, m_TexResize, the post-scale texture
        size_t convStride = 0, midStride = 0, postStride = 0;
        int n = 1;
        const FusedFrame *lastTab = nullptr;   // the last draw's targets: the render targets, or the post-scale slots with the HDR10 step
        const FusedFrame *rtTab = nullptr;     // the HDR10 step's render targets
        int aligned = 1;                       // with a table: every lastTab target on a 16-byte boundary (one frame: its target's address decides)
    };
    HRESULT ResizeShaderPass(const uint8_t *sample, void *rt, int rtPitch, const DrawFrames &df, const RunOn &on);     // :3103 (+ FinalPass :3189 fused into the last draw)
    HRESULT ProcessOne(const uint8_t *sample, void *rt, int rtPitch, const RunOn &on);
    // Process with what Render and the snapshot add: clearBytes of the back buffer are cleared in front of the frame, on whatever stream it
    // runs on; onContextStream: the frame stays off the lanes (a read-back follows on the context stream)
    HRESULT ProcessFrame(void *pRenderTarget, int rtPitch, const CRect *srcRect, const CRect *dstRect, size_t clearBytes, bool onContextStream);
    HRESULT UploadPlanTables(const PlanTables &t);     // one copy per axis pack, one for the strip pack; sets the views below
    bool ConvertEnabled() const;                       // m_PSConvColorData.bEnable (:849-853)
    int TexPitch() const;                              // row pitch of the source texture (differs from the sample's for v210)
    HRESULT PrepareSample(const uint8_t *dev_sample, const uint8_t **tex);   // device sample -> source texture
    void FillConvertParams(const uint8_t *sample, ConvertParams *P) const;
    StoreParams MakeStore(void *dst, int pitch, int dstFmt, bool rt) const;
    // (inflight: only a single frame on the lanes passes more than 1 — plan probes, ClassifyBatch and the batch routes take the default)
    void FillFusedParams(const uint8_t *sample, void *rt, int rtPitch, FusedParams *fp, int inflight = 1) const;

    bool m_bInit = false;
    int m_device = 0;
    hipStream_t m_stream = nullptr;         // the context stream, everywhere (Init / SetStream): what a call runs on travels as a RunOn
    bool m_ownStream = false;
    hipEvent_t m_evStart = nullptr, m_evStop = nullptr;
    bool m_timed = false;
    // FrameStats.h:145-173 beside paintticks: the last CopySample (host wall time = copyticks :2594, and its H2D transfer on the copy
    // stream) and the last GetCurentImage read-back
    hipEvent_t m_evUp0 = nullptr, m_evUp1 = nullptr, m_evRb0 = nullptr, m_evRb1 = nullptr;
    bool m_upTimed = false, m_rbTimed = false;
    float m_copyHostMs = -1.0f;
    std::string m_lastError;

    // settings (Settings_t mirror)
    mpcvr_settings m_cfg{};
    ProcAmp m_procAmp;
    int m_iRotation = 0;
    bool m_bFlip = false;
    int m_SampleFormat = 0;        // 0 progressive, 1 TFF, 2 BFF
    bool m_hdrOutput = false, m_hdrMetaValid = false;
    int m_hdrToneMapType = 0;
    float m_hdrDisplayMaxNits = 1000.0f, m_hdrMeta[4] = {0, 0, 0, 0};
    HdrToneMapParams m_hdrTm{};
    void UpdateHdrToneMapParams();
    // m_Dovi / m_DoviExtensionMetadata: the RPU of the current sample; L1 / L2 stay as last seen until Flush (:4082)
    struct DoviSlot { DoviParams *pinned = nullptr; hipEvent_t copied = nullptr; };
    bool m_doviValid = false;
    mpcvr_dovi_metadata m_doviMd{};
    DoviParams m_doviHost{};
    bool m_doviL1Present = false, m_doviL2Present = false;
    uint32_t m_doviL1[3] = {0, 0, 0};
    float m_doviL2Raw[5] = {0, 0, 0, 0, 0};       // cbuffer values for the last level-2 selection
    DevBuffer m_doviDev;
    DoviSlot m_doviSlots[4];
    unsigned m_doviSlotNext = 0;
    HRESULT UploadDoviParams();
    HRESULT ApplyDoviMetadata(const mpcvr_dovi_metadata *md);       // SetDoviMetadata without the upload
    // ProcessBatchDovi: one RPU per frame of a batch.  What the kernels of frame k read that its RPU decides ...
    struct DoviFrameState { DoviParams p; float cm[12]; HdrToneMapParams tm; };
    // ... and everything an RPU changes in the context (to take a step back when frame j turns out to open the next run)
    struct DoviWalkState {
        bool valid, l1Present, l2Present, blobOverride, planDirty;
        mpcvr_dovi_metadata md; DoviParams host; uint32_t l1[3]; float l2raw[5]; float cm[12]; int tail; float gamma; HdrToneMapParams tm;
    };
    void SaveDoviWalk(DoviWalkState *s) const;
    void RestoreDoviWalk(const DoviWalkState &s);
    // One batch call in flight, handed down by reference from ProcessBatch / ProcessBatchDovi to the launches: the frames, for a run of
    // ProcessBatchDovi its per-frame RPU state, and the stream PlaceBatch put it on.  Nothing of it outlives the call.
    struct BatchRun {
        int n = 0;
        const void *const *srcs = nullptr;
        void *const *dsts = nullptr;
        int rtPitch = 0;
        const DoviFrameState *dvFrames = nullptr;      // one RPU per frame: the frames of the run (null: the context's own RPU, if any)
        const DoviParams *dvTab = nullptr;             // ... and its tables on the device, DoviParams[n] then cm[12 n] (null: not uploaded, the run goes frame by frame)
        const float *dvCm = nullptr;
        bool started = false;                          // m_evStart is in place already (error diffusion: in front of the first chunk)
        bool usedTables = false;                       // out: a whole-batch route read dvTab / dvCm
        RunOn on;                                      // where the launches go: decided by PlaceBatch (until then: no stream)
        BatchRun Slice(int at, int m) const {          // the frames [at, at + m), every per-frame pointer advanced together
            BatchRun r = *this;
            r.n = m; r.srcs += at; r.dsts += at;
            if (dvFrames) r.dvFrames += at;
            if (dvTab) { r.dvTab += at; r.dvCm += (size_t)12 * at; }
            r.usedTables = false;
            return r;
        }
    };
    // A slot of a TableRing on loan: leaving scope records the slot's event on the stream the copy was queued on, that is
    // behind every launch queued there since, and the slot is rewritten only after that event.  Scope = the last launch that reads the slot.
    struct SlotLease {
        const void *dev = nullptr; hipEvent_t done = nullptr; hipStream_t stream = nullptr;
        SlotLease() = default;
        SlotLease(const void *d, hipEvent_t e, hipStream_t s) : dev(d), done(e), stream(s) {}
        SlotLease(SlotLease &&o) noexcept : dev(o.dev), done(o.done), stream(o.stream) { o.done = nullptr; }             // (move-only: copies are deleted with it)
        SlotLease &operator=(SlotLease &&o) noexcept { std::swap(dev, o.dev); std::swap(done, o.done); std::swap(stream, o.stream); return *this; }     // (what was here leaves with o)
        ~SlotLease() { if (done) (void)hipEventRecord(done, stream); }
        const FusedFrame *frames() const { return (const FusedFrame *)dev; }
    };
    // A ring of table slots, so that the host can queue several batches ahead: a slot is a pinned host copy, a device copy and the event
    // behind the last launch that reads the device copy (SlotLease).  The slots take turns; a table is filled, then sent
    class TableRing {
    public:
        TableRing(CHipVideoProcessor *owner, int slots) : m_owner(owner), m_slots((size_t)slots) {}
        // *pinned: the host copy of the slot whose turn it is, free to be rewritten (the host has waited for the launches behind its last lease; an
        // event never recorded counts as complete) and large enough for `bytes` (allocated for `atLeast` or more: batches of growing size do not reallocate one by one)
        HRESULT Next(size_t bytes, size_t atLeast, void **pinned);
        // its first `bytes` to the device on `stream` (`what` names the copy in an error); *lease: the device copy on loan.  The turn passes on
        HRESULT Send(size_t bytes, hipStream_t stream, const char *what, SlotLease *lease);
        // both around fill(Row *rows), which writes the table's n rows into the pinned copy: (const Row *)lease->dev is the table on the device
        template <class Row, class Fill>
        HRESULT SendRows(int n, hipStream_t stream, const char *what, SlotLease *lease, Fill fill)
        {
            Row *rows;
            if (HRESULT hr = Next(sizeof(Row) * n, sizeof(Row) * 64, (void **)&rows)) return hr;
            fill(rows);
            return Send(sizeof(Row) * n, stream, what, lease);
        }
        size_t Sent() const { return m_sent; }
        void Release();
    private:
        struct Slot { void *pinned = nullptr; size_t cap = 0; DevBuffer dev; hipEvent_t done = nullptr; };
        CHipVideoProcessor *m_owner;
        std::vector<Slot> m_slots;
        size_t m_sent = 0;             // tables sent so far: slot m_sent % slots is next
    };
    TableRing m_dvTableRing{this, 2};                 // the Dolby Vision tables of a run
    HRESULT UploadDoviTables(BatchRun *run, hipStream_t stream, SlotLease *lease);
    HRESULT ApplyDoviFrame(const DoviFrameState &f);
    std::string m_dvLastInfo;                         // the runs of the last batch call, if it was a ProcessBatchDovi (GetLastBatchInfo: ";dovi_runs=3:tables,1:frames")
    unsigned m_laneFrames = 0;                        // frames queued on the frame lanes (the timing pair is recorded on every n-th)
    unsigned m_launches = 0;                          // kernel launches so far (CheckHip) ...
    int m_lastBatchLane = -1;                                // the lane the last batch ran on (-1: the context stream)
    int m_lastBatchUploads = 0;                              // frame / plane tables the last batch call sent (a table of up to 32 frames travels in the exact-2x kernel's arguments: 0)
    int m_lastBatchFrames = 0, m_lastBatchLaunches = 0;      // ... and what the last batch call used
    int m_up2xForm = -1;                                     // the form of the last exact-2x launch since the last batch call began (FusedUp2xLastForm; -1: none)
    HRESULT CheckTargetLayout(int n, void *const *dsts, int rtPitch);
    // The record of a batch call (GetLastBatchInfo), open for as long as the call runs: every batch entry point starts with one, so a refused call reports an empty record
    struct BatchRecord {
        CHipVideoProcessor &vp; const unsigned launches; const size_t uploads;
        BatchRecord(CHipVideoProcessor &v, int frames) : vp(v), launches(v.m_launches), uploads(v.m_tableRing.Sent())
        {
            vp.m_lastBatchFrames = frames; vp.m_lastBatchLaunches = vp.m_lastBatchUploads = 0; vp.m_lastBatchLane = -1; vp.m_lastBatchWaits = 0;
            vp.m_dvLastInfo.clear(); vp.m_yuvLastInfo.clear(); vp.m_up2xForm = -1;
        }
        ~BatchRecord() { vp.m_lastBatchLaunches = (int)(vp.m_launches - launches); vp.m_lastBatchUploads = (int)(vp.m_tableRing.Sent() - uploads); }     // (what the call launched and sent up to its return)
    };
    HRESULT CheckBatchArgs(int n, const void *const *srcs, void *const *dsts, int rtPitch);     // what the RGB batch entry points check, before anything is applied or queued
    HRESULT RunBatch(BatchRun &run);                  // a validated batch: the plan, then error diffusion or the routes
    HRESULT ProcessBatchRoutes(BatchRun &run);
    bool ToneMapActive() const;

    // input
    const FmtConvParams *m_srcParams = nullptr;
    int m_srcWidth = 0, m_srcHeight = 0, m_srcPitch = 0, m_srcLines = 0;
    bool m_srcBottomUp = false;    // RGB DIB stored bottom-up (negative m_srcPitch in the reference)
    CRect m_srcRect;
    int m_srcRectWidth = 0, m_srcRectHeight = 0;
    ExtFmt m_decExFmt{0}, m_srcExFmt{0};
    CRect m_videoRect, m_windowRect;

    // constants (PS_COLOR_TRANSFORM, PS_PARAMETERS, matrix_conv_prim)
    float m_cm[12] = {0};
    float m_lumScale = 80.0f;
    float m_gamut[9] = {0};
    int m_tail = TAIL_NONE;
    float m_gamma = 1.0f;
    bool m_blobOverride = false;
    DevBuffer m_bcast;             // the blob in device memory while an RCCL broadcast is in flight
    bool m_bcastPending = false, m_bcastIsRoot = false;
    std::vector<unsigned char> m_bcastHost;      // host side of that copy: alive until BroadcastParamBlobEnd

    // plan
    bool m_planDirty = true;
    PassPlan m_plan;
    Up2xWeights m_upX{}, m_upY{};

    // device resources
    DevBuffer m_TexSrcVideo;       // uploaded sample (for v210: the Y210 texture CopyFrameV210 fills)
    DevBuffer m_TexRaw;            // v210 only: the raw sample before the unpack
    DevBuffer m_TexPost;           // m_TexsPostScale stand-in: input of the HDR10 tone-mapping step
    // upload ring (N3): pinned staging + device buffer per slot, copies on their own stream so that the upload of the
    // next sample overlaps the processing of the current one
    struct UploadSlot {
        void *pinned = nullptr; size_t pinnedSize = 0;
        DevBuffer dev;
        hipEvent_t uploaded = nullptr, consumed = nullptr;
        bool inFlight = false;         // an upload into this slot has been queued
        bool consumedRecorded = false; // a Process that read it has been queued after that upload
        hipStream_t consumedOn = nullptr;   // ... and `consumed` was last recorded on this stream (compared only, never used: MarkConsumed)
    };
    static constexpr int kUploadSlots = 3;
    UploadSlot m_up[kUploadSlots];
    int m_upNext = 0, m_curSlot = -1;
    hipStream_t m_copyStream = nullptr;
    void MarkConsumed();
    // What CopySample's host branches, CopySampleTensor and CopySampleFields share.  Acquire: the slot whose turn it is (*si), free to be rewritten
    // (the host has waited for the work that last used it), its device buffer of `bytes` or more.  Publish, once its new content is queued on
    // `recordedOn`: `uploaded` recorded there (another stream than the context's: that one waits for it), the slot current, its buffer the sample
    HRESULT AcquireUploadSlot(size_t bytes, int *si);
    HRESULT PublishUploadSlot(int si, hipStream_t recordedOn);
    const uint8_t *m_curSample = nullptr;   // device pointer of the current sample (own buffer or zero-copy)
    DevBuffer m_TexConvertOutput, m_TexResize, m_BackBuffer, m_Snapshot;
    int m_backW = 0, m_backH = 0, m_backFmt = 0;       // the last frame Render put into m_BackBuffer: size and format (GetDisplayedImage)
    DevBuffer m_dither;
    DevBuffer m_pqLut;             // kPqLutSize floats (fused path tone-map table)
    DevBuffer m_hlgLut;            // kPqLutSize floats: per-channel inverse HLG OETF (fused kernels' HLG -> SDR tail)
    DevBuffer m_eotfLut;           // kEotfLutSize + 1 floats: PQ EOTF (Dolby Vision block convert), uploaded with the first RPU
    float m_pqLutHost[kPqLutSize];
    bool m_pqLutValid = false;
    // the exact-2x kernel's table LDS image (BakeFusedTables, vp_launch.h), rebuilt by UpdatePlan from m_ditherHost and the plan's tone-map table
    DevBuffer m_fusedTab;
    std::vector<unsigned char> m_fusedTabHost;      // its host copy (GetFusedTables)
    std::vector<float> m_hlgLutHost;                // what m_hlgLut holds
    const float *m_fusedTabLut = nullptr;           // the device table its tone-map part was baked from (null: none)
    bool m_fusedTabValid = false;
    HRESULT UploadFusedTables();
    // The current plan's tables (vp_plan_tables.h), replaced whole by UpdatePlan, and their copies on the device: one buffer per axis
    // pack and m_stripTab.  m_tapsX / m_tapsY / m_otherX / m_otherY are views of those copies: null where the plan has no such table
    PlanTables m_tables;
    DevBuffer m_axisX, m_axisY;
    AxisTaps m_tapsX{}, m_tapsY{};
    const int32_t *m_otherX = nullptr, *m_otherY = nullptr;
    // (eight slots: a chunk of mpcvr_process_batch_yuv takes up to two, its frames' and its planes' — the host queues four such chunks before it waits for the first)
    TableRing m_tableRing{this, 8};        // the frame tables of mpcvr_process_batch and the plane tables of mpcvr_process_batch_yuv (GetLastBatchInfo's uploads=)
    uint16_t m_ditherHost[1024];
    // Frames and whole batches of a context that owns its stream overlap on the frame lanes (vp_lanes.h: the streams, what is in flight on
    // them and what orders it).  What may take a lane is decided here, from the plan: FrameLanesUsable for frames, BatchLaneEligible for batches
    FrameLanes m_lanes;
    int m_lastBatchWaits = 0;                 // writers still in flight on other lanes the last batch was ordered behind (GetLastBatchInfo)
    hipStream_t m_lastRun = nullptr;          // the stream the current sample's last Process ran on (MarkConsumed records there)
    bool FrameLanesUsable() const;
    // what a frame written through `rt` covers (RtSpan, vp_spans.h): the window's rows at this pitch
    RtSpan TargetSpan(const void *rt, int rtPitch) const { return RowsSpan(rt, (size_t)rtPitch, m_windowRect.Height(), (size_t)m_windowRect.Width() * 4); }
    // host_wait: block until the lanes are idle; otherwise the context stream waits for them (work queued on it afterwards runs behind
    // every frame in flight)
    HRESULT JoinFrameLanes(bool host_wait) { return CheckHip(m_lanes.Join(host_wait, m_stream), "frame lane sync"); }
    // work is about to be queued on the context stream: behind whatever the lanes hold, and what the lanes are given next behind it (LaneWaitsForStream)
    void OrderOnContextStream() { (void)JoinFrameLanes(false); m_lanes.NoteStreamWork(); }
    size_t m_convBytes = 0, m_midBytes = 0, m_postBytes = 0;
    // whole-batch launches of the pass-per-kernel path (block convert + folded resize kernels with a frame dimension)
    DevBuffer m_batchConv, m_batchMid;
    DevBuffer m_batchPost;         // HDR10 tone-mapping step of a batch: the frames' m_TexsPostScale copies side by side
    // EXTENSION (bUseDither = 2, m_plan.errdiff): the frames as a 10-bit swap chain would receive them, window geometry, side by side;
    // the error-diffusion pass (vp_errdiff.hip) reads them and writes the real render targets
    DevBuffer m_edPost;
    DevBuffer m_edHandoff;         // the pass's hand-off rows between bands of 64 rows (vp_errdiff.hip)
    struct EdLayout {              // what the hand-off rows of the last pass were laid out for (ErrDiffPass): compared field by field
        int x0 = 0, x1 = 0, y0 = 0, y1 = 0, n = 0; const void *rows = nullptr;
        bool operator==(const EdLayout &o) const { return x0 == o.x0 && x1 == o.x1 && y0 == o.y0 && y1 == o.y1 && n == o.n && rows == o.rows; }
    };
    int m_edGen = 0; EdLayout m_edKey;       // generation of the hand-off words of the last pass, and the layout they belong to
    int m_edPatience = 0;          // SetErrorDiffusionPatience: polls per group before a band gives up (0: the launcher's default)
    int *m_edStatus = nullptr;     // pinned host word the pass sets when a band gave up waiting (checked at the next pass and in Synchronize)
    uint8_t *m_edBase = nullptr;   // first intermediate (m_edPost.ptr + a margin)
    int m_edPitch = 0;             // bytes per row of an intermediate (a multiple of 256)
    size_t m_edStride = 0;         // bytes per intermediate
    HRESULT PrepareErrDiff(int frames);
    HRESULT ErrDiffPass(const LaunchFrames &frames, int rtPitch, hipStream_t s);
    HRESULT ProcessBatchErrDiff(BatchRun &run);
    size_t PostStride() const { return (m_postBytes + 255) & ~(size_t)255; }
    // a frame table in a slot of the ring (pinned copy + device copy): frame i = {srcs ? srcs[i] : null, dsts ? dsts[i] : dst_base + i * dst_stride}
    HRESULT UploadFrameTable(int n, const void *const *srcs, void *const *dsts, uint8_t *dst_base, size_t dst_stride, hipStream_t stream, SlotLease *lease);
    // the frames {srcs[i], dsts[i]} of a launch that takes byValueMax rows in its arguments: in `rows` (kHostTableMax of them), or uploaded (*lease)
    HRESULT BatchFrames(int n, const void *const *srcs, void *const *dsts, int byValueMax, hipStream_t stream, FusedFrame *rows, SlotLease *lease, LaunchFrames *frames);
    DevBuffer m_batchTex;          // interleaved RGB / v210 batches: the frames' m_TexSrcVideo copies side by side (ProcessBatch)
    bool m_texSrcZeroed = false, m_batchTexZeroed = false;     // the texels the RGB copy loops never write have been cleared for the current media type
    // Jinc2m phase tables of the first / second draw (null: weights per pixel)
    DevBuffer m_jincFirst, m_jincSecond, m_jincFused;
    const float *m_jincFusedTab = nullptr;                                  // the fused Jinc2m kernel's weight table (BuildFusedJincTable), PassPlan::fused_jinc
    const void *m_jincFirstTab = nullptr, *m_jincSecondTab = nullptr;
    const float *m_jincFirstCtr = nullptr, *m_jincSecondCtr = nullptr;     // the plain kernel's texcoord tables (no phase table: BuildDrawCentres), in the same buffers
    HRESULT UploadJincPhases(const DrawCoords &dc, DevBuffer &buf, const void **tab, const float **ctr);
    // arbitrary-ratio fused kernel (vp_fused_strip.hip): geometry planned with the tap tables (UpdatePlan)
    bool m_strip = false;          // raw 4:2:0 sample -> render target in one kernel
    bool m_stripSurf = false;      // any other source: the convert kernel's output (or the RGB source texture) -> render target through the same kernel, no convert stage
    bool FillStripSurfParams(const Surface &src, const StoreParams &store, FusedStripParams *sp) const;
    DevBuffer m_stripTab;          // m_tables.stripPack on the device
    bool FillStripParams(const uint8_t *sample, void *dst, int dstPitch, const StoreParams &store, FusedStripParams *sp, int inflight = 1) const;
    bool FillStripTables(const StoreParams &store, int perForce, FusedStripParams *sp) const;     // what the two above share
    // periodic-phase variant of the same launch (vp_fused_period.h): vertical ratio 4:3 / 3:2 / 2:3 / 1:2 / 3:1, tables behind the strip kernel's in m_stripTab (m_tables.period)
    mutable int m_stripRan = -1;   // which kernel the last strip launch of this plan really ran (1 = k_fused_period, 0 = k_fused_strip, -1 = none yet): the plan-time
                                   // probe uses a null, aligned target — a real target with an odd pitch or offset sends the launch to k_fused_strip (GetPathInfo reports what ran)
    mutable bool m_fusedAside = false;   // the last frame / batch of this plan went past the fused kernel the plan names (exact-2x, strip / periodic): a condition
                                   // asked per call failed — StoreRowsFit32 for the exact-2x kernels; for the strip kernels whatever FillStripParams /
                                   // FillStripSurfParams refuse with this call's target (rows that span 4 GiB, the LDS the launch would need) — and the
                                   // convert kernel + resize draws ran (GetPathInfo reports what ran)
    bool m_period = false;         // the planned launch (window-sized target) takes the periodic kernel: what GetVPInfo reports
    // the route of a mpcvr_process_batch call, in order of precedence (ClassifyBatch), and what its launches need
    enum class BatchRoute { DirectConvert, RgbSurfaceStrip, StripToneMap, FrameByFrame, WholeBatchLaunches, Strip, FusedUp2x };
    struct BatchRoutePlan {
        BatchRoute route = BatchRoute::FrameByFrame;
        size_t repackSlot = 0;         // v210: the samples are repacked first, into slots of m_batchTex of this many bytes (256-byte aligned); 0: not
        bool aligned = true, aligned8 = true, src16 = true, src4 = true;   // every render target on a 16- / 8-byte boundary; every sample the launches read on a 16- / 4-byte one
        FusedStripParams strip{};      // RgbSurfaceStrip / StripToneMap / Strip (surface / post-scale pointers: set by RunBatchRoute)
        FusedParams conv{}, direct{};  // WholeBatchLaunches / DirectConvert (BatchPlan)
    };
    BatchRoutePlan ClassifyBatch(const BatchRun &run) const;
    // may a batch of this route run on a batch lane beside the one before it?
    bool BatchLaneEligible(const BatchRoutePlan &rp, const BatchRun &run) const;
    // where a classified batch runs and what it is ordered behind; `writes`: the spans it writes for the caller.  Sets run.on; returns the lane (-1: none)
    int PlaceBatch(const BatchRoutePlan &rp, BatchRun &run, std::vector<RtSpan> &&writes);
    void NoteBatchQueued(int lane) { if (lane >= 0) m_lanes.NoteLaneBatch(lane); }      // the batch PlaceBatch placed has been queued
    // mpcvr_process_batch_yuv: one RGB surface per batch lane (a lane's chunks write, read and reuse its surface in stream order); chunks on
    // the context stream use the first (they run behind everything the lanes hold, and the lanes' next work behind them)
    struct YuvSurface {
        DevBuffer buf;
        CRect window, video;           // what it was last cleared for (the letterbox is never written by Process)
        bool cleared = false;
    };
    YuvSurface m_yuvSurf[FrameLanes::kFrameLanes];
    size_t m_yuvBudget = 0;            // SetBatchYuvBudget; 0: kBatchYuvDefaultBudget
    std::string m_yuvLastInfo;         // ";yuv_chunks=..;yuv_lanes=.." (";tensor_chunks=..;tensor_lanes=..", ";lut3d_chunks=..;lut3d_lanes=..;lut3d_table=..", ";deband_chunks=..;deband_lanes=..;deband_taps=..", ";sharpen_chunks=..;sharpen_lanes=..") of the last batch call, if it was a ProcessBatchYuv (ProcessBatchTensor, ProcessBatchLut3d, ProcessBatchDeband, ProcessBatchSharpen)
    DevBuffer m_sampleSurf;            // ProcessBatchFromTensors / ProcessBatchDeint: the samples of one chunk side by side (PlanBatchSamples), written and read in stream order on the context stream
    // the chunk loop of ProcessBatchYuv / ProcessBatchTensor: surfaces, lanes and order; writesOf(at, m): what the chunk writes for the caller, pass(run, at): its pass
    template <class WritesOf, class Pass>
    HRESULT RunSurfaceChunks(int n, const void *const *srcs, const BatchYuvLayout &lay, const char *tag, WritesOf writesOf, Pass pass);
    // its mirror, the chunk loop of ProcessBatchFromTensors / ProcessBatchDeint: pass(at, m, samples, stream) writes the chunk's samples into m_sampleSurf
    template <class Pass>
    HRESULT RunSampleChunks(int n, const ChunkLayout &lay, void *const *dsts, int rtPitch, const char *tag, Pass pass);
    // one chunk into its surface: rp / run.dsts name the surface's frames, run.on the stream
    HRESULT RenderChunk(BatchRoutePlan &rp, BatchRun &run, YuvSurface &surf);
    // ... and its passes behind it: `encode` holds the launch's pitches, size and coefficients
    HRESULT EncodeChunk(BatchRun &run, const EncodeParams &encode, const EncodePlan &plan, void *const *yPlanes, void *const *uvPlanes, uint32_t *histRows);
    // video rect ∩ window: the active picture the measure pass counts (empty: all zero)
    mpcvr_rect ActiveRect() const;
    HRESULT RunBatchRoute(BatchRoutePlan &rp, BatchRun &run);
    bool BatchPlan(const uint8_t *sample0, void *rt0, int rtPitch, bool aligned, bool repacked, bool src16, FusedParams *conv, FusedParams *direct) const;
    HRESULT ProcessBatchLaunches(const BatchRun &run, const FusedFrame *table, bool aligned, FusedParams conv);
};

}  // namespace mpcvr
