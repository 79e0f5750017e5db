// hip_video_processor.cpp — pass sequencing and resource management of the shader video processor on
// HIP.  Restates the control flow of CDX11VideoProcessor::{InitMediaType, Configure, CopySample,
// Process, ConvertColorPass, ResizeShaderPass, FinalPass, GetCurentImage}
// (Source/DX11VideoProcessor.cpp) without the D3D11 plumbing; the batch machinery is here as well.  The calls without a
// counterpart in the reference (the EXTENSIONS of include/mpcvr.h) are in hip_video_processor_ext.cpp.
#include "hip_video_processor.h"

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cstdlib>

#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstring>

namespace mpcvr {

static const uint16_t kDitherTable[1024] = {
#include "dither_table.inc"
};

// parameter blob exchanged between ranks (mpcvr_get/set_param_blob)
struct ParamBlob {
    uint32_t magic;          // 'MPVB'
    uint32_t version;
    float cm[12];
    float lum_scale;
    float gamut[9];
    int32_t tail;
    float gamma;
    Up2xWeights upx, upy;
    uint16_t dither[1024];
    float pq_lut[kPqLutSize];      // tone-map LUT (valid when tail == PQ->SDR)
};
static const uint32_t kBlobMagic = 0x4256504du;

// ------------------------------------------------------------------------------------------------
hipError_t DevBuffer::CheckCreate(size_t bytes)
{
    if (bytes <= size && ptr) return hipSuccess;
    Release();
    hipError_t e = hipMalloc(&ptr, bytes);
    if (e == hipSuccess) size = bytes; else ptr = nullptr;
    return e;
}
void DevBuffer::Release()
{
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr; size = 0;
}

CHipVideoProcessor::CHipVideoProcessor() { std::memcpy(m_ditherHost, kDitherTable, sizeof(m_ditherHost)); }

CHipVideoProcessor::~CHipVideoProcessor()
{
    // runs after a failed Init as well (the stream / events / dither buffer may exist already): every handle below is guarded
    if (!m_bInit && !m_stream && !m_evStart && !m_evStop && !m_dither.ptr) return;
    (void)hipSetDevice(m_device);
    if (m_stream) (void)hipStreamSynchronize(m_stream);
    for (DevBuffer *b : {&m_batchConv, &m_batchMid, &m_batchPost, &m_edPost, &m_edHandoff, &m_batchTex, &m_jincFirst, &m_jincSecond, &m_jincFused, &m_TexSrcVideo, &m_TexRaw, &m_TexPost, &m_TexConvertOutput, &m_TexResize, &m_BackBuffer, &m_Snapshot, &m_dither,
                         &m_pqLut, &m_hlgLut, &m_eotfLut, &m_stripTab, &m_axisX, &m_axisY})
        b->Release();
    for (YuvSurface &ys : m_yuvSurf) ys.buf.Release();
    m_sampleSurf.Release();
    for (UploadSlot &u : m_up) {
        u.dev.Release();
        if (u.pinned) (void)hipHostFree(u.pinned);
        if (u.uploaded) (void)hipEventDestroy(u.uploaded);
        if (u.consumed) (void)hipEventDestroy(u.consumed);
    }
    if (m_edStatus) (void)hipHostFree(m_edStatus);
    if (m_copyStream) (void)hipStreamDestroy(m_copyStream);
    m_doviDev.Release();
    m_bcast.Release();
    for (DoviSlot &d : m_doviSlots) {
        if (d.pinned) (void)hipHostFree(d.pinned);
        if (d.copied) (void)hipEventDestroy(d.copied);
    }
    m_dvTableRing.Release();
    m_lanes.Release();
    m_tableRing.Release();
    if (m_evStart) (void)hipEventDestroy(m_evStart);
    if (m_evStop) (void)hipEventDestroy(m_evStop);
    for (hipEvent_t *e : {&m_evUp0, &m_evUp1, &m_evRb0, &m_evRb1}) { if (*e) (void)hipEventDestroy(*e); *e = nullptr; }
    if (m_ownStream && m_stream) (void)hipStreamDestroy(m_stream);
}

// MPCVR_LOG=1: failures (and, =2, every plan the context settles on) go to stderr as well — the stand-in for the reference's
// DLog() lines (Utils/Util.h); mpcvr_last_error carries the same text to the caller either way.
static int LogLevel()
{
    static const int lvl = [] { const char *e = std::getenv("MPCVR_LOG"); return e && *e ? std::atoi(e) : 0; }();
    return lvl;
}

HRESULT CHipVideoProcessor::Fail(HRESULT hr, const std::string &msg)
{
    m_lastError = msg;
    if (LogLevel() >= 1) std::fprintf(stderr, "mpcvr[%p]: error 0x%08x: %s\n", (void *)this, (unsigned)hr, msg.c_str());
    return hr;
}

HRESULT CHipVideoProcessor::CheckHip(hipError_t e, const char *what)
{
    if (what[0] == 'k' && what[1] == '_') m_launches++;        // (kernel launches are checked under their kernel's name: GetLastBatchInfo counts them)
    if (e == hipSuccess) return MPCVR_S_OK;
    return Fail(e == hipErrorOutOfMemory ? MPCVR_E_OUTOFMEMORY : MPCVR_E_FAIL,
                std::string(what) + ": " + hipGetErrorString(e));
}

static bool ValidSettings(const mpcvr_settings &s, std::string *why)
{
    auto bad = [&](const char *m) { *why = m; return false; };
    if (s.iTexFormat != MPCVR_TEXFMT_AUTOINT && s.iTexFormat != MPCVR_TEXFMT_8INT &&
        s.iTexFormat != MPCVR_TEXFMT_10INT && s.iTexFormat != MPCVR_TEXFMT_16FLOAT) return bad("iTexFormat");
    if (s.iChromaScaling < 0 || s.iChromaScaling > MPCVR_CHROMA_CatmullRom) return bad("iChromaScaling");
    if (s.iUpscaling < 0 || s.iUpscaling > MPCVR_UPSCALE_Spline36_EXT) return bad("iUpscaling");
    if (s.iDownscaling < 0 || s.iDownscaling > MPCVR_DOWNSCALE_Lanczos) return bad("iDownscaling");
    if (s.iSDRDisplayNits < 25 || s.iSDRDisplayNits > 400) return bad("iSDRDisplayNits");   // IVideoRenderer.h:87-90
    if (s.output_format != MPCVR_OUT_BGRA8 && s.output_format != MPCVR_OUT_RGB10A2) return bad("output_format");
    if (s.bUseDither < 0 || s.bUseDither > MPCVR_DITHER_ErrorDiffusion_EXT) return bad("bUseDither");
    return true;
}

HRESULT CHipVideoProcessor::Init(int device, const mpcvr_settings &settings)
{
    std::string why;
    if (!ValidSettings(settings, &why)) return Fail(MPCVR_E_INVALIDARG, "invalid settings: " + why);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return Fail(MPCVR_E_FAIL, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device < 0 || device >= count) return Fail(MPCVR_E_INVALIDARG, "device ordinal out of range");
    m_device = device;
    HRESULT hr;
    if ((hr = CheckHip(hipSetDevice(device), "hipSetDevice"))) return hr;
    // the context's own stream is a BLOCKING stream: it orders itself against the legacy null stream, so a caller that
    // prepares samples / render targets on stream 0 (torch's default stream) and never hands over a stream is still ordered
    if ((hr = CheckHip(hipStreamCreateWithFlags(&m_stream, hipStreamDefault), "hipStreamCreate"))) return hr;
    m_ownStream = true;
    if ((hr = CheckHip(hipEventCreate(&m_evStart), "hipEventCreate"))) return hr;
    if ((hr = CheckHip(hipEventCreate(&m_evStop), "hipEventCreate"))) return hr;
    // dither texture load — DX11VideoProcessor.cpp:1414-1440
    if ((hr = CheckHip(m_dither.CheckCreate(sizeof(m_ditherHost)), "dither alloc"))) return hr;
    if ((hr = CheckHip(hipMemcpy(m_dither.ptr, m_ditherHost, sizeof(m_ditherHost), hipMemcpyHostToDevice), "dither upload"))) return hr;
    m_cfg = settings;
    m_bInit = true;
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::SetStream(hipStream_t s)
{
    if (!m_bInit) return Fail(MPCVR_E_NOT_VALID_STATE, "not initialised");
    (void)hipSetDevice(m_device);
    (void)JoinFrameLanes(true);
    if (m_stream) (void)hipStreamSynchronize(m_stream);
    if (m_ownStream && m_stream) (void)hipStreamDestroy(m_stream);
    m_ownStream = false;
    m_stream = s;
    if (!s) {
        // NULL (which is also the handle of the legacy default stream) = the context's own BLOCKING stream, see Init
        HRESULT hr = CheckHip(hipStreamCreateWithFlags(&m_stream, hipStreamDefault), "hipStreamCreate");
        if (hr) return hr;
        m_ownStream = true;
    }
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::Synchronize()
{
    if (!m_bInit) return Fail(MPCVR_E_NOT_VALID_STATE, "not initialised");
    (void)hipSetDevice(m_device);
    HRESULT hr = JoinFrameLanes(true);
    if (hr) return hr;
    if ((hr = CheckHip(hipStreamSynchronize(m_stream), "hipStreamSynchronize"))) return hr;
    if (m_edStatus && *m_edStatus) { *m_edStatus = 0; return Fail(MPCVR_E_FAIL, "error diffusion: a band gave up waiting for the band above"); }
    return MPCVR_S_OK;
}

// ---- frame lanes (vp_lanes.h): what may take one ----
// A frame may run beside its predecessor when nothing it touches is shared with it: the context owns its stream (a caller's stream
// promises stream order), the sample is read in place (no repack / copy into m_TexSrcVideo), no per-frame constants are uploaded on
// the context stream (Dolby Vision), and the plan has no intermediate surface (one fused kernel per frame: exact 2x, the strip /
// periodic kernel without the HDR10 tone-mapping step, the same-size block convert).
bool CHipVideoProcessor::FrameLanesUsable() const
{
    static const bool off = [] { const char *e = std::getenv("MPCVR_NO_FRAME_LANES"); return e && *e && *e != '0'; }();
    if (off || !m_ownStream || (m_cfg.flags & MPCVR_FLAG_NO_FRAME_LANES) || m_doviValid || !m_srcParams) return false;
    if (m_srcParams->cformat == MPCVR_CF_V210 || m_srcParams->layout == LAY_RGB || ((uintptr_t)m_curSample & 3) != 0) return false;
    // (the error-diffusion pass reads the context's one intermediate)
    return !m_plan.errdiff && (m_plan.fused_up2x || (m_strip && !m_plan.hdr_tonemap) || m_plan.direct_convert);
}

// ------------------------------------------------------------------------------------------------
// InitMediaType — DX11VideoProcessor.cpp:1742-1959 (shader-path half: InitializeTexVP :2018-2047)
// ------------------------------------------------------------------------------------------------
HRESULT CHipVideoProcessor::InitMediaType(int cformat, int width, int height, int pitch, const CRect *srcRect, uint32_t extfmt)
{
    if (!m_bInit) return Fail(MPCVR_E_NOT_VALID_STATE, "not initialised");
    const FmtConvParams *f = GetFmtConvParams(cformat);
    if (!f) return Fail(MPCVR_E_NOTIMPL, "colour format not supported by this build");
    if (width <= 0 || height <= 0 || width > 16384 || height > 16384) return Fail(MPCVR_E_INVALIDARG, "bad frame size");
    if ((f->div_w == 2 && (width & 1)) || (f->div_h == 2 && (height & 1)))
        return Fail(MPCVR_E_INVALIDARG, "subsampled formats need even dimensions");
    const int defPitch = DefaultPitch(*f, width);
    if (pitch == 0) pitch = defPitch;
    // a bottom-up RGB DIB arrives with a negative pitch (BI_RGB && biHeight > 0 => m_srcPitch = -m_srcPitch, :1801-1803)
    bool bottomUp = false;
    if (pitch < 0) {
        if (f->layout != LAY_RGB) return Fail(MPCVR_E_INVALIDARG, "a negative pitch (bottom-up) is only defined for the RGB formats");
        bottomUp = true; pitch = -pitch;
    }
    if (pitch < width * f->Packsize) return Fail(MPCVR_E_INVALIDARG, "pitch smaller than a row");
    if (f->cformat == MPCVR_CF_V210 && (pitch < (width + 5) / 6 * 16 || (pitch & 3)))
        return Fail(MPCVR_E_INVALIDARG, "v210 pitch smaller than a row of 16-byte groups");
    if (f->bytes == 2 && (pitch & 1)) return Fail(MPCVR_E_INVALIDARG, "16-bit formats need an even pitch");
    if (f->bytes == 4 && (pitch & 3)) return Fail(MPCVR_E_INVALIDARG, "32-bit texels need a pitch that is a multiple of 4");
    // the chroma planes of a three-plane format lie at pitch / div_w (MemCopyToTexSrcVideo :1230-1241): 16-bit samples there need that pitch even as well
    if (f->planes == 3 && f->bytes == 2 && ((pitch / f->div_w) & 1))
        return Fail(MPCVR_E_INVALIDARG, "three-plane 16-bit formats need an even chroma pitch (pitch / 2): a luma pitch that is a multiple of 4");
    CRect r = srcRect ? *srcRect : CRect();
    if (r.IsRectNull()) r = CRect(0, 0, width, height);                        // :1821-1823
    if (r.left < 0 || r.top < 0 || r.right > width || r.bottom > height || r.Width() <= 0 || r.Height() <= 0)
        return Fail(MPCVR_E_INVALIDARG, "source rect outside the frame");

    m_srcParams = f;
    m_srcWidth = width; m_srcHeight = height;
    m_srcPitch = pitch;
    m_srcBottomUp = bottomUp;
    m_srcLines = SourceLines(*f, height);
    m_srcRect = r;
    m_srcRectWidth = r.Width(); m_srcRectHeight = r.Height();
    m_decExFmt.value = extfmt;
    m_srcExFmt = SpecifyExtendedFormat(m_decExFmt, *f, m_srcRectWidth, m_srcRectHeight);   // :1827
    m_blobOverride = false;
    if (m_videoRect.IsRectNull()) m_videoRect = CRect(0, 0, m_srcRectWidth, m_srcRectHeight);
    if (m_windowRect.IsRectNull()) m_windowRect = CRect(0, 0, m_videoRect.right, m_videoRect.bottom);
    SetShaderConvertColorParams();
    SetShaderLuminanceParams();
    m_curSample = nullptr;
    m_planDirty = true;
    m_texSrcZeroed = m_batchTexZeroed = false;      // another format / size: the RGB48 remainder texels must be cleared again
    return MPCVR_S_OK;
}

void CHipVideoProcessor::SetShaderConvertColorParams()
{
    if (!m_srcParams || m_blobOverride) return;
    if (m_doviValid) DoviColorMatrix(m_doviMd, *m_srcParams, m_procAmp, m_cm);     // :817-834
    else ComputeColorMatrix(m_srcExFmt, *m_srcParams, m_procAmp, m_cm);
    ComputeGamut2020to709(m_gamut);
    SelectTail(m_srcExFmt, m_cfg.bConvertToSdr != 0, &m_tail, &m_gamma, m_hdrOutput, m_doviValid);
}

void CHipVideoProcessor::SetShaderLuminanceParams()
{
    if (m_blobOverride) return;
    m_lumScale = 10000.0f / m_cfg.iSDRDisplayNits;                              // :891
}

HRESULT CHipVideoProcessor::SetVideoRect(const CRect &r)
{
    if (r.Width() <= 0 || r.Height() <= 0) return Fail(MPCVR_E_INVALIDARG, "empty video rect");
    if (r != m_videoRect) { m_videoRect = r; m_planDirty = true; }
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::SetWindowRect(const CRect &r)
{
    if (r.Width() <= 0 || r.Height() <= 0) return Fail(MPCVR_E_INVALIDARG, "empty window rect");
    const CRect w(0, 0, r.Width(), r.Height());
    if (w != m_windowRect) { m_windowRect = w; m_planDirty = true; }
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::SetRotation(int value)
{
    if (value != 0 && value != 90 && value != 180 && value != 270) return Fail(MPCVR_E_INVALIDARG, "rotation must be 0, 90, 180 or 270");
    if (value != m_iRotation) { m_iRotation = value; m_planDirty = true; }
    return MPCVR_S_OK;
}

// HDR output: stands in for m_bHdrPassthroughSupport && (m_bHdrPassthrough || m_bHdrLocalToneMapping) — the display is in
// HDR10 mode, so HDR sources are not converted to SDR (convertType :2948-2950) — plus m_bHdrLocalToneMapping /
// m_iHdrLocalToneMappingType / m_iHdrDisplayMaxNits
HRESULT CHipVideoProcessor::SetHdrOutput(bool enable, int toneMapType, float displayMaxNits)
{
    if (toneMapType < 0 || toneMapType > 6) return Fail(MPCVR_E_INVALIDARG, "tone mapping type must be 0 (off) .. 6");
    m_hdrOutput = enable; m_hdrToneMapType = toneMapType; m_hdrDisplayMaxNits = displayMaxNits;
    UpdateHdrToneMapParams();
    m_blobOverride = false;
    SetShaderConvertColorParams();
    m_planDirty = true;
    if (m_doviValid) {          // the level-2 selection depends on the display peak (:2384)
        const mpcvr_dovi_metadata md = m_doviMd;
        return SetDoviMetadata(&md);
    }
    return MPCVR_S_OK;
}

// the HDR10 metadata Render() hands to SetHDR10ShaderParams (:2716-2727): mastering min/max luminance, MaxCLL, MaxFALL
HRESULT CHipVideoProcessor::SetHdrMetadata(float minMastering, float maxMastering, float maxCLL, float maxFALL)
{
    m_hdrMeta[0] = minMastering; m_hdrMeta[1] = maxMastering; m_hdrMeta[2] = maxCLL; m_hdrMeta[3] = maxFALL;
    m_hdrMetaValid = true;
    UpdateHdrToneMapParams();
    m_planDirty = true;
    return MPCVR_S_OK;
}

// SetHDR10ShaderParams — DX11VideoProcessor.cpp:907-917
void CHipVideoProcessor::UpdateHdrToneMapParams()
{
    HdrToneMapParams k{m_hdrMeta[0], m_hdrMeta[1], m_hdrMeta[2], m_hdrMeta[3], m_hdrDisplayMaxNits, m_hdrToneMapType};
    if (m_doviValid && m_doviL1Present) {       // Render :2716-2720: L1 min, max, max, avg; BT.2390 -> ST 2094-10
        k.min_mastering = (float)m_doviL1[0]; k.max_mastering = (float)m_doviL1[1];
        k.max_cll = (float)m_doviL1[1]; k.max_fall = (float)m_doviL1[2];
        if (k.selection == 5) k.selection = 6;
    }
    k.l2_enabled = (m_doviValid && m_doviL2Present) ? 1 : 0;      // m_pDoViDynamicConstants at b1 (:3362-3364)
    std::memcpy(k.l2k, m_doviL2Raw, sizeof(k.l2k));
    SanitiseHdr10Params(&k);
    m_hdrTm = k;
}

// m_pPSHDR10ToneMapping exists once an HDR10/HLG source is shown in HDR with local tone mapping on and metadata known
bool CHipVideoProcessor::ToneMapActive() const
{
    const unsigned tf = m_srcExFmt.VideoTransferFunction();
    if (m_doviValid) return m_hdrOutput && m_hdrToneMapType > 0 && (m_hdrMetaValid || m_doviL1Present);     // SourceIsHDR()
    return m_hdrOutput && m_hdrToneMapType > 0 && m_hdrMetaValid && (tf == 15 || tf == 16);
}

// CopySample, IID_MediaSideDataDOVIMetadataV2 branch — DX11VideoProcessor.cpp:2270-2520
HRESULT CHipVideoProcessor::SetDoviMetadata(const mpcvr_dovi_metadata *md)
{
    const HRESULT hr = ApplyDoviMetadata(md);
    return (hr || !md) ? hr : UploadDoviParams();
}

// the host side of an RPU: curves, matrices, trims, what the plan depends on — everything but the copy to the device
HRESULT CHipVideoProcessor::ApplyDoviMetadata(const mpcvr_dovi_metadata *md)
{
    if (!m_bInit) return Fail(MPCVR_E_NOT_VALID_STATE, "not initialised");
    if (!md) {
        if (m_doviValid) { m_doviValid = false; m_planDirty = true; }
        m_doviL1Present = m_doviL2Present = false;
        m_blobOverride = false;
        SetShaderConvertColorParams();
        UpdateHdrToneMapParams();
        return MPCVR_S_OK;
    }
    if (!CheckDoviCurves(*md)) return Fail(MPCVR_E_INVALIDARG, "Dolby Vision curves: num_pivots outside [2,9], mapping_idc > 1 or more than 32 level-2 blocks");
    const bool wasValid = m_doviValid, hadToneMap = m_srcParams && ToneMapActive();
    m_doviMd = *md;
    m_doviValid = true;
    uint32_t l1[3];
    if (DoviL1Nits(*md, l1)) { m_doviL1Present = true; std::memcpy(m_doviL1, l1, sizeof(l1)); }
    float k[5];
    if (DoviL2Constants(*md, (int)m_hdrDisplayMaxNits, k)) { m_doviL2Present = true; std::memcpy(m_doviL2Raw, k, sizeof(k)); }
    else if (!m_doviL2Present) std::memcpy(m_doviL2Raw, k, sizeof(k));       // the cbuffer of an absent L2 (:956-960)
    PackDoviCurves(*md, &m_doviHost);
    DoviLmsMatrix(*md, m_doviHost.lms);
    m_doviHost.l2_enabled = m_doviL2Present ? 1 : 0;
    std::memcpy(m_doviHost.l2k, m_doviL2Raw, sizeof(m_doviHost.l2k));
    m_blobOverride = false;
    SetShaderConvertColorParams();
    UpdateHdrToneMapParams();
    if (!wasValid || (m_srcParams && hadToneMap != ToneMapActive())) m_planDirty = true;
    return MPCVR_S_OK;
}

// the curve / trim constant buffers travel through a small pinned ring so per-frame RPUs never stall the stream
HRESULT CHipVideoProcessor::UploadDoviParams()
{
    (void)hipSetDevice(m_device);
    HRESULT hr;
    if ((hr = CheckHip(m_doviDev.CheckCreate(sizeof(DoviParams)), "dovi constants"))) return hr;
    if (!m_eotfLut.ptr) {           // the PQ EOTF table of the block convert's Dolby Vision variants: a constant of the transfer function
        std::vector<float> lut(kPqEncOffset + kPqEncSize + 1, 0.0f);      // the EOTF table, then (16-byte aligned) the PQ encode table of the level-2 variant
        BuildPqEotfLut(lut.data());
        BuildPqEncodeLut(lut.data() + kPqEncOffset);
        if ((hr = CheckHip(m_eotfLut.CheckCreate(lut.size() * sizeof(float)), "pq eotf lut"))) return hr;
        if ((hr = CheckHip(hipMemcpy(m_eotfLut.ptr, lut.data(), lut.size() * sizeof(float), hipMemcpyHostToDevice), "pq eotf lut upload"))) return hr;
    }
    DoviSlot &slot = m_doviSlots[m_doviSlotNext++ % 4];
    if (!slot.pinned) {
        if ((hr = CheckHip(hipHostMalloc((void **)&slot.pinned, sizeof(DoviParams), hipHostMallocDefault), "dovi staging"))) return hr;
        if ((hr = CheckHip(hipEventCreateWithFlags(&slot.copied, hipEventDisableTiming), "dovi event"))) return hr;
    } else if ((hr = CheckHip(hipEventSynchronize(slot.copied), "dovi staging wait"))) return hr;
    *slot.pinned = m_doviHost;
    if ((hr = CheckHip(hipMemcpyAsync(m_doviDev.ptr, slot.pinned, sizeof(DoviParams), hipMemcpyHostToDevice, m_stream), "dovi upload"))) return hr;
    return CheckHip(hipEventRecord(slot.copied, m_stream), "dovi event record");
}

HRESULT CHipVideoProcessor::SetSampleFormat(int frameFormat)
{
    if (frameFormat < 0 || frameFormat > 2) return Fail(MPCVR_E_INVALIDARG, "frame format must be 0 (progressive), 1 (TFF) or 2 (BFF)");
    if (frameFormat != m_SampleFormat) { m_SampleFormat = frameFormat; m_planDirty = true; }
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::SetFlip(bool value)
{
    if (value != m_bFlip) { m_bFlip = value; m_planDirty = true; }
    return MPCVR_S_OK;
}

// Configure — DX11VideoProcessor.cpp:3800-4050: diff, then rebuild only what changed
HRESULT CHipVideoProcessor::Configure(const mpcvr_settings &c)
{
    if (!m_bInit) return Fail(MPCVR_E_NOT_VALID_STATE, "not initialised");
    std::string why;
    if (!ValidSettings(c, &why)) return Fail(MPCVR_E_INVALIDARG, "invalid settings: " + why);
    bool changeConvertShader = false, changeLuminance = false, changePlan = false;
    if (c.iTexFormat != m_cfg.iTexFormat) changePlan = true;
    if (c.iChromaScaling != m_cfg.iChromaScaling) changeConvertShader = true;
    if (c.iUpscaling != m_cfg.iUpscaling || c.iDownscaling != m_cfg.iDownscaling ||
        c.bInterpolateAt50pct != m_cfg.bInterpolateAt50pct) changePlan = true;
    if (c.bUseDither != m_cfg.bUseDither || c.output_format != m_cfg.output_format || c.flags != m_cfg.flags) changePlan = true;
    if (c.bConvertToSdr != m_cfg.bConvertToSdr) changeConvertShader = true;
    if (c.bDeintBlend != m_cfg.bDeintBlend) changePlan = true;
    if (c.iSDRDisplayNits != m_cfg.iSDRDisplayNits) changeLuminance = true;
    m_cfg = c;
    if (changeConvertShader || changeLuminance) m_blobOverride = false;
    if (changeConvertShader) { SetShaderConvertColorParams(); changePlan = true; }
    if (changeLuminance) { SetShaderLuminanceParams(); changePlan = true; }
    if (changePlan) m_planDirty = true;
    return (changeConvertShader || changeLuminance || changePlan) ? MPCVR_S_OK : MPCVR_S_FALSE;
}

// SetProcAmpValues — DX11VideoProcessor.cpp:4506-4537 (clamped to the ranges of Helper.cpp:182-187)
HRESULT CHipVideoProcessor::SetProcAmpValues(uint32_t flags, float b, float c, float h, float s)
{
    auto clampf = [](float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); };
    if (flags & MPCVR_PROCAMP_BRIGHTNESS) m_procAmp.brightness = clampf(b, -100.f, 100.f);
    if (flags & MPCVR_PROCAMP_CONTRAST) m_procAmp.contrast = clampf(c, 0.f, 2.f);
    if (flags & MPCVR_PROCAMP_HUE) m_procAmp.hue = clampf(h, -180.f, 180.f);
    if (flags & MPCVR_PROCAMP_SATURATION) m_procAmp.saturation = clampf(s, 0.f, 2.f);
    m_blobOverride = false;
    SetShaderConvertColorParams();
    m_planDirty = true;
    return MPCVR_S_OK;
}

static size_t SurfBytesPerPixel(int fmt) { return fmt == SF_RGBA16F ? 8 : 4; }
static int RgbTexFmt(const FmtConvParams &f);

// the plan's tables onto the device: one copy per axis pack and one for the strip pack.  The views are set from the packs alone: a table
// this plan does not have reads as null, whatever the buffers still hold
HRESULT CHipVideoProcessor::UploadPlanTables(const PlanTables &t)
{
    HRESULT hr;
    const std::pair<const std::vector<int32_t> *, DevBuffer *> packs[] = {{&t.x.words, &m_axisX}, {&t.y.words, &m_axisY}, {&t.stripPack.words, &m_stripTab}};
    for (const auto &p : packs) {
        if (p.first->empty()) continue;
        const size_t bytes = p.first->size() * sizeof(int32_t);
        if ((hr = CheckHip(p.second->CheckCreate(bytes), "plan tables alloc"))) return hr;
        if ((hr = CheckHip(hipMemcpy(p.second->ptr, p.first->data(), bytes, hipMemcpyHostToDevice), "plan tables upload"))) return hr;
    }
    m_tapsX = t.x.View(m_axisX.ptr); m_otherX = t.x.Other(m_axisX.ptr);
    m_tapsY = t.y.View(m_axisY.ptr); m_otherY = t.y.Other(m_axisY.ptr);
    return MPCVR_S_OK;
}

// UpdateTexures (:2869-2892) + UpdatePostScaleTexures (:2894-2912) + the per-axis shader choice of
// ResizeShaderPass (:3103-3133), evaluated once per geometry/settings change instead of per frame.
HRESULT CHipVideoProcessor::UpdatePlan()
{
    if (!m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    (void)hipSetDevice(m_device);
    (void)JoinFrameLanes(true);
    (void)hipStreamSynchronize(m_stream);    // resources below may still be in use
    const int w1 = m_srcRectWidth, h1 = m_srcRectHeight;
    const int w2 = m_videoRect.Width(), h2 = m_videoRect.Height();
    // 1. the plan
    {
        const PlanGeometry g{w1, h1, m_videoRect.left, m_videoRect.top, m_videoRect.right, m_videoRect.bottom,
                             m_windowRect.Width(), m_windowRect.Height(), m_iRotation, m_bFlip ? 1 : 0,
                             ConvertEnabled() ? 1 : 0, ToneMapActive() ? 1 : 0, m_doviValid ? 1 : 0};
        std::string why;
        if (!DecidePlan(m_cfg.iTexFormat, m_cfg.iChromaScaling, m_cfg.iUpscaling, m_cfg.iDownscaling,
                        m_cfg.bInterpolateAt50pct, m_cfg.bUseDither, m_cfg.output_format,
                        m_cfg.flags,
                        *m_srcParams, g, &m_plan, &why))
            return Fail(MPCVR_E_NOTIMPL, why);
    }

    // 2. the surfaces
    HRESULT hr;
    if (m_plan.hdr_tonemap &&
        (hr = CheckHip(m_TexPost.CheckCreate((size_t)w2 * SurfBytesPerPixel(m_plan.internal_fmt) * h2), "m_TexsPostScale"))) return hr;
    m_postBytes = m_plan.hdr_tonemap ? (size_t)w2 * SurfBytesPerPixel(m_plan.internal_fmt) * h2 : 0;
    m_midBytes = 0;
    // m_TexConvertOutput: srcRect-sized, internal format (:2889-2890)
    const size_t convPitch = (size_t)w1 * SurfBytesPerPixel(m_plan.internal_fmt);
    if ((hr = CheckHip(m_TexConvertOutput.CheckCreate(convPitch * h1), "m_TexConvertOutput"))) return hr;
    m_convBytes = convPitch * h1;

    if (m_plan.two_pass) {
        // m_TexResize: fp16, dst width x (source extent along screen y) (:3143-3160)
        if ((hr = CheckHip(m_TexResize.CheckCreate((size_t)w2 * 8 * m_plan.mid_h), "m_TexResize"))) return hr;
        m_midBytes = (size_t)w2 * 8 * m_plan.mid_h;
    }

    // 3. + 4. the tables (vp_plan_tables.h): built as one value, uploaded, then the context's replaced whole
    {
        static const bool no_strip_env = [] { const char *e = std::getenv("MPCVR_NO_STRIP"); return e && *e && *e != '0'; }();
        const PlanTablesInput in{m_srcRect.left, m_srcRect.top, w1, h1, m_srcWidth, m_srcHeight, w2, h2, m_cfg.iUpscaling, m_cfg.flags,
                                 m_tail == TAIL_PQ_TO_SDR || m_tail == TAIL_HLG_TO_SDR, no_strip_env};
        PlanTables tables;
        std::string why;
        if (!BuildPlanTables(m_plan, in, &tables, &why)) return Fail(MPCVR_E_NOTIMPL, why);
        if ((hr = UploadPlanTables(tables))) return hr;
        m_tables = std::move(tables);
    }

    // 5. Jinc2m phase tables of the draws that run the 2-D shader (their builders live beside the kernels)
    m_jincFirstTab = m_jincSecondTab = nullptr; m_jincFirstCtr = m_jincSecondCtr = nullptr;
    if (m_tables.firstJinc && (hr = UploadJincPhases(m_tables.firstCoords, m_jincFirst, &m_jincFirstTab, &m_jincFirstCtr))) return hr;
    if (m_tables.secondJinc && (hr = UploadJincPhases(m_tables.secondCoords, m_jincSecond, &m_jincSecondTab, &m_jincSecondCtr))) return hr;

    // the arbitrary-ratio fused kernel, where the tables fit it: straight from the raw sample for 4:2:0 sources (m_strip; the probes below
    // have the last word), else from the convert kernel's output / the RGB source texture (m_stripSurf): a frame turned upside down goes
    // convert kernel -> m_TexConvertOutput -> k_fused_strip:surface
    m_stripSurf = false;
    m_stripRan = -1;
    m_fusedAside = false;
    m_strip = m_tables.stripPlanned && m_plan.convert && !m_doviValid && m_plan.internal_fmt != SF_RGBA16F && m_plan.rotation == 0;

    // 6. the LUTs and the exact-2x kernel's baked image.  PQ -> SDR table: the fused kernel's tone-map stage and the folded convert kernel's
    if (m_tail == TAIL_PQ_TO_SDR) {
        if (!m_blobOverride) BuildPqSdrLut(m_lumScale, m_pqLutHost);
        if ((hr = CheckHip(m_pqLut.CheckCreate(sizeof(m_pqLutHost)), "pq lut"))) return hr;
        if ((hr = CheckHip(hipMemcpy(m_pqLut.ptr, m_pqLutHost, sizeof(m_pqLutHost), hipMemcpyHostToDevice), "pq lut upload"))) return hr;
        m_pqLutValid = true;
    } else {
        m_pqLutValid = false;
    }
    if (m_tail == TAIL_HLG_TO_SDR && !m_hlgLut.ptr) {          // constants only: built once per context
        std::vector<float> &t = m_hlgLutHost;
        t.resize(kPqLutSize);
        BuildHlgInverseLut(t.data());
        if ((hr = CheckHip(m_hlgLut.CheckCreate(t.size() * sizeof(float)), "hlg lut"))) return hr;
        if ((hr = CheckHip(hipMemcpy(m_hlgLut.ptr, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice), "hlg lut upload"))) return hr;
    }
    if ((hr = UploadFusedTables())) return hr;
    m_jincFusedTab = nullptr;
    if (m_plan.fused_jinc) {
        // the fused Jinc2m kernel's weights: the phase table of a 2x draw (integer origins drop out of it) in the kernel's reading order
        // (the draw the kernel replaces: the whole m_TexConvertOutput, src-rect sized, onto the video rect; BuildJincPhases checks every
        // output index's tap base against the shader's own texture coordinate)
        DrawCoords dc{};
        dc.step_x = dc.step_y = 0.5f;
        dc.len_x = dc.tex_x = m_srcRectWidth; dc.len_y = dc.tex_y = m_srcRectHeight;
        dc.n_x = m_videoRect.Width(); dc.n_y = m_videoRect.Height();
        std::vector<unsigned char> phases(JincPhasesBytes());
        std::vector<float> tab(FusedJincTableBytes() / sizeof(float));
        if (!BuildJincPhases(dc, phases.data(), kNominalPhaseMaxCodes / (float)m_plan.quant)) m_plan.fused_up2x = m_plan.fused_jinc = false;
        else {
#ifdef MPCVR_DEBUG_HOOKS        // (debug builds only — tools/debug/jinc_diff.py: a one-tap filter, which texel does an output pixel read?)
            if (const char *e = std::getenv("MPCVR_JINC_DBG")) {
                JincPhases &jp = *(JincPhases *)phases.data();
                const int tap = std::atoi(e);
                for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) { for (int k = 0; k < 16; k++) jp.w[a][b][k] = k == tap ? 1.0f : 0.0f; jp.wsum[a][b] = 1.0f; }
            }
#endif
            BuildFusedJincTable(phases.data(), tab.data());
            if ((hr = CheckHip(m_jincFused.CheckCreate(tab.size() * sizeof(float)), "fused jinc table"))) return hr;
            if ((hr = CheckHip(hipMemcpy(m_jincFused.ptr, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice), "fused jinc table upload"))) return hr;
            m_jincFusedTab = (const float *)m_jincFused.ptr;
        }
    }
    // 7. the exact-2x weights
    if (m_plan.fused_up2x) {
        if (!m_plan.fused_jinc && (!m_blobOverride || m_upX.ntaps == 0)) {
            float w[6];
            const int n = UpscaleWeights(m_cfg.iUpscaling, 0.75f, w);
            m_upX.ntaps = n; std::memset(m_upX.w_even, 0, sizeof(m_upX.w_even)); std::memset(m_upX.w_odd, 0, sizeof(m_upX.w_odd));
            std::memcpy(m_upX.w_even, w, sizeof(float) * n);
            UpscaleWeights(m_cfg.iUpscaling, 0.25f, w);
            std::memcpy(m_upX.w_odd, w, sizeof(float) * n);
            m_upX.q1_quirk = (m_cfg.iUpscaling == MPCVR_UPSCALE_Lanczos3 && !(m_cfg.flags & MPCVR_FLAG_LANCZOS3_FIXED)) ? 1 : 0;
            m_upY = m_upX;
        }
        FusedParams fp{};
        FillFusedParams(nullptr, nullptr, 0, &fp);
        m_plan.fused_up2x = FusedUp2xSupported(fp);
        // the fused Jinc2m kernel wants 114 - 146 KiB of LDS per workgroup: where the device grants less, the convert + k_jinc2 draws (advisor, round 5)
        if (m_plan.fused_jinc && FusedJincLdsBytes(fp) > DeviceLdsLimit()) m_plan.fused_up2x = false;
        if (!m_plan.fused_up2x) m_plan.fused_jinc = false;
        // experiment knob: exact 2x through the arbitrary-ratio kernel instead (DESIGN.md §4.3 compares the two)
        static const bool no_up2x_env = [] { const char *e = std::getenv("MPCVR_NO_UP2X"); return e && *e && *e != '0'; }();
        if (no_up2x_env && m_strip) m_plan.fused_up2x = false;
    }
    // 8. the launch-time probes
    m_period = false;
    // the store the resize draws will meet: the render target, or m_TexsPostScale in front of the HDR10 tone-mapping step (:3359-3367)
    const StoreParams probeStore = m_plan.hdr_tonemap ? MakeStore(nullptr, (int)(w2 * SurfBytesPerPixel(m_plan.internal_fmt)), m_plan.internal_fmt, false)
                                                      : MakeStore(nullptr, m_windowRect.Width() * 4, m_plan.swap_fmt, true);
    if (m_strip) {      // the launch-time conditions that do not depend on the frame pointers
        FusedStripParams sp{};
        m_strip = FillStripParams(nullptr, nullptr, probeStore.dst_pitch, probeStore, &sp);
        m_period = m_strip && FusedPeriodTakes(sp);
    }
    if (m_tables.stripPlanned && !m_strip) {
        FusedStripParams sp{};
        const Surface probe = m_plan.convert ? Surface{nullptr, (int)(w1 * SurfBytesPerPixel(m_plan.internal_fmt)), w1, h1, m_plan.internal_fmt}
                                             : Surface{nullptr, TexPitch(), m_srcWidth, m_srcHeight, RgbTexFmt(*m_srcParams)};
        m_stripSurf = FillStripSurfParams(probe, probeStore, &sp);
        m_period = m_stripSurf && FusedPeriodTakes(sp);
    }
    m_planDirty = false;
    if (LogLevel() >= 2)
        std::fprintf(stderr, "mpcvr[%p]: plan %s (%dx%d -> %dx%d in %dx%d)\n", (void *)this, GetPathInfo().c_str(), m_srcRectWidth, m_srcRectHeight,
                     m_videoRect.Width(), m_videoRect.Height(), m_windowRect.Width(), m_windowRect.Height());
    return MPCVR_S_OK;
}

// dyadic, unrotated Jinc2m draws take their 16 weights from a phase table (vp_kernels.hip: k_jinc2_phases)
HRESULT CHipVideoProcessor::UploadJincPhases(const DrawCoords &dc, DevBuffer &buf, const void **tab, const float **ctr)
{
    *tab = nullptr; *ctr = nullptr;
    HRESULT hr;
    std::vector<unsigned char> host(JincPhasesBytes());
    if ((m_cfg.flags & MPCVR_FLAG_NO_FUSED) || !BuildJincPhases(dc, host.data(), kNominalPhaseMaxCodes / (float)m_plan.quant)) {
        // the plain kernel: its per-column / per-row texture coordinates as a table (FillVertices' corner values interpolated in fp64, once per index)
        std::vector<float> c((size_t)dc.n_x + dc.n_y);
        BuildDrawCentres(dc, c.data());
        if ((hr = CheckHip(buf.CheckCreate(c.size() * sizeof(float)), "jinc centres"))) return hr;
        if ((hr = CheckHip(hipMemcpy(buf.ptr, c.data(), c.size() * sizeof(float), hipMemcpyHostToDevice), "jinc centres upload"))) return hr;
        *ctr = (const float *)buf.ptr;
        return MPCVR_S_OK;
    }
    if ((hr = CheckHip(buf.CheckCreate(host.size()), "jinc phases"))) return hr;
    if ((hr = CheckHip(hipMemcpy(buf.ptr, host.data(), host.size(), hipMemcpyHostToDevice), "jinc phases upload"))) return hr;
    *tab = buf.ptr;
    return MPCVR_S_OK;
}

bool CHipVideoProcessor::ConvertEnabled() const { return ConvertDrawEnabled(*m_srcParams, m_procAmp, m_doviValid); }

int CHipVideoProcessor::TexPitch() const
{
    if (!m_srcParams) return m_srcPitch;
    if (m_srcParams->cformat == MPCVR_CF_V210) return V210TexPitch(m_srcWidth);
    if (m_srcParams->layout == LAY_RGB) return m_srcWidth * (m_srcParams->bits10 ? 4 : 4 * m_srcParams->bytes);
    return m_srcPitch;
}

// format of the texture an interleaved RGB sample is copied into (Helper.cpp:345-354)
static int RgbTexFmt(const FmtConvParams &f) { return f.bits10 ? SF_RGB10A2 : (f.bytes == 2 ? SF_RGBA16 : SF_BGRA8); }

// GetCopyPlaneFunction (Helper.cpp:377-412): every format handled here is copied as is (the <<6 of CopyPlane10to16 is
// applied when a texel is loaded) except v210, which CopyFrameV210 unpacks into a Y210 texture.
HRESULT CHipVideoProcessor::PrepareSample(const uint8_t *dev_sample, const uint8_t **tex)
{
    HRESULT hr;
    if (m_srcParams->cformat != MPCVR_CF_V210 && m_srcParams->layout != LAY_RGB) {
        if (((uintptr_t)dev_sample & 3) == 0) { *tex = dev_sample; return MPCVR_S_OK; }
        // a device sample that does not start on a dword: the kernels read rows with 4- / 16-byte loads, so it is copied into
        // the context's own texture first — what the reference does with EVERY decoder-owned sample (CopySubresourceRegion,
        // DX11VideoProcessor.cpp:2563-2569)
        const size_t bytes = (size_t)m_srcPitch * m_srcLines;
        if ((hr = CheckHip(m_TexSrcVideo.CheckCreate(bytes), "m_TexSrcVideo"))) return hr;
        m_texSrcZeroed = false;
        // the copy runs on the context stream: behind every lane frame that still reads the texture, and in front of the lane frames to come
        OrderOnContextStream();
        if ((hr = CheckHip(hipMemcpyAsync(m_TexSrcVideo.ptr, dev_sample, bytes, hipMemcpyDeviceToDevice, m_stream), "sample copy"))) return hr;
        *tex = (const uint8_t *)m_TexSrcVideo.ptr;
        return MPCVR_S_OK;
    }
    const int tp = TexPitch();
    OrderOnContextStream();           // (the repacks below run on the context stream)
    const bool fresh = m_TexSrcVideo.size < (size_t)tp * m_srcHeight || !m_TexSrcVideo.ptr || !m_texSrcZeroed;
    if ((hr = CheckHip(m_TexSrcVideo.CheckCreate((size_t)tp * m_srcHeight), "m_TexSrcVideo"))) return hr;
    if (m_srcParams->layout == LAY_RGB) {
        // texels the reference's copy loop never writes (RGB48 remainder) stay zero
        if (fresh && (hr = CheckHip(hipMemsetAsync(m_TexSrcVideo.ptr, 0, (size_t)tp * m_srcHeight, m_stream), "clear texture"))) return hr;
        m_texSrcZeroed = true;
        if ((hr = CheckHip(LaunchRepackRgb(m_srcParams->repack, dev_sample, m_srcBottomUp ? -m_srcPitch : m_srcPitch,
                                           (uint8_t *)m_TexSrcVideo.ptr, tp, m_srcWidth, m_srcHeight, m_stream), "k_repack_rgb"))) return hr;
        *tex = (const uint8_t *)m_TexSrcVideo.ptr;
        return MPCVR_S_OK;
    }
    m_texSrcZeroed = false;
    if ((hr = CheckHip(LaunchRepackV210(dev_sample, m_srcPitch, (uint8_t *)m_TexSrcVideo.ptr, tp, m_srcHeight, m_stream), "k_repack_v210"))) return hr;
    *tex = (const uint8_t *)m_TexSrcVideo.ptr;
    return MPCVR_S_OK;
}

void CHipVideoProcessor::FillConvertParams(const uint8_t *sample, ConvertParams *P) const
{
    const FmtConvParams &f = *m_srcParams;
    std::memset(P, 0, sizeof(*P));
    // plane walk of MemCopyToTexSrcVideo — DX11VideoProcessor.cpp:1213-1252
    const int pitch0 = TexPitch();
    const int cromaH = m_srcHeight / f.div_h;
    const int cromaPitch = (f.planes == 3) ? pitch0 / f.div_w : pitch0;
    P->plane[0] = sample;
    P->plane[1] = (sample && f.planes > 1) ? sample + (size_t)pitch0 * m_srcHeight : nullptr;
    P->plane[2] = (sample && f.planes > 2) ? P->plane[1] + (size_t)cromaPitch * cromaH : nullptr;
    P->pitch[0] = pitch0; P->pitch[1] = cromaPitch; P->pitch[2] = cromaPitch;
    P->tex_w = m_srcWidth; P->tex_h = m_srcHeight;
    P->cw = m_srcWidth / f.div_w; P->ch = cromaH;
    P->rect_l = m_srcRect.left; P->rect_t = m_srcRect.top;
    P->out_w = m_srcRectWidth; P->out_h = m_srcRectHeight;
    P->fmt.planes = f.planes; P->fmt.bytes = f.bytes; P->fmt.div_w = f.div_w; P->fmt.div_h = f.div_h;
    P->fmt.shift = f.shift; P->fmt.v_first = f.v_first; P->fmt.subsampling = f.Subsampling; P->fmt.cdepth = f.CDepth;
    // m_pPSConvertColorDeint: 4:2:0 planar/bi-planar only (:2964), used for interlaced samples when bDeintBlend (:3075)
    P->blend_deint = (m_cfg.bDeintBlend && m_SampleFormat != 0 && f.Subsampling == 420 && f.planes >= 2) ? 1 : 0;
    P->fmt.layout = f.layout; P->fmt.bits10 = f.bits10;
    for (int k = 0; k < 4; k++) P->fmt.ci[k] = f.ci[k];
    P->chroma_scaling = m_cfg.iChromaScaling;
    switch (m_srcExFmt.VideoChromaSubsampling()) {          // Shaders.cpp:121-137
    case 7: P->chroma_loc = CLOC_COSITED; break;
    case 1: P->chroma_loc = CLOC_MPEG1; break;
    default: P->chroma_loc = CLOC_MPEG2; break;
    }
    P->tail = m_tail; P->gamma = m_gamma;
    std::memcpy(P->cm, m_cm, sizeof(m_cm));
    P->lum_scale = m_lumScale;
    std::memcpy(P->gamut, m_gamut, sizeof(m_gamut));
    P->out_fmt = m_plan.internal_fmt;
    P->dovi = m_doviValid ? (const DoviParams *)m_doviDev.ptr : nullptr;        // (one RPU per frame: RunBatchRoute points a whole-batch launch at the run's tables)
    P->pq_lut = (m_pqLutValid && !(m_cfg.flags & (MPCVR_FLAG_NO_LUT | MPCVR_FLAG_NO_FUSED))) ? (const float *)m_pqLut.ptr : nullptr;
}

StoreParams CHipVideoProcessor::MakeStore(void *dst, int pitch, int dstFmt, bool rt) const
{
    StoreParams s{};
    s.dst = dst; s.dst_pitch = pitch; s.dst_fmt = dstFmt;
    s.mode = ST_SURFACE; s.mid_fmt = m_plan.internal_fmt; s.quant = m_plan.quant;
    s.dither = (const uint16_t *)m_dither.ptr;
    if (rt) {
        s.off_x = m_videoRect.left; s.off_y = m_videoRect.top;
        s.clip_w = m_windowRect.Width(); s.clip_h = m_windowRect.Height();
        if (m_plan.final_pass) s.mode = ST_FINAL;
    }
    return s;
}

void CHipVideoProcessor::FillFusedParams(const uint8_t *sample, void *rt, int rtPitch, FusedParams *fp, int inflight) const
{
    FillConvertParams(sample, &fp->conv);
    fp->plane_off[0] = 0;
    fp->plane_off[1] = (size_t)m_srcPitch * m_srcHeight;
    fp->plane_off[2] = fp->plane_off[1] + (size_t)fp->conv.pitch[1] * fp->conv.ch;
    fp->wx = m_upX; fp->wy = m_upY;
    fp->out_w = m_videoRect.Width(); fp->out_h = m_videoRect.Height();
    fp->store = MakeStore(rt, rtPitch, m_plan.swap_fmt, true);
    const bool no_lut = (m_cfg.flags & MPCVR_FLAG_NO_LUT) != 0;
    fp->pq_lut = (m_pqLutValid && !no_lut) ? (const float *)m_pqLut.ptr : nullptr;
    fp->literal_tail = no_lut ? 1 : 0;
    fp->hlg_lut = (m_tail == TAIL_HLG_TO_SDR && !no_lut) ? (const float *)m_hlgLut.ptr : nullptr;
    fp->eotf_lut = (m_doviValid && !no_lut) ? (const float *)m_eotfLut.ptr : nullptr;
    fp->dovi_l2 = (m_doviValid && m_doviHost.l2_enabled) ? 1 : 0;
    fp->dovi_cm = nullptr;
    fp->jinc_tab = m_plan.fused_jinc ? m_jincFusedTab : nullptr;
    fp->exact_wide = m_plan.hdr_tonemap ? 1 : 0;
    fp->inflight = inflight;
    static const bool no_baked = [] { const char *e = std::getenv("MPCVR_FUSED_NO_BAKED"); return e && *e && *e != '0'; }();     // (A/B: the kernel's own staging loops)
    fp->baked = (m_fusedTabValid && !no_baked) ? m_fusedTab.ptr : nullptr;
    fp->baked_lut = m_fusedTabLut;
    fp->dst_aligned16 = (((uintptr_t)rt) & 15) == 0;        // batches: ProcessBatch checks every target
    fp->src_aligned16 = (((uintptr_t)sample) & 15) == 0;
    // vectorised convert: dword loads need 4-byte aligned rows and a source rect starting on a 4-px boundary
    fp->fast_convert = (m_srcRect.left % 4 == 0) && (m_srcRect.top % 2 == 0) && (m_srcPitch % 4 == 0) &&
                       (fp->conv.pitch[1] % 4 == 0) && (fp->plane_off[1] % 4 == 0) && (fp->plane_off[2] % 4 == 0) &&
                       !(m_cfg.flags & MPCVR_FLAG_NO_FAST_CONVERT);
}

// ------------------------------------------------------------------------------------------------
// CopySample — DX11VideoProcessor.cpp:2202-2597 (memory branch -> MemCopyToTexSrcVideo :1213-1252)
// ------------------------------------------------------------------------------------------------
HRESULT CHipVideoProcessor::CopySample(const void *data, int pitch, int memKind)
{
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (!data) return Fail(MPCVR_E_POINTER, "null sample");
    if (pitch != (m_srcBottomUp ? -m_srcPitch : m_srcPitch)) return Fail(MPCVR_E_UNEXPECTED, "sample pitch differs from the media type");   // :2545
    // (every refusal comes before anything is touched: the current sample, its upload slot and the stream it was last drawn on stay as they are)
    if (memKind != MPCVR_MEM_HOST && memKind != MPCVR_MEM_DEVICE && memKind != MPCVR_MEM_HOST_PINNED) return Fail(MPCVR_E_INVALIDARG, "mem_kind");
    (void)hipSetDevice(m_device);
    const size_t bytes = (size_t)m_srcPitch * m_srcLines;
    HRESULT hr;
    const auto t_host0 = std::chrono::steady_clock::now();
    struct HostTimer { CHipVideoProcessor *self; std::chrono::steady_clock::time_point t0;
                       ~HostTimer() { self->m_copyHostMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); } } host_timer{this, t_host0};
    MarkConsumed();                                  // the previous sample is done with as far as the host is concerned
    m_curSlot = -1;
    m_lastRun = nullptr;
    if (memKind == MPCVR_MEM_DEVICE) {               // zero-copy, cf. the IMediaSampleD3D11 branch :2528-2569
        return PrepareSample((const uint8_t *)data, &m_curSample);
    }
    if (!m_copyStream && (hr = CheckHip(hipStreamCreateWithFlags(&m_copyStream, hipStreamNonBlocking), "copy stream"))) return hr;
    int si;
    if ((hr = AcquireUploadSlot(bytes, &si))) return hr;
    UploadSlot &u = m_up[si];
    const void *from = data;
    if (memKind == MPCVR_MEM_HOST) {
        if (u.pinnedSize < bytes) {
            if (u.pinned) (void)hipHostFree(u.pinned);
            u.pinned = nullptr; u.pinnedSize = 0;
            if ((hr = CheckHip(hipHostMalloc(&u.pinned, bytes, hipHostMallocDefault), "pinned staging"))) return hr;
            u.pinnedSize = bytes;
        }
        std::memcpy(u.pinned, data, bytes);          // the reference's only per-frame CPU work (MemCopyToTexSrcVideo); the
        from = u.pinned;                             // <<6 / v210 / RGB repacks happen on the device (PrepareSample)
    }
    // the new data must not overtake work of the main stream that still reads this device buffer
    if (!m_evUp0 && ((hr = CheckHip(hipEventCreate(&m_evUp0), "upload timer")) || (hr = CheckHip(hipEventCreate(&m_evUp1), "upload timer")))) return hr;
    (void)hipEventRecord(m_evUp0, m_copyStream);
    if ((hr = CheckHip(hipMemcpyAsync(u.dev.ptr, from, bytes, hipMemcpyHostToDevice, m_copyStream), "upload"))) return hr;
    (void)hipEventRecord(m_evUp1, m_copyStream);
    m_upTimed = true;
    return PublishUploadSlot(si, m_copyStream);
}

HRESULT CHipVideoProcessor::AcquireUploadSlot(size_t bytes, int *si)
{
    *si = m_upNext;
    m_upNext = (m_upNext + 1) % kUploadSlots;
    UploadSlot &u = m_up[*si];
    HRESULT hr;
    if (!u.uploaded) {
        if ((hr = CheckHip(hipEventCreateWithFlags(&u.uploaded, hipEventDisableTiming), "upload event"))) return hr;
        if ((hr = CheckHip(hipEventCreateWithFlags(&u.consumed, hipEventDisableTiming), "consume event"))) return hr;
    }
    // the slot's staging / device buffers are free once the work that last used them has completed
    if (u.inFlight && (hr = CheckHip(hipEventSynchronize(u.consumedRecorded ? u.consumed : u.uploaded), "upload slot wait"))) return hr;
    return CheckHip(u.dev.CheckCreate(bytes), "upload buffer");
}

HRESULT CHipVideoProcessor::PublishUploadSlot(int si, hipStream_t recordedOn)
{
    UploadSlot &u = m_up[si];
    HRESULT hr;
    if ((hr = CheckHip(hipEventRecord(u.uploaded, recordedOn), "upload event"))) return hr;
    if (recordedOn != m_stream && (hr = CheckHip(hipStreamWaitEvent(m_stream, u.uploaded, 0), "stream wait"))) return hr;
    u.inFlight = true; u.consumedRecorded = false;
    m_curSlot = si;
    return PrepareSample((const uint8_t *)u.dev.ptr, &m_curSample);
}

// a Process / Render that read the current upload slot has been queued: the slot may be recycled after it
void CHipVideoProcessor::MarkConsumed()
{
    if (m_curSlot < 0) return;
    UploadSlot &u = m_up[m_curSlot];
    if (!u.consumed) return;
    hipStream_t const s = m_lastRun ? m_lastRun : m_stream;
    // one event stands for every reader: a sample drawn again on another stream (a second target on another lane, Render, the snapshot) puts
    // that stream behind the readers recorded so far before the event moves there.  A sample drawn once records on one stream and never waits.
    if (u.consumedRecorded && u.consumedOn != s) (void)hipStreamWaitEvent(s, u.consumed, 0);
    if (hipEventRecord(u.consumed, s) == hipSuccess) { u.consumedRecorded = true; u.consumedOn = s; }
}

// the block convert into m_TexConvertOutput (`out`; a batch's chunks set it to theirs) in front of a draw
FusedParams CHipVideoProcessor::ConvertOutputParams(const uint8_t *sample, void *out, int inflight) const
{
    const int pitch = (int)(m_srcRectWidth * SurfBytesPerPixel(m_plan.internal_fmt));
    FusedParams fp{};
    FillFusedParams(sample, out, pitch, &fp, inflight);
    fp.store = MakeStore(out, pitch, m_plan.internal_fmt, false);
    fp.dst_aligned16 = 1;
    fp.exact_convert = 1;
    return fp;
}

HRESULT CHipVideoProcessor::ConvertColorPass(const uint8_t *sample, const RunOn &on)
{
    ConvertParams P;
    FillConvertParams(sample, &P);
    Surface out{m_TexConvertOutput.ptr, (int)(m_srcRectWidth * SurfBytesPerPixel(m_plan.internal_fmt)),
                m_srcRectWidth, m_srcRectHeight, m_plan.internal_fmt};
    if (!(m_cfg.flags & MPCVR_FLAG_NO_FUSED)) {           // the fused kernel's block convert, when the source qualifies
        const FusedParams fp = ConvertOutputParams(sample, out.ptr, on.inflight);
        if (ConvertBlocksSupported(fp, false))
            return CheckHip(LaunchConvertBlocks(fp, LaunchFrames::One(sample, out.ptr), on.stream), "k_convert_blocks");
    }
    return CheckHip(LaunchConvert(P, out, on.stream, (m_cfg.flags & MPCVR_FLAG_NO_FUSED) != 0), "k_convert");
}

// ResizeShaderPass (:3103-3187) with FinalPass (:3189-3233) folded into the epilogue of the last draw: one frame, or a chunk of a batch
// with the chunk as every launch's frame dimension (DrawFrames)
HRESULT CHipVideoProcessor::ResizeShaderPass(const uint8_t *sample, void *rt, int rtPitch, const DrawFrames &df, const RunOn &on)
{
    const int w1 = m_srcRectWidth, h1 = m_srcRectHeight, w2 = m_videoRect.Width(), h2 = m_videoRect.Height();
    Surface conv{df.conv, (int)(w1 * SurfBytesPerPixel(m_plan.internal_fmt)), w1, h1, m_plan.internal_fmt};
    // (a batch reaches neither the source texture nor the copy below: BatchPlan refuses a plan without the convert draw, or with neither
    // a draw nor the HDR10 step)
    if (!m_plan.convert)      // pInputTexture = &m_TexSrcVideo (:3321-3323)
        conv = Surface{(void *)sample, TexPitch(), m_srcWidth, m_srcHeight, RgbTexFmt(*m_srcParams)};
    const StoreParams final = MakeStore(rt, rtPitch, m_plan.swap_fmt, true);
    // with the HDR10 tone-mapping step the resize draws into a post-scale texture (internal format, video-rect sized)
    // and the step itself writes the render target / runs the final pass (:3359-3367)
    Surface post{df.post, (int)(w2 * SurfBytesPerPixel(m_plan.internal_fmt)), w2, h2, m_plan.internal_fmt};
    const StoreParams last = m_plan.hdr_tonemap ? MakeStore(post.ptr, post.pitch, m_plan.internal_fmt, false) : final;
    // a draw from the convert output into the last draw's targets
    ResizeBatch b; b.n = df.n; b.in_stride = df.convStride; b.frames = df.lastTab; b.dst_aligned8 = df.aligned;
    HRESULT hr = MPCVR_S_OK;
    bool drawn = true;
    const bool plain = (m_cfg.flags & MPCVR_FLAG_NO_FUSED) != 0;      // keep the whole path on the one-kernel-fits-all versions
    const bool jfast = !(m_cfg.flags & (MPCVR_FLAG_NO_FUSED | MPCVR_FLAG_NO_FAST_CONVERT));       // Jinc2m quad kernel: default tier only
    FusedStripParams ssp{};
    const bool surfStrip = m_stripSurf && FillStripSurfParams(conv, last, &ssp);
    if (m_stripSurf) m_fusedAside = !surfStrip;
    if (surfStrip) {
        // convert output (or RGB source texture) -> both draws -> final pass in the arbitrary-ratio fused kernel, no convert stage
        ssp.surf_stride = df.convStride;
        if (df.lastTab) ssp.fp.dst_aligned16 = df.aligned;
        const LaunchFrames frames = df.lastTab ? LaunchFrames::Device(df.lastTab, df.n) : LaunchFrames::One((const uint8_t *)conv.ptr, last.dst);
        hr = CheckHip(LaunchFusedStrip(ssp, frames, on.stream), "k_fused_strip<surface>");
    } else if (m_plan.two_pass && !plain && !m_tables.firstJinc && !m_tables.secondJinc && m_tables.firstAxis == 0 && !m_tables.firstSwap &&
        Resize2DSupported(conv, m_tapsX, m_tapsY, last)) {
        // both draws in one LDS-tiled kernel: m_TexResize stays on chip
        hr = CheckHip(LaunchResize2D(conv, m_tapsX, m_tapsY, m_otherX, m_plan.mid_h, w2, h2, last, on.stream, &b), "k_resize_2d");
    } else if (m_plan.two_pass) {
        Surface mid{df.mid, w2 * 8, w2, m_plan.mid_h, SF_RGBA16F};
        StoreParams st = MakeStore(mid.ptr, mid.pitch, SF_RGBA16F, false);
        ResizeBatch b1; b1.n = df.n; b1.in_stride = df.convStride; b1.dst_stride = df.midStride;
        if (m_tables.firstJinc) hr = CheckHip(LaunchJinc2(conv, m_tables.firstCoords, w2, m_plan.mid_h, st, on.stream, m_jincFirstTab, jfast, &b1, m_jincFirstCtr), "k_jinc2");
        else hr = CheckHip(LaunchResize(m_tables.firstAxis, m_tables.firstSwap, conv, m_tapsX, m_otherX, w2, m_plan.mid_h, st, on.stream, plain, &b1), "k_resize<first>");
        if (hr) return hr;
        ResizeBatch b2 = b; b2.in_stride = df.midStride;
        if (m_tables.secondJinc) hr = CheckHip(LaunchJinc2(mid, m_tables.secondCoords, w2, h2, last, on.stream, m_jincSecondTab, jfast, &b2, m_jincSecondCtr), "k_jinc2");
        else hr = CheckHip(LaunchResize(1, false, mid, m_tapsY, m_otherY, w2, h2, last, on.stream, plain, &b2), "k_resize<Y>");
    } else if (m_plan.one_pass) {
        if (m_tables.firstJinc) hr = CheckHip(LaunchJinc2(conv, m_tables.firstCoords, w2, h2, last, on.stream, m_jincFirstTab, jfast, &b, m_jincFirstCtr), "k_jinc2");
        else hr = CheckHip(LaunchResize(m_tables.firstAxis, m_tables.firstSwap, conv, m_tapsX, m_otherX, w2, h2, last, on.stream, plain, &b), "k_resize<one>");
    } else {
        drawn = false;
        if (!m_plan.convert) {    // the next step reads the source rect of the texture (pTex = pInputTexture, :3352)
            const int bpp = conv.fmt == SF_RGBA16 ? 8 : 4;
            conv.ptr = (uint8_t *)conv.ptr + (size_t)m_srcRect.top * conv.pitch + (size_t)m_srcRect.left * bpp;
            conv.w = w1; conv.h = h1;
        }
        if (!m_plan.hdr_tonemap) {
            StoreParams direct = final;
            if (!m_plan.convert) direct.mid_fmt = conv.fmt;   // nothing was drawn into m_TexsPostScale: the final pass sees the texture's own precision
            return CheckHip(LaunchCopy(conv, w2, h2, direct, on.stream), "k_copy");
        }
    }
    if (hr || !m_plan.hdr_tonemap) return hr;
    ResizeBatch tb; tb.n = df.n; tb.in_stride = drawn ? df.postStride : df.convStride; tb.frames = df.rtTab;
    return CheckHip(LaunchHdr10ToneMap(drawn ? post : conv, m_hdrTm, w2, h2, final, on.stream, &tb), "k_hdr10_tonemap");
}

// what both forms of the arbitrary-ratio fused kernel take from the plan: the target, the strip tables and, for a periodic vertical ratio,
// the register-window kernel's (per_force: FusedStripParams::per_force); false: this launch cannot take it (alignment, sizes)
bool CHipVideoProcessor::FillStripTables(const StoreParams &store, int perForce, FusedStripParams *sp) const
{
    sp->fp.store = store;
    sp->ran_period = &m_stripRan;
    if (!m_tables.stripPlanned) return false;
    const int32_t *tab = (const int32_t *)m_stripTab.ptr;
    const size_t *so = m_tables.stripPack.stripOff, *po = m_tables.stripPack.periodOff;
    sp->yrange = tab + so[0]; sp->xstrip = tab + so[1];
    sp->xi_t = tab + so[2]; sp->xw_t = tab + so[3];
    sp->yi = tab + so[4]; sp->yw = tab + so[5];
    sp->out_w = m_videoRect.Width(); sp->out_h = m_videoRect.Height();
    sp->nt = m_tables.strip.nt; sp->pxl = m_tables.strip.pxl; sp->strip_w = m_tables.strip.strip_w; sp->ring = m_tables.strip.ring; sp->acols = m_tables.strip.acols;
    sp->per_P = 0;
    if (m_tables.period.P && !(m_cfg.flags & MPCVR_FLAG_NO_PERIOD)) {
        sp->per_P = m_tables.period.P; sp->per_Q = m_tables.period.Q; sp->per_nt = m_tables.period.nt; sp->per_acols = m_tables.period.acols; sp->per_strip_w = m_tables.period.strip_w; sp->per_own = m_tables.period.own; sp->per_force = perForce;
        sp->per_xi_t = tab + po[0]; sp->per_xw_t = tab + po[1]; sp->per_yw = tab + po[2]; sp->per_xstrip = tab + po[3];
    }
    return FusedStripSupported(*sp) && FusedStripLdsBytes(*sp) <= DeviceLdsLimit();
}

// parameters of the arbitrary-ratio fused kernel for one launch; false: this launch cannot take it (alignment, sizes)
bool CHipVideoProcessor::FillStripParams(const uint8_t *sample, void *dst, int dstPitch, const StoreParams &store, FusedStripParams *sp, int inflight) const
{
    FillFusedParams(sample, dst, dstPitch, &sp->fp, inflight);
    sp->fp.dst_aligned16 = (((uintptr_t)dst) & 7) == 0;         // (8 bytes here, as in FillStripSurfParams)
    return FillStripTables(store, (m_cfg.flags & MPCVR_FLAG_FORCE_PERIOD) ? 1 : 0, sp);
}

// the same kernel without its convert stage: `src` = m_TexConvertOutput (any convert kernel wrote it) or the RGB source texture
bool CHipVideoProcessor::FillStripSurfParams(const Surface &src, const StoreParams &store, FusedStripParams *sp) const
{
    *sp = FusedStripParams{};
    // (the strip kernel decides its 8-byte stores from the pointer itself, the periodic kernel from this flag: 8 bytes is all either needs —
    // a single frame into a target on an 8-byte boundary takes the periodic kernel like a batch into it does.  Batches: the caller knows
    // every target of the table and overrides it)
    sp->fp.dst_aligned16 = (((uintptr_t)store.dst) & 7) == 0;
    sp->surface_mode = 1;
    sp->surf = src;
    sp->other = m_tapsX.other_identity ? nullptr : m_otherX;
    sp->mid_h = m_plan.mid_h;
    return FillStripTables(store, 1, sp);      // (per_force: with a periodic vertical ratio the register-window kernel reads the surface as well)
}

HRESULT CHipVideoProcessor::ProcessOne(const uint8_t *sample, void *rt, int rtPitch, const RunOn &on)
{
    HRESULT hr;
    m_fusedAside = false;
    if (m_plan.fused_up2x) {
        FusedParams fp{};
        FillFusedParams(sample, rt, rtPitch, &fp, on.inflight);
        // UpdatePlan asked FusedUp2xSupported without a target (pitch 0): what depends on THIS call's target is asked here, as the strip and
        // same-size routes below ask it — rows that span 4 GiB go to the convert kernel and the resize draws, which store through size_t
        if (StoreRowsFit32(fp.store, fp.out_h))       // (a single frame travels by value in the kernel arguments)
        {
            FusedUp2xLastForm() = -1;
            const hipError_t e = LaunchFusedUp2x(fp, LaunchFrames::One(sample, rt), on.stream);
            if (FusedUp2xLastForm() >= 0) m_up2xForm = FusedUp2xLastForm();      // (GetLastBatchInfo: ";up2x=")
            return CheckHip(e, "k_fused_up2x");
        }
        m_fusedAside = true;
    }
    if (m_strip) {
        // with the HDR10 tone-mapping step the resize draws into the post-scale texture and the step writes the target (:3359-3367)
        const int w2 = m_videoRect.Width(), h2 = m_videoRect.Height();
        Surface post{m_TexPost.ptr, (int)(w2 * SurfBytesPerPixel(m_plan.internal_fmt)), w2, h2, m_plan.internal_fmt};
        const StoreParams final = MakeStore(rt, rtPitch, m_plan.swap_fmt, true);
        const StoreParams last = m_plan.hdr_tonemap ? MakeStore(post.ptr, post.pitch, m_plan.internal_fmt, false) : final;
        FusedStripParams sp{};
        if (FillStripParams(sample, last.dst, last.dst_pitch, last, &sp, on.inflight)) {
            if ((hr = CheckHip(LaunchFusedStrip(sp, LaunchFrames::One(sample, last.dst), on.stream), "k_fused_strip"))) return hr;
            if (!m_plan.hdr_tonemap) return MPCVR_S_OK;
            return CheckHip(LaunchHdr10ToneMap(post, m_hdrTm, w2, h2, final, on.stream), "k_hdr10_tonemap");
        }
        m_fusedAside = true;
    }
    if (m_plan.direct_convert) {
        FusedParams fp{};
        FillFusedParams(sample, rt, rtPitch, &fp, on.inflight);
        if (ConvertBlocksSupported(fp, true))
            return CheckHip(LaunchConvertBlocks(fp, LaunchFrames::One(sample, rt), on.stream), "k_convert_blocks");
        ConvertParams P;
        FillConvertParams(sample, &P);
        return CheckHip(LaunchConvertDirect(P, MakeStore(rt, rtPitch, m_plan.swap_fmt, true), on.stream), "k_convert_direct");
    }
    if (m_plan.convert && (hr = ConvertColorPass(sample, on))) return hr;
    return ResizeShaderPass(sample, rt, rtPitch, DrawFrames{m_TexConvertOutput.ptr, m_TexResize.ptr, m_TexPost.ptr}, on);
}

// A render target is made of dwords (4 bytes per pixel, and no kernel stores less than one): its first byte and its pitch are multiples of 4
// (include/mpcvr.h).  Checked in front of every launch, so a target that is refused stays untouched.
HRESULT CHipVideoProcessor::CheckTargetLayout(int n, void *const *dsts, int rtPitch)
{
    if (rtPitch & 3) return Fail(MPCVR_E_INVALIDARG, "render-target pitch is not a multiple of 4");
    for (int i = 0; i < n; i++)
        if ((uintptr_t)dsts[i] & 3) return Fail(MPCVR_E_INVALIDARG, "render target does not start on a multiple of 4 bytes");
    return MPCVR_S_OK;
}

// Process — DX11VideoProcessor.cpp:3285-3424
HRESULT CHipVideoProcessor::ProcessFrame(void *pRenderTarget, int rtPitch, const CRect *srcRect, const CRect *dstRect, size_t clearBytes, bool onContextStream)
{
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (!pRenderTarget) return Fail(MPCVR_E_POINTER, "null render target");
    if (HRESULT bad = CheckTargetLayout(1, &pRenderTarget, rtPitch)) return bad;
    if (!m_curSample) return Fail(MPCVR_E_NOT_VALID_STATE, "no sample: call CopySample first");
    if (srcRect && !srcRect->IsRectNull() && *srcRect != m_srcRect)
        return Fail(MPCVR_E_INVALIDARG, "src_rect must equal the input's source rect");
    (void)hipSetDevice(m_device);
    HRESULT hr;
    if (dstRect && !dstRect->IsRectNull()) { if ((hr = SetVideoRect(*dstRect))) return hr; }
    if (rtPitch < m_windowRect.Width() * 4) return Fail(MPCVR_E_INVALIDARG, "render-target pitch smaller than a row");
    if (m_planDirty && (hr = UpdatePlan())) return hr;
    const RtSpan span = TargetSpan(pRenderTarget, rtPitch);
    // (where the target's rows span 4 GiB the fused kernels step aside — ProcessOne — and a resize then goes through the context's intermediates,
    // which are shared: such a frame runs in stream order.  The same-size per-pixel convert shares nothing and would be safe on a lane; it stays
    // off them too, so that one condition decides)
    const bool rows32 = StoreRowsFit32(MakeStore(pRenderTarget, rtPitch, m_plan.swap_fmt, true), m_videoRect.Height());
    const int lane = (onContextStream || !rows32 || !FrameLanesUsable()) ? -1 : m_lanes.PickFrameLane(span);
    // (on the lanes the kernels size their segments for that many frames side by side)
    const RunOn on{lane >= 0 ? m_lanes.Stream(lane) : m_stream, lane >= 0 ? FrameLanes::Count() : 1};
    if (lane >= 0) {
        m_lanes.LaneWaitsForStream(lane, m_stream);     // behind a batch / an off-lane frame / a sample copy still queued on the context stream
        // the sample's upload (copy stream) was ordered in front of the context stream by CopySample: the lane needs the same edge
        if (m_curSlot >= 0 && m_up[m_curSlot].uploaded) (void)hipStreamWaitEvent(on.stream, m_up[m_curSlot].uploaded, 0);
    } else OrderOnContextStream();        // strictly in stream order behind whatever the lanes still hold (a plan that left the lanes, a caller's stream, the snapshot)
    if (clearBytes) (void)hipMemsetAsync(m_BackBuffer.ptr, 0, clearBytes, on.stream);
    // the timing pair (m_RenderStats.paintticks' stand-in): every frame off the lanes; on the lanes one frame in eight — two timestamped
    // events per frame are two more packets in front of and behind a 45 us kernel on each of four queues (same box, timed every frame /
    // every 8th: 4K -> 8K 20.03 k -> 20.35 k frames/s, 1080p same size 111 k -> 121-162 k; profiles/r04/ab_call29_lane_timing.jsonl)
    static const int every = [] { const char *e = std::getenv("MPCVR_LANE_TIMING_EVERY"); const int v = e && *e ? std::atoi(e) : 8; return v < 1 ? 1 : v; }();
    const bool timeIt = lane < 0 || every == 1 || (m_laneFrames++ % (unsigned)every) == 0 || !m_timed;
    if (timeIt) (void)hipEventRecord(m_evStart, on.stream);
    if (m_plan.errdiff) {
        // EXTENSION (bUseDither = 2): the draws render into the window-sized R10G10B10A2 intermediate, as for a 10-bit swap chain; the
        // error-diffusion pass takes it to the render target
        if (!(hr = PrepareErrDiff(1)) && !(hr = ProcessOne(m_curSample, m_edBase, m_edPitch, on)))
            hr = ErrDiffPass(LaunchFrames::One(m_edBase, pRenderTarget), rtPitch, on.stream);
    } else
        hr = ProcessOne(m_curSample, pRenderTarget, rtPitch, on);
    if (timeIt) (void)hipEventRecord(m_evStop, on.stream);
    m_lastRun = on.stream;
    MarkConsumed();
    if (lane >= 0) m_lanes.NoteLaneFrame(lane, span);
    m_timed = true;
    return hr;
}

HRESULT CHipVideoProcessor::CheckBatchArgs(int n, const void *const *srcs, void *const *dsts, int rtPitch)
{
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (n <= 0 || !srcs || !dsts) return Fail(MPCVR_E_INVALIDARG, "empty batch");
    if (rtPitch < m_windowRect.Width() * 4) return Fail(MPCVR_E_INVALIDARG, "render-target pitch smaller than a row");
    if (HRESULT bad = CheckTargetLayout(n, dsts, rtPitch)) return bad;
    for (int i = 0; i < n; i++)
        if (!srcs[i] || !dsts[i]) return Fail(MPCVR_E_POINTER, "null frame in batch");
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::ProcessBatch(int n, const void *const *srcs, void *const *dsts, int rtPitch)
{
    const BatchRecord record(*this, n);
    if (HRESULT bad = CheckBatchArgs(n, srcs, dsts, rtPitch)) return bad;
    BatchRun run{n, srcs, dsts, rtPitch};
    return RunBatch(run);
}

HRESULT CHipVideoProcessor::RunBatch(BatchRun &run)
{
    (void)hipSetDevice(m_device);
    if (HRESULT bad = m_planDirty ? UpdatePlan() : MPCVR_S_OK) return bad;
    return m_plan.errdiff ? ProcessBatchErrDiff(run) : ProcessBatchRoutes(run);
}

// One batch: classified once (ClassifyBatch), then run on one of two lanes beside the batch before it when its route shares nothing
// with it (FrameLanes); everything else — and every batch of a context on a caller's stream — in stream order on the context stream
HRESULT CHipVideoProcessor::ProcessBatchRoutes(BatchRun &run)
{
    BatchRoutePlan rp = ClassifyBatch(run);
    std::vector<RtSpan> targets((size_t)run.n);
    for (int i = 0; i < run.n; i++) targets[i] = TargetSpan(run.dsts[i], run.rtPitch);
    const int bl = PlaceBatch(rp, run, std::move(targets));
    const HRESULT hr = RunBatchRoute(rp, run);
    NoteBatchQueued(bl);
    return hr;
}

int CHipVideoProcessor::PlaceBatch(const BatchRoutePlan &rp, BatchRun &run, std::vector<RtSpan> &&writes)
{
    // The same rule as for single frames — nothing a batch touches may be shared with the batch beside it — read off the route the batch takes:
    // the exact-2x kernel, the strip / periodic kernel reading the samples themselves, the same-size block convert (no intermediate surface; a
    // repacked v210 batch reads the shared m_batchTex); default tier only.  Two launches in flight were measured to pay on every such route (same
    // box, bench.py process_batch_on_lanes against `value`, a quarter of a second of batches each; profiles/r06/bench_batch_lanes_all_routes_call32.txt,
    // bench_batch_lanes_call27.txt): same-size block convert +11-16 %, exact-2x kernel +2-5 % (4K -> 8K, four rounds of waves per batch) to +15 %
    // (1080p -> 4K, one round), strip / periodic kernel +11-29 % (1080p -> 1440p 99.8 k -> 116.4 k frames/s, 720p -> 1080p 190 k -> 246 k), fused
    // Jinc2m +4 %.  (An earlier table that had the strip kernels LOSE was a wall clock around 30 launches of 0.3 ms: it measured the closing synchronize.)
    const int bl = BatchLaneEligible(rp, run) ? m_lanes.PickBatchLane(std::move(writes), &m_lastBatchWaits) : -1;
    run.on = RunOn{bl >= 0 ? m_lanes.Stream(bl) : m_stream};
    if (bl >= 0) {
        m_lastBatchLane = bl;
        m_lanes.LaneWaitsForStream(bl, m_stream);    // behind whatever the context stream was given since the lane last looked
    } else OrderOnContextStream();           // behind every single frame still in flight, and single frames queued after it run behind the batch
    return bl;
}

// May the batch run on a batch lane?  One launch with nothing shared, on a context that owns its stream, default tier (the measurements: the
// comment in PlaceBatch).  PrepareSample, ApplyDoviFrame / UploadDoviParams and UploadDoviTables queue on the context stream whatever
// the run says: they are reached only from routes that never take a lane — FrameByFrame is no lane route, and a run with Dolby Vision
// metadata fails the condition below.
bool CHipVideoProcessor::BatchLaneEligible(const BatchRoutePlan &rp, const BatchRun &run) const
{
    static const bool lanesOff = [] { const char *e = std::getenv("MPCVR_NO_BATCH_LANES"); return e && *e && *e != '0'; }();
    const bool laneRoute = rp.route == BatchRoute::FusedUp2x || rp.route == BatchRoute::Strip || rp.route == BatchRoute::DirectConvert;
    return laneRoute && !rp.repackSlot && !lanesOff && m_ownStream && run.n >= 2 && !m_doviValid && !run.dvFrames && !m_plan.errdiff && !m_plan.hdr_tonemap &&
           !(m_cfg.flags & (MPCVR_FLAG_NO_FRAME_LANES | MPCVR_FLAG_NO_FUSED | MPCVR_FLAG_NO_FAST_CONVERT | MPCVR_FLAG_NO_STRIP));
}

// The route of a batch, from the plan and the frames' pointers alone: nothing is launched, allocated or written here.  The pointers of
// buffers RunBatchRoute may still (re)allocate are left null in the parameters (their checks do not read them).
CHipVideoProcessor::BatchRoutePlan CHipVideoProcessor::ClassifyBatch(const BatchRun &run) const
{
    const int n = run.n, rtPitch = run.rtPitch;
    const void *const *const srcs = run.srcs;
    void *const *const dsts = run.dsts;
    BatchRoutePlan rp;
    const bool v210 = m_srcParams->cformat == MPCVR_CF_V210, rgb = m_srcParams->layout == LAY_RGB;
    const bool fast = !(m_cfg.flags & (MPCVR_FLAG_NO_FUSED | MPCVR_FLAG_NO_FAST_CONVERT)), fastStrip = fast && !(m_cfg.flags & MPCVR_FLAG_NO_STRIP);
    // v210 samples are repacked into m_TexSrcVideo's layout first (CopyFrameV210, Helper.cpp:709-748): a batch gets one repack launch
    // per 32 frames into the slots of a batch texture, and the launches read the slots as if they were the samples
    const size_t slot = ((size_t)TexPitch() * m_srcHeight + 255) & ~(size_t)255;
    if (v210 && n > 1 && fast && slot * (size_t)n <= ((size_t)1 << 30)) rp.repackSlot = slot;
    for (int i = 0; i < n; i++) {
        if (!rp.repackSlot && ((uintptr_t)srcs[i] & 15) != 0) rp.src16 = false;
        if (!rp.repackSlot && ((uintptr_t)srcs[i] & 3) != 0) rp.src4 = false;
        if (((uintptr_t)dsts[i] & 15) != 0) rp.aligned = false;
        if (((uintptr_t)dsts[i] & 7) != 0) rp.aligned8 = false;
    }
    // samples that are repacked into m_TexSrcVideo one by one (v210 past the batch texture, interleaved RGB) cannot be read in place by a
    // whole-batch launch: they go frame by frame like samples that do not start on a dword
    if ((v210 && !rp.repackSlot) || rgb) rp.src4 = false;
    // (the launches take every sample from the frame table: the planners see the first one's alignment — slot 0 of m_batchTex when repacked)
    const uint8_t *const sample0 = rp.repackSlot ? nullptr : (const uint8_t *)srcs[0];
    const StoreParams target = MakeStore(dsts[0], rtPitch, m_plan.swap_fmt, true);
    // the arbitrary-ratio fused kernel takes the whole batch in one launch, like the 2x kernel
    FusedStripParams sp{};
    // the exact-2x kernels were planned without a target (UpdatePlan): this batch's pitch has its say here, as in ProcessOne
    const bool up2x = m_plan.fused_up2x && StoreRowsFit32(target, m_videoRect.Height());
    const bool strip = m_strip && !up2x && !m_plan.hdr_tonemap && rp.src4 && !run.dvFrames && FillStripParams(sample0, dsts[0], rtPitch, target, &sp);
    m_fusedAside = m_plan.fused_up2x ? !up2x : (m_strip && !m_plan.hdr_tonemap && !strip);       // (frame by frame: ProcessOne says it again per frame)
    // pass-per-kernel path, whole batch per launch: possible when every stage has a kernel with a frame dimension.  One RPU per frame
    // (ProcessBatchDovi): the block convert's Dolby Vision variants index the run's tables by the frame; the HDR10 tone-mapping step takes
    // its level-1 constants by value, so such a run goes frame by frame
    const bool batchable = !up2x && !strip && n > 1 && rp.src4 && fast && !(run.dvFrames && (!run.dvTab || m_plan.hdr_tonemap)) &&
                           BatchPlan(sample0, dsts[0], rtPitch, rp.aligned, rp.repackSlot != 0, rp.src16, &rp.conv, &rp.direct);
    auto take = [&rp](BatchRoute r) { rp.route = r; return rp; };
    if (batchable && m_plan.direct_convert) return take(BatchRoute::DirectConvert);
    if (rgb && !m_plan.convert && m_stripSurf && m_plan.two_pass && !m_plan.hdr_tonemap && n > 1 && fastStrip &&
        FillStripSurfParams(Surface{nullptr, TexPitch(), m_srcWidth, m_srcHeight, RgbTexFmt(*m_srcParams)}, target, &sp)) {
        rp.strip = sp;
        return take(BatchRoute::RgbSurfaceStrip);
    }
    if (m_plan.hdr_tonemap && m_strip && !up2x && rp.src4 && n > 1 && fastStrip) {
        const int postPitch = (int)(m_videoRect.Width() * SurfBytesPerPixel(m_plan.internal_fmt));
        if (FillStripParams(sample0, nullptr, postPitch, MakeStore(nullptr, postPitch, m_plan.internal_fmt, false), &sp)) {
            rp.strip = sp;
            return take(BatchRoute::StripToneMap);
        }
    }
    // (a batch of one needs no frame table: the frame travels in the kernel arguments, like mpcvr_process)
    if ((!up2x && !strip && !batchable) || !rp.src4 || n == 1) return take(BatchRoute::FrameByFrame);
    if (batchable) return take(BatchRoute::WholeBatchLaunches);
    if (strip) {
        rp.strip = sp;
        return take(BatchRoute::Strip);
    }
    return take(BatchRoute::FusedUp2x);
}

// the launches of a classified batch on run.on.stream (the context stream or a lane's)
HRESULT CHipVideoProcessor::RunBatchRoute(BatchRoutePlan &rp, BatchRun &run)
{
    const int n = run.n, rtPitch = run.rtPitch;
    const void *const *srcs = run.srcs;
    void *const *const dsts = run.dsts;
    hipStream_t const stream = run.on.stream;
    HRESULT hr = MPCVR_S_OK;
    bool started = run.started;                         // m_evStart sits in front of the batch's first launch (the repack's, if any)
    auto start = [&] { if (!started) (void)hipEventRecord(m_evStart, stream); started = true; };
    std::vector<const void *> slots;
    if (rp.repackSlot) {
        if ((hr = CheckHip(m_batchTex.CheckCreate(rp.repackSlot * n), "batch source texture"))) return hr;
        start();                                        // the repack is part of the batch's process time
        if ((hr = CheckHip(LaunchRepackV210(nullptr, m_srcPitch, (uint8_t *)m_batchTex.ptr, TexPitch(), m_srcHeight, stream, srcs, n, rp.repackSlot), "k_repack_v210"))) return hr;
        m_batchTexZeroed = false;                       // (the RGB batches' zeroed remainder columns are gone)
        slots.resize(n);
        for (int i = 0; i < n; i++) slots[i] = (uint8_t *)m_batchTex.ptr + (size_t)i * rp.repackSlot;
        srcs = slots.data();
    }
    if (run.dvFrames && (rp.route == BatchRoute::DirectConvert || rp.route == BatchRoute::WholeBatchLaunches)) {
        // one RPU per frame: the block convert indexes the run's tables by the frame (ClassifyBatch takes these routes only with the tables uploaded)
        run.usedTables = true;
        rp.direct.conv.dovi = rp.conv.conv.dovi = run.dvTab; rp.direct.dovi_cm = rp.conv.dovi_cm = run.dvCm;
    }
    SlotLease table;        // the batch's frame table, where it travels through the ring: on loan until the end of this function, behind the launches that read it
    FusedFrame rows[kHostTableMax]; LaunchFrames frames;       // ... and where it travels in the kernel arguments (BatchFrames)
    switch (rp.route) {
    case BatchRoute::DirectConvert:
        // same-size frames: one convert launch, the frame table in its kernel arguments where the kernel that takes the launch carries n rows
        if ((hr = BatchFrames(n, srcs, dsts, ConvertBlocksByValueMax(rp.direct), stream, rows, &table, &frames))) break;
        start();
        hr = CheckHip(LaunchConvertBlocks(rp.direct, frames, stream), "k_convert_blocks");
        break;
    case BatchRoute::RgbSurfaceStrip: {
        // Interleaved RGB without a convert draw (m_PSConvColorData.bEnable false, :849-853): every frame is repacked into its own slot of a
        // batch texture (the reference's CopyFrame* upload: one repack launch per 32 frames, the sample pointers in its arguments) and ONE
        // k_fused_strip:surface launch resizes the whole chunk from there, instead of a repack + a resize launch per frame
        const int tp = TexPitch();
        const size_t texBytes = (size_t)tp * m_srcHeight;
        const int chunk = FramesPerChunk(n, texBytes, (size_t)1 << 30);
        const bool fresh = m_batchTex.size < texBytes * chunk || !m_batchTex.ptr || !m_batchTexZeroed;     // (not by size alone: a v210 batch or another media type may have used it since)
        if ((hr = CheckHip(m_batchTex.CheckCreate(texBytes * chunk), "batch source texture"))) break;
        // texels the reference's copy loop never writes (RGB48 remainder) stay zero, as in PrepareSample
        if (fresh && (hr = CheckHip(hipMemsetAsync(m_batchTex.ptr, 0, texBytes * chunk, stream), "clear batch texture"))) break;
        m_batchTexZeroed = true;
        if ((hr = UploadFrameTable(n, srcs, dsts, nullptr, 0, stream, &table))) break;
        rp.strip.surf.ptr = m_batchTex.ptr;
        rp.strip.surf_stride = texBytes;
        rp.strip.fp.dst_aligned16 = rp.aligned8 ? 1 : 0;
        start();
        for (int at = 0; at < n && !hr; at += chunk) {
            const int m = std::min(chunk, n - at);
            hr = CheckHip(LaunchRepackRgb(m_srcParams->repack, nullptr, m_srcBottomUp ? -m_srcPitch : m_srcPitch, (uint8_t *)m_batchTex.ptr, tp,
                                          m_srcWidth, m_srcHeight, stream, srcs + at, m, texBytes), "k_repack_rgb");
            if (!hr) hr = CheckHip(LaunchFusedStrip(rp.strip, LaunchFrames::Device(table.frames() + at, m), stream), "k_fused_strip<surface>");
        }
        break;
    }
    case BatchRoute::StripToneMap: {
        // HDR10 tone-mapping step behind the one-kernel strip path (what a single frame of this plan runs, ProcessOne): the strip kernel draws
        // every frame of a chunk into its slot of m_batchPost (a second frame table: same samples, the slots as targets) and ONE
        // k_hdr10_tonemap launch writes the render targets (:3359-3367)
        const int w2 = m_videoRect.Width(), h2 = m_videoRect.Height();
        const size_t postStride = PostStride();
        const int chunk = FramesPerChunk(n, postStride, (size_t)4 << 30);
        if ((hr = CheckHip(m_batchPost.CheckCreate(postStride * chunk), "batch post-scale textures"))) break;
        const Surface post{m_batchPost.ptr, (int)(w2 * SurfBytesPerPixel(m_plan.internal_fmt)), w2, h2, m_plan.internal_fmt};
        rp.strip.fp.store.dst = post.ptr;
        rp.strip.fp.dst_aligned16 = 1;                         // the slots start on 256-byte boundaries
        start();
        for (int at = 0; at < n && !hr; at += chunk) {
            const int m = std::min(chunk, n - at);
            SlotLease drawTab, realTab;            // (both until the end of the chunk's two launches)
            if ((hr = UploadFrameTable(m, srcs + at, nullptr, (uint8_t *)m_batchPost.ptr, postStride, stream, &drawTab))) break;
            if ((hr = UploadFrameTable(m, srcs + at, dsts + at, nullptr, 0, stream, &realTab))) break;
            ResizeBatch tb; tb.n = m; tb.in_stride = postStride; tb.frames = realTab.frames();
            if (!(hr = CheckHip(LaunchFusedStrip(rp.strip, LaunchFrames::Device(drawTab.frames(), m), stream), "k_fused_strip")))
                hr = CheckHip(LaunchHdr10ToneMap(post, m_hdrTm, w2, h2, MakeStore(dsts[at], rtPitch, m_plan.swap_fmt, true), stream, &tb), "k_hdr10_tonemap");
        }
        break;
    }
    case BatchRoute::FrameByFrame:
        // samples that are repacked (or, not starting on a dword, copied) into m_TexSrcVideo one by one share it: frame by frame
        start();
        for (int i = 0; i < n && !hr; i++) {
            const uint8_t *tex = (const uint8_t *)srcs[i];           // (repacked: already in m_TexSrcVideo's layout, a slot of the batch texture)
            if (!rp.repackSlot && (hr = PrepareSample((const uint8_t *)srcs[i], &tex))) break;
            if (run.dvFrames && (hr = ApplyDoviFrame(run.dvFrames[i]))) break;          // this frame's RPU: constants, matrix, tone-mapping metadata
            hr = ProcessOne(tex, dsts[i], rtPitch, run.on);
        }
        break;
    case BatchRoute::WholeBatchLaunches:
        if ((hr = UploadFrameTable(n, srcs, dsts, nullptr, 0, stream, &table))) break;
        start();
        hr = ProcessBatchLaunches(run, table.frames(), rp.aligned, rp.conv);
        break;
    case BatchRoute::Strip:
        if ((hr = UploadFrameTable(n, srcs, dsts, nullptr, 0, stream, &table))) break;
        rp.strip.fp.dst_aligned16 = rp.aligned8 ? 1 : 0;
        start();
        hr = CheckHip(LaunchFusedStrip(rp.strip, LaunchFrames::Device(table.frames(), n), stream), "k_fused_strip");
        break;
    case BatchRoute::FusedUp2x: {
        FusedParams fp{};
        FillFusedParams((const uint8_t *)srcs[0], nullptr, rtPitch, &fp);
        fp.dst_aligned16 = rp.aligned ? 1 : 0;
        // the frames the exact-2x kernel carries travel in its arguments: no table copy on the stream in front of the launch and no slot event
        // behind it (the fused Jinc2m kernel, which LaunchFusedUp2x may launch instead, reads an uploaded table)
        if ((hr = BatchFrames(n, srcs, dsts, FusedUp2xByValueMax(fp), stream, rows, &table, &frames))) break;
        start();
        FusedUp2xLastForm() = -1;
        hr = CheckHip(LaunchFusedUp2x(fp, frames, stream), "k_fused_up2x");
        if (FusedUp2xLastForm() >= 0) m_up2xForm = FusedUp2xLastForm();
        break;
    }
    }
    (void)hipEventRecord(m_evStop, stream);
    m_timed = true;
    return hr;
}

// ---- EXTENSION: error-diffusion final pass (bUseDither = 2; no reference counterpart, include/mpcvr.h) -----------------------------
// The plan of such a context is the 10-bit swap chain's (DecidePlan: swap_fmt = SF_RGB10A2, no final pass for UNORM internal formats),
// so every kernel of the library — fused, batched, Dolby Vision — runs as it does for a 10-bit target; only the target differs: a
// window-sized intermediate per frame, from which k_error_diffusion writes the B8G8R8A8 render target inside video rect ∩ window.
HRESULT CHipVideoProcessor::PrepareErrDiff(int frames)
{
    m_edPitch = (m_windowRect.Width() * 4 + 255) & ~255;
    m_edStride = (size_t)m_edPitch * (size_t)m_windowRect.Height();
    // (256 bytes in front and behind: the pass reads its rows in 16-byte pieces that may start two pixels in front of a row and end three
    // behind it — inside the image that is the neighbouring row's padding, at its two ends it is this margin)
    const HRESULT hr = CheckHip(m_edPost.CheckCreate(m_edStride * (size_t)frames + 512), "error-diffusion intermediates");
    m_edBase = hr ? nullptr : (uint8_t *)m_edPost.ptr + 256;
    return hr;
}

HRESULT CHipVideoProcessor::ErrDiffPass(const LaunchFrames &frames, int rtPitch, hipStream_t s)
{
    ErrDiffParams P{};
    P.x0 = std::max((int)m_videoRect.left, 0); P.y0 = std::max((int)m_videoRect.top, 0);
    P.x1 = std::min((int)m_videoRect.right, m_windowRect.Width()); P.y1 = std::min((int)m_videoRect.bottom, m_windowRect.Height());
    if (P.x1 <= P.x0 || P.y1 <= P.y0) return MPCVR_S_OK;          // the video rect lies outside the window: nothing is drawn
    P.src_pitch = m_edPitch; P.dst_pitch = rtPitch;
    // band-major ticket order: same box, 32 frames 4K -> 8K: 3.85 k frames/s against 3.28 k frame-major (profiles/r04/ab_call24_errdiff_order.jsonl)
    static const int order = [] { const char *e = std::getenv("MPCVR_ERRDIFF_ORDER"); return e ? std::atoi(e) : 1; }();
    P.order = order;
    // (tests: a band that never publishes and a short patience, read per call — the give-up path must end in an error, not in a hang)
    const char *stall = std::getenv("MPCVR_ERRDIFF_TEST_STALL"), *spin = std::getenv("MPCVR_ERRDIFF_SPIN");
    P.test_stall = stall && *stall && *stall != '0' ? 1 : 0;
    P.spin_limit = spin && *spin ? std::atoi(spin) : m_edPatience;      // (0: the launcher's default, 2^21 polls of about a microsecond)
    HRESULT hr;
    if (!m_edStatus) {
        if ((hr = CheckHip(hipHostMalloc((void **)&m_edStatus, sizeof(int), hipHostMallocDefault), "error-diffusion status word"))) return hr;
        *m_edStatus = 0;
    }
    if (*m_edStatus) { *m_edStatus = 0; return Fail(MPCVR_E_FAIL, "error diffusion: a band of an earlier pass gave up waiting for the band above"); }
    // the hand-off rows are cleared and rewritten by every launch: launches of one context run in stream order on one buffer
    if (s != m_stream) (void)hipStreamSynchronize(m_stream);
    const size_t need = ErrorDiffusionHandoffBytes(P, frames.n);
    if ((hr = CheckHip(m_edHandoff.CheckCreate(need), "error-diffusion hand-off rows"))) return hr;
    P.handoff = (uint32_t *)m_edHandoff.ptr; P.status = m_edStatus;
    // the hand-off words carry the launch's generation: rows of the same layout need no clearing from launch to launch (600 MB for a 32-frame
    // batch of 8K frames); another layout, another buffer or a wrapped count: gen = 0 = the launcher clears them and starts at 1
    // (the layout is compared field by field — round 5 hashed it into 64 bits, and two layouts whose hashes met would have shared uncleared rows)
    const EdLayout key{P.x0, P.x1, P.y0, P.y1, frames.n, (const void *)P.handoff};
    if (!(key == m_edKey) || m_edGen >= 4095 || m_edGen <= 0 || P.test_stall) { P.gen = 0; m_edGen = 1; m_edKey = P.test_stall ? EdLayout{} : key; }
    else P.gen = ++m_edGen;
    return CheckHip(LaunchErrorDiffusion(P, frames, s), "k_error_diffusion");
}

// a validated batch of an error-diffusion plan (RunBatch): chunks of frames through the routes into the intermediates, a pass behind each
HRESULT CHipVideoProcessor::ProcessBatchErrDiff(BatchRun &run)
{
    const int n = run.n;
    HRESULT hr;
    const size_t one = ((size_t)((m_windowRect.Width() * 4 + 255) & ~255)) * (size_t)m_windowRect.Height();
    // intermediates for up to ~4 GiB of frames at a time, in chunks of equal size: the pass is a chain of dependent steps per frame and only
    // many frames side by side fill the chip (a 33-frame batch as 32 + 1 took 13.8 ms where 32 take 8.5: the odd frame ran alone)
    static const int cap = [] { const char *e = std::getenv("MPCVR_ERRDIFF_CHUNK"); return e ? std::atoi(e) : 0; }();      // (tests: chunks of a few small frames)
    int most = FramesPerChunk(n, one, (size_t)4 << 30);
    if (cap > 0) most = std::min(most, cap);
    const int chunks = (n + most - 1) / most;
    const int chunk = (n + chunks - 1) / chunks;
    if ((hr = PrepareErrDiff(chunk))) return hr;
    std::vector<void *> mids(chunk);
    for (int i = 0; i < chunk; i++) mids[i] = m_edBase + (size_t)i * m_edStride;
    // the batch's process time runs from in front of the first chunk to behind the last chunk's pass
    (void)JoinFrameLanes(false);
    (void)hipEventRecord(m_evStart, m_stream);
    for (int at = 0; at < n; at += chunk) {
        const int m = std::min(chunk, n - at);
        // the whole-batch routes of the 10-bit plan, into the intermediates (the previous chunk's pass reads them in stream order); a run of
        // ProcessBatchDovi: the chunk sees its own slice of the per-frame RPU state
        BatchRun part = run.Slice(at, m);
        part.dsts = mids.data(); part.rtPitch = m_edPitch; part.started = true;
        hr = ProcessBatchRoutes(part);
        run.usedTables = run.usedTables || part.usedTables;
        if (hr) return hr;
        SlotLease tab;
        if ((hr = UploadFrameTable(m, (const void *const *)mids.data(), run.dsts + at, nullptr, 0, m_stream, &tab))) return hr;
        if ((hr = ErrDiffPass(LaunchFrames::Device(tab.frames(), m), run.rtPitch, m_stream))) return hr;
    }
    (void)hipEventRecord(m_evStop, m_stream);       // (the batch's process time includes the pass)
    m_timed = true;
    return MPCVR_S_OK;
}

void CHipVideoProcessor::TableRing::Release()
{
    for (Slot &slot : m_slots) {
        slot.dev.Release();
        if (slot.pinned) (void)hipHostFree(slot.pinned);
        if (slot.done) (void)hipEventDestroy(slot.done);
    }
}

HRESULT CHipVideoProcessor::TableRing::Next(size_t bytes, size_t atLeast, void **pinned)
{
    Slot &slot = m_slots[m_sent % m_slots.size()];
    HRESULT hr = slot.done ? m_owner->CheckHip(hipEventSynchronize(slot.done), "table slot wait")
                           : m_owner->CheckHip(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming), "table slot event");
    if (hr) return hr;
    if (bytes > slot.cap) {
        if (slot.pinned) (void)hipHostFree(slot.pinned);
        slot.pinned = nullptr; slot.cap = 0;
        const size_t cap = std::max(bytes, atLeast);
        if ((hr = m_owner->CheckHip(hipHostMalloc(&slot.pinned, cap, hipHostMallocDefault), "table slot pinned"))) return hr;
        if ((hr = m_owner->CheckHip(slot.dev.CheckCreate(cap), "table slot"))) return hr;
        slot.cap = cap;
    }
    *pinned = slot.pinned;
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::TableRing::Send(size_t bytes, hipStream_t stream, const char *what, SlotLease *lease)
{
    Slot &slot = m_slots[m_sent % m_slots.size()];
    *lease = SlotLease(slot.dev.ptr, slot.done, stream);
    if (HRESULT hr = m_owner->CheckHip(hipMemcpyAsync(slot.dev.ptr, slot.pinned, bytes, hipMemcpyHostToDevice, stream), what)) return hr;
    m_sent++;
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::UploadFrameTable(int n, const void *const *srcs, void *const *dsts, uint8_t *dst_base, size_t dst_stride, hipStream_t stream, SlotLease *lease)
{
    return m_tableRing.SendRows<FusedFrame>(n, stream, "frame table", lease, [&](FusedFrame *fr) {
        for (int i = 0; i < n; i++) { fr[i].src = srcs ? (const uint8_t *)srcs[i] : nullptr; fr[i].dst = dsts ? dsts[i] : (void *)(dst_base + (size_t)i * dst_stride); }
    });
}

// The frames of a whole-batch launch that takes byValueMax rows in its kernel arguments (the launcher's own answer: ConvertBlocksByValueMax,
// FusedUp2xByValueMax): up to that many go into `rows` (the caller's, kHostTableMax of them) and nothing is queued; more go through the table ring
HRESULT CHipVideoProcessor::BatchFrames(int n, const void *const *srcs, void *const *dsts, int byValueMax, hipStream_t stream, FusedFrame *rows, SlotLease *lease, LaunchFrames *frames)
{
    if (n <= byValueMax) {
        for (int i = 0; i < n; i++) rows[i] = FusedFrame{(const uint8_t *)srcs[i], dsts[i]};
        *frames = LaunchFrames::Host(rows, n);
        return MPCVR_S_OK;
    }
    const HRESULT hr = UploadFrameTable(n, srcs, dsts, nullptr, 0, stream, lease);
    if (!hr) *frames = LaunchFrames::Device(lease->frames(), n);
    return hr;
}

// The exact-2x kernel's tables as it keeps them in LDS, computed once per plan instead of by every workgroup of every launch
// (vp_launch.h has the layout).  The expressions are the kernel prologue's own, in the same fp32 operations; the float -> unsigned
// conversion saturates as v_cvt_u32_f32 does, so a dither table from a parameter blob gives the same words whatever it holds.
void BakeFusedTables(const uint16_t *dither, const float *lut, void *out)
{
    auto half_bits_to_float = [](uint16_t h) {
        const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
        float mag;
        if (e == 31) { uint32_t b = 0x7f800000u | (m << 13); std::memcpy(&mag, &b, 4); }
        else if (e == 0) mag = (float)m * (1.0f / 16777216.0f);                     // subnormal: m * 2^-24, exact
        else { uint32_t b = ((e + 112u) << 23) | (m << 13); std::memcpy(&mag, &b, 4); }
        uint32_t b;
        std::memcpy(&b, &mag, 4);
        b |= sign;
        std::memcpy(&mag, &b, 4);
        return mag;
    };
    unsigned char *o = (unsigned char *)out;
    uint16_t *D = (uint16_t *)o;
    uint32_t *Di = (uint32_t *)(o + 1024 * 2);
    float *T = (float *)(o + kBakedDitherBytes);
    for (int i = 0; i < 1024; i++) {
        D[i] = dither[i];
        const float x = half_bits_to_float(dither[i]) * 1024.0f + 0.5f;
        const uint32_t j = x >= 4294967296.0f ? 0xffffffffu : x > 0.0f ? (uint32_t)x : 0u;       // (a NaN gives 0)
        Di[i] = j << 14;
    }
    for (int i = 0; i < kPqLutSize; i++) {
        const float v = lut ? lut[i] : 0.0f, n = lut ? lut[std::min(i + 1, kPqLutSize - 1)] : 0.0f;
        T[2 * i] = v;
        T[2 * i + 1] = n - v;
    }
}

HRESULT CHipVideoProcessor::UploadFusedTables()
{
    m_fusedTabValid = false;
    const float *host = nullptr;
    m_fusedTabLut = nullptr;
    if (m_tail == TAIL_PQ_TO_SDR && m_pqLutValid) { host = m_pqLutHost; m_fusedTabLut = (const float *)m_pqLut.ptr; }
    else if (m_tail == TAIL_HLG_TO_SDR && m_hlgLut.ptr && m_hlgLutHost.size() == (size_t)kPqLutSize) { host = m_hlgLutHost.data(); m_fusedTabLut = (const float *)m_hlgLut.ptr; }
    m_fusedTabHost.resize(kBakedTableBytes);
    BakeFusedTables(m_ditherHost, host, m_fusedTabHost.data());
    HRESULT hr;
    if ((hr = CheckHip(m_fusedTab.CheckCreate(kBakedTableBytes), "fused tables"))) return hr;
    if ((hr = CheckHip(hipMemcpy(m_fusedTab.ptr, m_fusedTabHost.data(), kBakedTableBytes, hipMemcpyHostToDevice), "fused tables upload"))) return hr;
    m_fusedTabValid = true;
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::GetFusedTables(void *buf, size_t *size)
{
    if (!size) return Fail(MPCVR_E_POINTER, "null size");
    if (!m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (!buf) { *size = kBakedTableBytes; return MPCVR_S_OK; }
    if (*size < (size_t)kBakedTableBytes) { *size = kBakedTableBytes; return Fail(MPCVR_E_INVALIDARG, "buffer too small"); }
    HRESULT hr;
    if (m_planDirty && (hr = UpdatePlan())) return hr;
    if (!m_fusedTabValid) return Fail(MPCVR_E_NOT_VALID_STATE, "no baked tables");
    std::memcpy(buf, m_fusedTabHost.data(), kBakedTableBytes);
    *size = kBakedTableBytes;
    return MPCVR_S_OK;
}

// Can this plan run as whole-batch launches?  *conv: the block convert into the (batched) convert output, its target set per chunk by
// ProcessBatchLaunches; *direct: the block convert straight into the render targets (same-size frames).  Exactly one of them is filled.
// repacked: the samples are v210 slots of m_batchTex; src16: every sample starts on a 16-byte boundary.
bool CHipVideoProcessor::BatchPlan(const uint8_t *sample0, void *rt0, int rtPitch, bool aligned, bool repacked, bool src16, FusedParams *conv, FusedParams *direct) const
{
    // every draw kernel has a frame dimension (round 4: the one-kernel-fits-all k_resize / k_jinc2 too — quarter turns, flips outside the
    // strip kernels' reach, the two-draw Jinc2m), so what decides is the convert stage: the 2x2-block kernel must take the sample
    if (!m_plan.convert) return false;
    if ((m_srcParams->cformat == MPCVR_CF_V210 && !repacked) || m_srcParams->layout == LAY_RGB) return false;
    if (m_plan.direct_convert) {
        FillFusedParams(sample0, rt0, rtPitch, direct);
        direct->dst_aligned16 = aligned ? 1 : 0;
        direct->src_aligned16 = src16 ? 1 : 0;
        return ConvertBlocksSupported(*direct, true);
    }
    // with the HDR10 tone-mapping step (:3359-3367) the draws go into the frames' post-scale textures (m_batchPost, internal format)
    // and one tone-mapping launch writes the render targets; without a resize the step reads the convert outputs
    if (!m_plan.two_pass && !m_plan.one_pass && !m_plan.hdr_tonemap) return false;
    *conv = ConvertOutputParams(sample0, nullptr);
    conv->src_aligned16 = src16 ? 1 : 0;
    return ConvertBlocksSupported(*conv, false);
}

// convert all -> first draw all -> second draw all, a frame dimension in every grid; the intermediates hold `chunk` frames
HRESULT CHipVideoProcessor::ProcessBatchLaunches(const BatchRun &run, const FusedFrame *table, bool aligned, FusedParams conv)
{
    const int n = run.n;
    HRESULT hr;
    // intermediates for up to `chunk` frames (at most ~4 GiB)
    const bool hdr = m_plan.hdr_tonemap;
    const size_t postStride = hdr ? PostStride() : 0;
    const size_t per = m_convBytes + m_midBytes + postStride;
    const int chunk = FramesPerChunk(n, per, (size_t)4 << 30);
    if ((hr = CheckHip(m_batchConv.CheckCreate(m_convBytes * chunk), "batch convert output"))) return hr;
    if (m_midBytes && (hr = CheckHip(m_batchMid.CheckCreate(m_midBytes * chunk), "batch resize texture"))) return hr;
    if (hdr && (hr = CheckHip(m_batchPost.CheckCreate(postStride * chunk), "batch post-scale textures"))) return hr;
    DrawFrames df{m_batchConv.ptr, m_batchMid.ptr, m_batchPost.ptr, m_convBytes, m_midBytes, postStride};
    // HDR10 tone-mapping step: the draws write frame z's post-scale texture (a second frame table whose targets are the slots of
    // m_batchPost), then ONE k_hdr10_tonemap launch per chunk writes the render targets (:3359-3367)
    SlotLease postTab;
    if (hdr) {
        if ((hr = UploadFrameTable(chunk, nullptr, nullptr, (uint8_t *)m_batchPost.ptr, postStride, run.on.stream, &postTab))) return hr;
        df.lastTab = postTab.frames();
        aligned = true;             // the slots of m_batchPost start on 256-byte boundaries
    }
    df.aligned = aligned ? 1 : 0;
    for (int at = 0; at < n; at += chunk) {
        const int m = std::min(chunk, n - at);
        // frame z of the chunk: sample from the table, output at m_batchConv + z * m_convBytes
        conv.store.dst = m_batchConv.ptr;
        const BatchRun part = run.Slice(at, m);
        if (part.dvTab) { conv.conv.dovi = part.dvTab; conv.dovi_cm = part.dvCm; }       // (the chunk's slice of the per-frame RPU tables)
        if ((hr = CheckHip(LaunchConvertBlocks(conv, LaunchFrames::Device(table + at, m), run.on.stream, m_convBytes), "k_convert_blocks"))) return hr;
        df.n = m;
        df.rtTab = table + at;
        if (!hdr) df.lastTab = df.rtTab;
        if ((hr = ResizeShaderPass(nullptr, run.dsts[0], run.rtPitch, df, run.on))) return hr;
    }
    return MPCVR_S_OK;
}

// ---- a batch with one Dolby Vision RPU per frame -------------------------------------------------------------------------------
// The reference reads the RPU of every sample in CopySample (IID_MediaSideDataDOVIMetadataV2, :2270-2520) and rebuilds the constant
// buffers when it differs from the previous one.  Here: rpus[i] is applied in front of frame i exactly as SetDoviMetadata would
// (level-1 / level-2 blocks stay as last seen until Flush), the frames are cut into runs that share a plan and a kernel variant
// (level-2 trims present or not), and a run goes through ProcessBatch — ONE launch per stage where the block convert's Dolby Vision
// variants take it (they index a table of DoviParams and colour matrices by the frame), frame by frame with the RPU's constants
// uploaded in stream order otherwise.  The context is left as after the last frame's SetDoviMetadata.
void CHipVideoProcessor::SaveDoviWalk(DoviWalkState *s) const
{
    s->valid = m_doviValid; s->l1Present = m_doviL1Present; s->l2Present = m_doviL2Present; s->blobOverride = m_blobOverride; s->planDirty = m_planDirty;
    s->md = m_doviMd; s->host = m_doviHost;
    std::memcpy(s->l1, m_doviL1, sizeof(m_doviL1)); std::memcpy(s->l2raw, m_doviL2Raw, sizeof(m_doviL2Raw)); std::memcpy(s->cm, m_cm, sizeof(m_cm));
    s->tail = m_tail; s->gamma = m_gamma; s->tm = m_hdrTm;
}
void CHipVideoProcessor::RestoreDoviWalk(const DoviWalkState &s)
{
    m_doviValid = s.valid; m_doviL1Present = s.l1Present; m_doviL2Present = s.l2Present; m_blobOverride = s.blobOverride; m_planDirty = s.planDirty;
    m_doviMd = s.md; m_doviHost = s.host;
    std::memcpy(m_doviL1, s.l1, sizeof(m_doviL1)); std::memcpy(m_doviL2Raw, s.l2raw, sizeof(m_doviL2Raw)); std::memcpy(m_cm, s.cm, sizeof(m_cm));
    m_tail = s.tail; m_gamma = s.gamma; m_hdrTm = s.tm;
}

HRESULT CHipVideoProcessor::ApplyDoviFrame(const DoviFrameState &f)
{
    m_doviHost = f.p;
    std::memcpy(m_cm, f.cm, sizeof(m_cm));
    m_hdrTm = f.tm;
    return UploadDoviParams();          // through the pinned ring, in stream order: the frames before this one read their own copy
}

// DoviParams[n] followed by cm[12 n], through the ring of two slots (ProcessBatchDovi keeps the lease until the run is queued); fills run->dvTab / dvCm
HRESULT CHipVideoProcessor::UploadDoviTables(BatchRun *run, hipStream_t stream, SlotLease *lease)
{
    const int n = run->n;
    const size_t each = sizeof(DoviParams) + 12 * sizeof(float), need = each * n;
    DoviParams *tp;
    if (HRESULT hr = m_dvTableRing.Next(need, each * 64, (void **)&tp)) return hr;
    float *tc = (float *)(tp + n);
    for (int i = 0; i < n; i++) {
        tp[i] = run->dvFrames[i].p;
        std::memcpy(tc + (size_t)12 * i, run->dvFrames[i].cm, 12 * sizeof(float));
    }
    if (HRESULT hr = m_dvTableRing.Send(need, stream, "dovi tables upload", lease)) return hr;
    run->dvTab = (const DoviParams *)lease->dev;
    run->dvCm = (const float *)(run->dvTab + n);
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::ProcessBatchDovi(int n, const void *const *srcs, void *const *dsts, int rtPitch, const mpcvr_dovi_metadata *rpus)
{
    const BatchRecord record(*this, n);
    if (HRESULT bad = CheckBatchArgs(n, rpus ? srcs : nullptr, dsts, rtPitch)) return bad;       // (no RPUs: an empty batch, like no samples)
    for (int i = 0; i < n; i++)         // all or nothing: no frame is drawn when one RPU of the batch is malformed
        if (!CheckDoviCurves(rpus[i])) return Fail(MPCVR_E_INVALIDARG, "Dolby Vision curves: num_pivots outside [2,9], mapping_idc > 1 or more than 32 level-2 blocks");
    (void)hipSetDevice(m_device);
    HRESULT hr = MPCVR_S_OK;
    std::vector<DoviFrameState> fs((size_t)n);
    auto collect = [&](int i) { fs[i].p = m_doviHost; std::memcpy(fs[i].cm, m_cm, sizeof(m_cm)); fs[i].tm = m_hdrTm; };
    DoviWalkState back;
    for (int i = 0; i < n && !hr;) {
        // frame i opens a run: its RPU may change the plan (the first RPU of a stream, level-1 data switching the tone mapping on)
        if ((hr = ApplyDoviMetadata(&rpus[i]))) break;
        if (m_planDirty && (hr = UpdatePlan())) break;
        collect(i);
        if ((hr = UploadDoviParams())) break;           // (the context's own copy and, at the first RPU of a stream, the PQ EOTF table exist from here on)
        int j = i + 1;
        for (; j < n; j++) {
            SaveDoviWalk(&back);
            if ((hr = ApplyDoviMetadata(&rpus[j]))) break;
            if (m_planDirty || m_doviHost.l2_enabled != fs[i].p.l2_enabled) { RestoreDoviWalk(back); break; }      // frame j opens the next run
            collect(j);
        }
        if (hr) break;
        const int len = j - i;
        BatchRun run{len, srcs + i, dsts + i, rtPitch, fs.data() + i};
        SlotLease tables;           // (until the run is queued)
        if (len > 1 && !m_plan.hdr_tonemap) hr = UploadDoviTables(&run, m_stream, &tables);       // (a run with RPUs stays on the context stream: BatchLaneEligible)
        if (!hr) hr = RunBatch(run);
        m_dvLastInfo += (m_dvLastInfo.empty() ? "" : ",") + std::to_string(len) + (run.usedTables ? ":tables" : ":frames");
        // the context's own copy of the constants: the run's last frame (a whole-batch route did not touch it)
        if (!hr && run.usedTables) hr = UploadDoviParams();
        i = j;
    }
    return hr;
}

// how the last mpcvr_process_batch[_dovi] call ran: "frames=<n>;launches=<kernel launches>;lane=<lane>;waits=<writers on other lanes it was ordered behind>;uploads=<frame tables copied to the device>[;dovi_runs=<frames>:<tables|frames>,...]" —
// a batch on a whole-batch route launches a handful of kernels whatever n is, a frame-by-frame one at least n
std::string CHipVideoProcessor::GetLastBatchInfo() const
{
    std::string s = "frames=" + std::to_string(m_lastBatchFrames) + ";launches=" + std::to_string(m_lastBatchLaunches) + ";lane=" + std::to_string(m_lastBatchLane) + ";waits=" + std::to_string(m_lastBatchWaits) +
                    ";uploads=" + std::to_string(m_lastBatchUploads);
    if (!m_dvLastInfo.empty()) s += ";dovi_runs=" + m_dvLastInfo;
    if (m_up2xForm >= 0) s += m_up2xForm == 1 ? ";up2x=bp" : ";up2x=generic";      // the exact-2x kernel's form (vp_fused_up2x_bp.h)
    s += m_yuvLastInfo;            // (";yuv_chunks=..;yuv_lanes=.." behind a ProcessBatchYuv, ";tensor_chunks=..;tensor_lanes=.." behind a ProcessBatchTensor, empty otherwise)
    return s;
}

// Render minus Present — DX11VideoProcessor.cpp:2599-2813
HRESULT CHipVideoProcessor::RenderBackBuffer(bool onContextStream)
{
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (!m_curSample) return MPCVR_S_FALSE;          // nothing to draw (cf. :2603-2606)
    (void)hipSetDevice(m_device);
    const int w = m_windowRect.Width(), h = m_windowRect.Height();
    const size_t bytes = (size_t)w * 4 * h;
    HRESULT hr;
    const bool fresh = m_BackBuffer.size < bytes || !m_BackBuffer.ptr;
    if ((hr = CheckHip(m_BackBuffer.CheckCreate(bytes), "back buffer"))) return hr;
    // ClearRenderTargetView to black (:2622) — only the letterbox area survives Process
    const size_t clearBytes = (fresh || m_videoRect != CRect(0, 0, w, h)) ? bytes : 0;     // queued on the stream the frame runs on
    hr = ProcessFrame(m_BackBuffer.ptr, w * 4, nullptr, nullptr, clearBytes, onContextStream);
    if (hr >= 0) { m_backW = w; m_backH = h; m_backFmt = m_cfg.output_format; }        // what GetDisplayedImage will find there
    return hr;
}

HRESULT CHipVideoProcessor::GetBackBuffer(void **ptr, int *pitch, int *w, int *h)
{
    if (!m_BackBuffer.ptr) return Fail(MPCVR_E_NOT_VALID_STATE, "Render has not been called");
    if (ptr) *ptr = m_BackBuffer.ptr;
    if (pitch) *pitch = m_windowRect.Width() * 4;
    if (w) *w = m_windowRect.Width();
    if (h) *h = m_windowRect.Height();
    return MPCVR_S_OK;
}

// GetDisplayedImage — DX11VideoProcessor.cpp:3610-3683: the back buffer as it was last rendered (no new draw), copied to host memory as the
// pixels of a top-down DIB: B8G8R8A8 as it is (CopyPlaneAsIs); R10G10B10A2 as BGR32 through ConvertR10G10B10A2toBGR32 (Helper.cpp:805-834:
// the top eight bits of each channel, X = 0xff) or, with m_bAllowDeepColorBitmaps, as BGR48 (ConvertR10G10B10A2toBGR48, :836-857: the ten
// bits in the top of each 16-bit word).  Rows are CalcDibRowPitch(width, bits) apart.  The BITMAPINFOHEADER and the LocalAlloc block the
// reference puts around the pixels are the caller's (the adapter's): host_pixels == NULL reports the size and the header's fields.
HRESULT CHipVideoProcessor::GetDisplayedImage(void *hostPixels, size_t *size, bool deepColor, int *width, int *height, int *bits)
{
    if (!size) return Fail(MPCVR_E_POINTER, "null size");
    if (!m_BackBuffer.ptr || m_backW <= 0 || m_backH <= 0) return Fail(MPCVR_E_NOT_VALID_STATE, "Render has not been called");     // (E_ABORT without a swap chain, :3612-3614)
    const int w = m_backW, h = m_backH;
    const bool ten = m_backFmt == MPCVR_OUT_RGB10A2;
    const int bpp = (ten && deepColor) ? 48 : 32;
    const size_t dibPitch = (((size_t)w * bpp + 31) & ~(size_t)31) / 8, need = dibPitch * h;      // CalcDibRowPitch
    if (width) *width = w;
    if (height) *height = h;
    if (bits) *bits = bpp;
    if (!hostPixels) { *size = need; return MPCVR_S_OK; }
    if (*size < need) { *size = need; return Fail(MPCVR_E_INVALIDARG, "buffer too small"); }
    HRESULT hr = Synchronize();                     // frames still on the lanes / the context stream write the buffer
    if (hr) return hr;
    const size_t srcPitch = (size_t)w * 4;
    if (!ten) {                                     // 32 bits per pixel: the DIB pitch is the back buffer's
        if ((hr = CheckHip(hipMemcpy(hostPixels, m_BackBuffer.ptr, need, hipMemcpyDeviceToHost), "displayed image read-back"))) return hr;
    } else {
        std::vector<uint32_t> staging((size_t)w * h);
        if ((hr = CheckHip(hipMemcpy(staging.data(), m_BackBuffer.ptr, srcPitch * h, hipMemcpyDeviceToHost), "displayed image read-back"))) return hr;
        for (int y = 0; y < h; y++) {
            const uint32_t *src = staging.data() + (size_t)y * w;
            uint8_t *row = (uint8_t *)hostPixels + (size_t)y * dibPitch;
            if (bpp == 32) {
                uint32_t *d = (uint32_t *)row;
                for (int x = 0; x < w; x++) {
                    const uint32_t t = src[x];
                    d[x] = ((t & 0x3fc00000u) >> 22) | ((t & 0x000ff000u) >> 4) | ((t & 0x000003fcu) << 14) | 0xff000000u;
                }
            } else {
                uint16_t *d = (uint16_t *)row;
                for (int x = 0; x < w; x++) {
                    const uint32_t t = src[x];
                    *d++ = (uint16_t)((t & 0x3ff00000u) >> 14); *d++ = (uint16_t)((t & 0x000ffc00u) >> 4); *d++ = (uint16_t)((t & 0x000003ffu) << 6);
                }
            }
        }
    }
    *size = need;
    return MPCVR_S_OK;
}

// GetCurentImage — DX11VideoProcessor.cpp:3493-3608
HRESULT CHipVideoProcessor::GetCurentImage(void *hostBGRA, size_t *size)
{
    if (!size) return Fail(MPCVR_E_POINTER, "null size");
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    int w = m_srcRectWidth, h = m_srcRectHeight;            // no anamorphic sources here (m_srcAnamorphic :3497-3499)
    if (m_iRotation == 90 || m_iRotation == 270) std::swap(w, h);     // :3500-3502
    const size_t need = (size_t)w * 4 * h;
    if (!hostBGRA) { *size = need; return MPCVR_S_OK; }
    if (*size < need) { *size = need; return Fail(MPCVR_E_INVALIDARG, "buffer too small"); }
    if (!m_curSample) return Fail(MPCVR_E_NOT_VALID_STATE, "no sample");
    (void)hipSetDevice(m_device);
    HRESULT hr;
    if ((hr = CheckHip(m_Snapshot.CheckCreate(need), "snapshot"))) return hr;
    // temporarily point video/window rect at the image (:3549-3553), B8G8R8X8 target (:3518)
    const CRect backupVid = m_videoRect, backupWnd = m_windowRect;
    const int backupOut = m_cfg.output_format;
    // an HDR source shown in HDR is snapshot as SDR: m_bHdrPassthrough / m_bHdrLocalToneMapping are cleared around the draw and
    // the convert shader rebuilt with the PQ / HLG -> SDR tail (:3530-3545, restored :3562-3580)
    const bool backupHdr = m_hdrOutput;
    const bool backupOverride = m_blobOverride;
    // a context running on rank 0's broadcast parameter blob keeps it: the whole block is saved and put back verbatim (recomputing
    // the parameters locally and then claiming "overridden" again would silently drop the blob's matrices, tail and tables)
    struct { float cm[12]; float lum; float gamut[9]; int tail; float gamma; Up2xWeights ux, uy; } keep{};
    std::vector<uint16_t> keepDither;
    std::vector<float> keepLut;
    if (m_hdrOutput && backupOverride) {
        std::memcpy(keep.cm, m_cm, sizeof(m_cm)); keep.lum = m_lumScale; std::memcpy(keep.gamut, m_gamut, sizeof(m_gamut));
        keep.tail = m_tail; keep.gamma = m_gamma; keep.ux = m_upX; keep.uy = m_upY;
        keepDither.assign(m_ditherHost, m_ditherHost + sizeof(m_ditherHost) / sizeof(m_ditherHost[0]));
        keepLut.assign(m_pqLutHost, m_pqLutHost + sizeof(m_pqLutHost) / sizeof(m_pqLutHost[0]));
    }
    if (m_hdrOutput) { m_hdrOutput = false; m_blobOverride = false; SetShaderConvertColorParams(); UpdateHdrToneMapParams(); }
    m_videoRect = CRect(0, 0, w, h); m_windowRect = m_videoRect; m_cfg.output_format = MPCVR_OUT_BGRA8;
    m_planDirty = true;
    hr = ProcessFrame(m_Snapshot.ptr, w * 4, nullptr, nullptr, 0, true);     // (off the lanes: the read-back below follows on the context stream)
    m_videoRect = backupVid; m_windowRect = backupWnd; m_cfg.output_format = backupOut;
    if (backupHdr) {
        m_hdrOutput = true; SetShaderConvertColorParams(); UpdateHdrToneMapParams();
        if (backupOverride) {
            std::memcpy(m_cm, keep.cm, sizeof(m_cm)); m_lumScale = keep.lum; std::memcpy(m_gamut, keep.gamut, sizeof(m_gamut));
            m_tail = keep.tail; m_gamma = keep.gamma; m_upX = keep.ux; m_upY = keep.uy;
            std::memcpy(m_ditherHost, keepDither.data(), sizeof(m_ditherHost));
            std::memcpy(m_pqLutHost, keepLut.data(), sizeof(m_pqLutHost));
            m_blobOverride = true;
        }
    }
    m_planDirty = true;
    if (hr) return hr;
    if (!m_evRb0 && ((hr = CheckHip(hipEventCreate(&m_evRb0), "read-back timer")) || (hr = CheckHip(hipEventCreate(&m_evRb1), "read-back timer")))) return hr;
    (void)hipEventRecord(m_evRb0, m_stream);
    if ((hr = CheckHip(hipMemcpyAsync(hostBGRA, m_Snapshot.ptr, need, hipMemcpyDeviceToHost, m_stream), "readback"))) return hr;
    (void)hipEventRecord(m_evRb1, m_stream);
    m_rbTimed = true;
    if ((hr = CheckHip(hipStreamSynchronize(m_stream), "readback sync"))) return hr;
    // (the error-diffusion pass's give-up flag: a snapshot is a result handed back, it must not carry a broken frame with S_OK)
    if (m_edStatus && *m_edStatus) { *m_edStatus = 0; return Fail(MPCVR_E_FAIL, "error diffusion: a band gave up waiting for the band above"); }
    *size = need;
    return MPCVR_S_OK;
}

void CHipVideoProcessor::Flush()
{
    if (m_bInit) { (void)hipSetDevice(m_device); (void)JoinFrameLanes(true); (void)hipStreamSynchronize(m_stream); }
    m_curSample = nullptr;
    // m_DoviExtensionMetadata = {} (:4082): L1 / L2 are forgotten; the uploaded constants change with the next RPU
    m_doviL1Present = m_doviL2Present = false;
    std::memset(m_doviL1, 0, sizeof(m_doviL1));
}

HRESULT CHipVideoProcessor::Reset()
{
    Flush();
    m_planDirty = true;
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::GetParamBlob(void *buf, size_t *size)
{
    if (!size) return Fail(MPCVR_E_POINTER, "null size");
    if (!m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (!buf) { *size = sizeof(ParamBlob); return MPCVR_S_OK; }
    if (*size < sizeof(ParamBlob)) { *size = sizeof(ParamBlob); return Fail(MPCVR_E_INVALIDARG, "buffer too small"); }
    HRESULT hr;
    if (m_planDirty && (hr = UpdatePlan())) return hr;
    ParamBlob b{};
    b.magic = kBlobMagic; b.version = 1;
    std::memcpy(b.cm, m_cm, sizeof(m_cm));
    b.lum_scale = m_lumScale;
    std::memcpy(b.gamut, m_gamut, sizeof(m_gamut));
    b.tail = m_tail; b.gamma = m_gamma;
    b.upx = m_upX; b.upy = m_upY;
    std::memcpy(b.dither, m_ditherHost, sizeof(m_ditherHost));
    if (m_tail == TAIL_PQ_TO_SDR) BuildPqSdrLut(m_lumScale, b.pq_lut);
    std::memcpy(buf, &b, sizeof(b));
    *size = sizeof(b);
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::SetParamBlob(const void *buf, size_t size)
{
    if (!buf) return Fail(MPCVR_E_POINTER, "null blob");
    if (size < sizeof(ParamBlob)) return Fail(MPCVR_E_INVALIDARG, "blob too small");
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    ParamBlob b;
    std::memcpy(&b, buf, sizeof(b));
    if (b.magic != kBlobMagic || b.version != 1) return Fail(MPCVR_E_INVALIDARG, "bad blob magic/version");
    // the blob crosses a process boundary (rank 0's broadcast): nothing in it is trusted to index or select kernels unchecked
    if (b.tail < TAIL_NONE || b.tail > TAIL_HLG_TO_PQ) return Fail(MPCVR_E_INVALIDARG, "blob: tail kind out of range");
    for (const Up2xWeights *w : {&b.upx, &b.upy})
        if ((w->ntaps != 0 && w->ntaps != 4 && w->ntaps != 6) || (w->q1_quirk != 0 && w->q1_quirk != 1))
            return Fail(MPCVR_E_INVALIDARG, "blob: phase-weight table malformed");
    if (!(b.lum_scale > 0.0f) || !(b.gamma > 0.0f || b.tail != TAIL_GAMMA_GAMUT)) return Fail(MPCVR_E_INVALIDARG, "blob: luminance scale / gamma");
    (void)hipSetDevice(m_device);
    std::memcpy(m_cm, b.cm, sizeof(m_cm));
    m_lumScale = b.lum_scale;
    std::memcpy(m_gamut, b.gamut, sizeof(m_gamut));
    m_tail = b.tail; m_gamma = b.gamma;
    m_upX = b.upx; m_upY = b.upy;
    std::memcpy(m_ditherHost, b.dither, sizeof(m_ditherHost));
    std::memcpy(m_pqLutHost, b.pq_lut, sizeof(m_pqLutHost));
    HRESULT hr;
    if ((hr = CheckHip(hipStreamSynchronize(m_stream), "sync"))) return hr;
    if ((hr = CheckHip(hipMemcpy(m_dither.ptr, m_ditherHost, sizeof(m_ditherHost), hipMemcpyHostToDevice), "dither upload"))) return hr;
    m_blobOverride = true;
    m_planDirty = true;
    return MPCVR_S_OK;
}

// ---- RCCL ----
// The library does not link librccl: a host that never broadcasts never loads it.  The communicator comes from the host, so the
// host's RCCL is already mapped when these entry points are called; it is looked up (RTLD_NOLOAD first: torch ships its own copy)
// and only loaded from the default search path when the process has none yet.  Prototypes as in rccl.h (ncclResult_t = int, ncclChar = 0).
namespace {
struct RcclApi {
    int (*Broadcast)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool ok = false;
};
const RcclApi &Rccl()
{
    static const RcclApi api = [] {
        RcclApi a;
        void *h = nullptr;
        for (const char *name : {"librccl.so.1", "librccl.so"})
            if (!h) h = dlopen(name, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
            if (!h) h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (!h) return a;
        a.Broadcast = (decltype(a.Broadcast))dlsym(h, "ncclBroadcast");
        a.GetErrorString = (decltype(a.GetErrorString))dlsym(h, "ncclGetErrorString");
        a.ok = a.Broadcast != nullptr;
        return a;
    }();
    return api;
}
}  // namespace

HRESULT CHipVideoProcessor::BroadcastParamBlobBegin(void *ncclComm, int root, int rank)
{
    if (!m_bInit || !m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (!ncclComm) return Fail(MPCVR_E_POINTER, "null RCCL communicator");
    if (m_bcastPending) return Fail(MPCVR_E_NOT_VALID_STATE, "a parameter-blob broadcast is already in flight");
    const RcclApi &R = Rccl();
    if (!R.ok) return Fail(MPCVR_E_FAIL, std::string("librccl.so could not be loaded: ") + (dlerror() ? dlerror() : "ncclBroadcast not found"));
    (void)hipSetDevice(m_device);
    HRESULT hr;
    if ((hr = CheckHip(m_bcast.CheckCreate(sizeof(ParamBlob)), "broadcast buffer"))) return hr;
    m_bcastIsRoot = rank == root;
    if (m_bcastIsRoot) {
        m_bcastHost.resize(sizeof(ParamBlob));
        size_t size = m_bcastHost.size();
        if ((hr = GetParamBlob(m_bcastHost.data(), &size))) return hr;
        if ((hr = CheckHip(hipMemcpyAsync(m_bcast.ptr, m_bcastHost.data(), sizeof(ParamBlob), hipMemcpyHostToDevice, m_stream), "blob upload"))) return hr;
    }
    const int rc = R.Broadcast(m_bcast.ptr, m_bcast.ptr, sizeof(ParamBlob), /* ncclChar */ 0, root, ncclComm, m_stream);
    if (rc != 0) return Fail(MPCVR_E_FAIL, std::string("ncclBroadcast: ") + (R.GetErrorString ? R.GetErrorString(rc) : "error"));
    m_bcastPending = true;
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::BroadcastParamBlobEnd()
{
    if (!m_bcastPending) return Fail(MPCVR_E_NOT_VALID_STATE, "no parameter-blob broadcast in flight");
    (void)hipSetDevice(m_device);
    m_bcastPending = false;
    HRESULT hr;
    if (m_bcastIsRoot) return CheckHip(hipStreamSynchronize(m_stream), "broadcast sync");
    m_bcastHost.resize(sizeof(ParamBlob));
    if ((hr = CheckHip(hipMemcpyAsync(m_bcastHost.data(), m_bcast.ptr, sizeof(ParamBlob), hipMemcpyDeviceToHost, m_stream), "blob download"))) return hr;
    if ((hr = CheckHip(hipStreamSynchronize(m_stream), "broadcast sync"))) return hr;
    return SetParamBlob(m_bcastHost.data(), m_bcastHost.size());
}

HRESULT CHipVideoProcessor::GetColorMatrix(float out[12])
{
    if (!m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    std::memcpy(out, m_cm, sizeof(m_cm));
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::GetExtFmt(uint32_t *v)
{
    if (!m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    *v = m_srcExFmt.value;
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::GetFrameBytes(size_t *bytes, int *pitch)
{
    if (!m_srcParams) return Fail(MPCVR_E_NOT_VALID_STATE, "InitMediaType has not been called");
    if (bytes) *bytes = (size_t)m_srcPitch * m_srcLines;
    if (pitch) *pitch = m_srcPitch;
    return MPCVR_S_OK;
}

std::string CHipVideoProcessor::GetPathInfo()
{
    if (!m_srcParams) return "uninitialised";
    if (m_planDirty && UpdatePlan() != MPCVR_S_OK) return "error: " + m_lastError;
    if (m_fusedAside) {     // the last frame / batch went past the plan's fused kernel (a per-call condition failed): what ran is the pass-per-kernel plan
        PassPlan p = m_plan;
        p.fused_up2x = p.fused_jinc = false;
        return p.describe();
    }
    if ((!m_strip && !m_stripSurf) || m_plan.fused_up2x) return m_plan.describe();
    if ((m_strip || m_stripSurf) && (m_stripRan >= 0 ? m_stripRan == 1 : m_period))
        return m_plan.describe() + (m_strip ? ";kernel=fused_period(rows=" : ";kernel=fused_period:surface(rows=") + std::to_string(m_tables.period.P) + ":" + std::to_string(m_tables.period.Q) + ",taps=" + std::to_string(m_tables.period.nt) + ",px_per_lane=2,strip=" + std::to_string(m_tables.period.strip_w) + ",window=6 rows in registers)";
    return m_plan.describe() + (m_strip ? ";kernel=fused_strip(taps=" : ";kernel=fused_strip:surface(taps=") + std::to_string(m_tables.strip.nt) + ",px_per_lane=" + std::to_string(m_tables.strip.pxl) +
           ",strip=" + std::to_string(m_tables.strip.strip_w) + ",ring=" + std::to_string(m_tables.strip.ring) + ")";
}

// FrameStats.h:145-173: copyticks (:2594), paintticks (:2790) and the snapshot's read-back; -1 = not timed yet
HRESULT CHipVideoProcessor::GetLastTimings(float *copy_host_ms, float *upload_ms, float *process_ms, float *readback_ms)
{
    (void)hipSetDevice(m_device);
    auto elapsed = [](bool on, hipEvent_t a, hipEvent_t b) {
        float ms = -1.0f;
        if (on && hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) != hipSuccess) ms = -1.0f;
        return ms;
    };
    if (copy_host_ms) *copy_host_ms = m_copyHostMs;
    if (upload_ms) *upload_ms = elapsed(m_upTimed, m_evUp0, m_evUp1);
    if (process_ms) *process_ms = elapsed(m_timed, m_evStart, m_evStop);
    if (readback_ms) *readback_ms = elapsed(m_rbTimed, m_evRb0, m_evRb1);
    return MPCVR_S_OK;
}

HRESULT CHipVideoProcessor::GetLastProcessMs(float *ms)
{
    if (!ms) return Fail(MPCVR_E_POINTER, "null");
    if (!m_timed) return Fail(MPCVR_E_NOT_VALID_STATE, "nothing timed yet");
    (void)hipSetDevice(m_device);
    HRESULT hr;
    if ((hr = CheckHip(hipEventSynchronize(m_evStop), "event sync"))) return hr;
    return CheckHip(hipEventElapsedTime(ms, m_evStart, m_evStop), "event elapsed");
}

}  // namespace mpcvr
