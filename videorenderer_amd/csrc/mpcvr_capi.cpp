// mpcvr_capi.cpp — extern "C" surface of libmpcvr.so (include/mpcvr.h) over CHipVideoProcessor.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/mpcvr.h"
#include "hip_video_processor.h"

using mpcvr::CHipVideoProcessor;
using mpcvr::CRect;

struct mpcvr_ctx {
    CHipVideoProcessor vp;
};

static inline CRect ToRect(const mpcvr_rect *r) { return r ? CRect(r->left, r->top, r->right, r->bottom) : CRect(); }

extern "C" {

int32_t mpcvr_settings_default(mpcvr_settings *s)
{   // Settings_t::SetDefault — IVideoRenderer.h:140-185
    if (!s) return MPCVR_E_POINTER;
    std::memset(s, 0, sizeof(*s));
    s->iTexFormat = MPCVR_TEXFMT_AUTOINT;
    s->iChromaScaling = MPCVR_CHROMA_Bilinear;
    s->iUpscaling = MPCVR_UPSCALE_CatmullRom;
    s->iDownscaling = MPCVR_DOWNSCALE_Hamming;
    s->bInterpolateAt50pct = 1;
    s->bUseDither = 1;
    s->bDeintBlend = 0;
    s->bConvertToSdr = 1;
    s->iSDRDisplayNits = 125;
    s->output_format = MPCVR_OUT_BGRA8;
    s->flags = 0;
    return MPCVR_S_OK;
}

int32_t mpcvr_create(const mpcvr_settings *settings, int32_t device, mpcvr_ctx **out)
{
    if (!out) return MPCVR_E_POINTER;
    *out = nullptr;
    mpcvr_settings def;
    mpcvr_settings_default(&def);
    mpcvr_ctx *ctx = new (std::nothrow) mpcvr_ctx();
    if (!ctx) return MPCVR_E_OUTOFMEMORY;
    const int32_t hr = ctx->vp.Init(device, settings ? *settings : def);
    if (hr < 0) {
        std::fprintf(stderr, "mpcvr_create: %s\n", ctx->vp.LastError());
        delete ctx;
        return hr;
    }
    *out = ctx;
    return MPCVR_S_OK;
}

int32_t mpcvr_destroy(mpcvr_ctx *ctx)
{
    if (!ctx) return MPCVR_E_POINTER;
    delete ctx;
    return MPCVR_S_OK;
}

#define CTX_OR_FAIL() do { if (!ctx) return MPCVR_E_POINTER; } while (0)

int32_t mpcvr_set_stream(mpcvr_ctx *ctx, void *hip_stream) { CTX_OR_FAIL(); return ctx->vp.SetStream((hipStream_t)hip_stream); }
int32_t mpcvr_synchronize(mpcvr_ctx *ctx) { CTX_OR_FAIL(); return ctx->vp.Synchronize(); }

int32_t mpcvr_set_input(mpcvr_ctx *ctx, int32_t cformat, int32_t width, int32_t height, int32_t pitch,
                        const mpcvr_rect *src_rect, uint32_t extfmt)
{
    CTX_OR_FAIL();
    const CRect r = ToRect(src_rect);
    return ctx->vp.InitMediaType(cformat, width, height, pitch, src_rect ? &r : nullptr, extfmt);
}

int32_t mpcvr_set_video_rect(mpcvr_ctx *ctx, const mpcvr_rect *r) { CTX_OR_FAIL(); if (!r) return MPCVR_E_POINTER; return ctx->vp.SetVideoRect(ToRect(r)); }
int32_t mpcvr_set_window_rect(mpcvr_ctx *ctx, const mpcvr_rect *r) { CTX_OR_FAIL(); if (!r) return MPCVR_E_POINTER; return ctx->vp.SetWindowRect(ToRect(r)); }
int32_t mpcvr_set_rotation(mpcvr_ctx *ctx, int32_t degrees) { CTX_OR_FAIL(); return ctx->vp.SetRotation(degrees); }
int32_t mpcvr_set_error_diffusion_patience(mpcvr_ctx *ctx, int32_t polls) { CTX_OR_FAIL(); return ctx->vp.SetErrorDiffusionPatience(polls); }
int32_t mpcvr_set_flip(mpcvr_ctx *ctx, int32_t flip) { CTX_OR_FAIL(); return ctx->vp.SetFlip(flip != 0); }
int32_t mpcvr_set_sample_format(mpcvr_ctx *ctx, int32_t frame_format) { CTX_OR_FAIL(); return ctx->vp.SetSampleFormat(frame_format); }
int32_t mpcvr_set_hdr_output(mpcvr_ctx *ctx, int32_t enable, int32_t tone_map_type, float display_max_nits)
{ CTX_OR_FAIL(); return ctx->vp.SetHdrOutput(enable != 0, tone_map_type, display_max_nits); }
int32_t mpcvr_set_hdr_metadata(mpcvr_ctx *ctx, float min_mastering_nits, float max_mastering_nits, float max_cll, float max_fall)
{ CTX_OR_FAIL(); return ctx->vp.SetHdrMetadata(min_mastering_nits, max_mastering_nits, max_cll, max_fall); }

int32_t mpcvr_set_dovi_metadata(mpcvr_ctx *ctx, const mpcvr_dovi_metadata *md)
{ CTX_OR_FAIL(); return ctx->vp.SetDoviMetadata(md); }

int32_t mpcvr_configure(mpcvr_ctx *ctx, const mpcvr_settings *settings)
{
    CTX_OR_FAIL();
    if (!settings) return MPCVR_E_POINTER;
    return ctx->vp.Configure(*settings);
}

int32_t mpcvr_set_procamp(mpcvr_ctx *ctx, uint32_t flags, float brightness, float contrast, float hue, float saturation)
{
    CTX_OR_FAIL();
    return ctx->vp.SetProcAmpValues(flags, brightness, contrast, hue, saturation);
}

int32_t mpcvr_copy_sample(mpcvr_ctx *ctx, const void *data, int32_t pitch, int32_t mem_kind)
{
    CTX_OR_FAIL();
    return ctx->vp.CopySample(data, pitch, mem_kind);
}

int32_t mpcvr_process(mpcvr_ctx *ctx, void *dst_dev, int32_t dst_pitch, const mpcvr_rect *src_rect,
                      const mpcvr_rect *dst_rect, int32_t second_field)
{
    CTX_OR_FAIL();
    const CRect s = ToRect(src_rect), d = ToRect(dst_rect);
    return ctx->vp.Process(dst_dev, dst_pitch, src_rect ? &s : nullptr, dst_rect ? &d : nullptr, second_field != 0);
}

// the reference's call pattern over n frames — CopySample + Process per frame, one after the other (DX11VideoProcessor.cpp:2143-2200 -> :2730) —
// as ONE entry: what a render thread written in C or C++ does anyway; a scripting-language caller (bench.py, the tests) otherwise times its own
// foreign-function calls (two per frame, ~1.5 us each from ctypes: 6 % of a 50 us frame) instead of the path
int32_t mpcvr_process_frames(mpcvr_ctx *ctx, int32_t n, const void *const *samples, int32_t pitch, int32_t mem_kind, void *const *dsts_dev, int32_t dst_pitch)
{
    CTX_OR_FAIL();
    if (n < 0 || (n > 0 && (!samples || !dsts_dev))) return MPCVR_E_POINTER;
    for (int32_t i = 0; i < n; i++) {
        int32_t hr = ctx->vp.CopySample(samples[i], pitch, mem_kind);
        if (hr < 0) return hr;
        hr = ctx->vp.Process(dsts_dev[i], dst_pitch, nullptr, nullptr, false);
        if (hr < 0) return hr;
    }
    return MPCVR_S_OK;
}

int32_t mpcvr_render(mpcvr_ctx *ctx, int32_t field) { CTX_OR_FAIL(); return ctx->vp.Render(field); }

int32_t mpcvr_render_yuv(mpcvr_ctx *ctx, int32_t field, int32_t out_cformat, uint32_t extfmt, void *y_plane, int32_t y_pitch, void *uv_plane, int32_t uv_pitch)
{
    CTX_OR_FAIL();
    if (!y_plane || !uv_plane) return MPCVR_E_POINTER;
    return ctx->vp.RenderYuv(field, out_cformat, extfmt, y_plane, y_pitch, uv_plane, uv_pitch);
}

int32_t mpcvr_get_backbuffer(mpcvr_ctx *ctx, void **dev_ptr, int32_t *pitch, int32_t *width, int32_t *height)
{
    CTX_OR_FAIL();
    return ctx->vp.GetBackBuffer(dev_ptr, pitch, width, height);
}

int32_t mpcvr_get_current_image(mpcvr_ctx *ctx, void *host_bgra, size_t *size) { CTX_OR_FAIL(); return ctx->vp.GetCurentImage(host_bgra, size); }
int32_t mpcvr_get_displayed_image(mpcvr_ctx *ctx, void *host_pixels, size_t *size, int32_t deep_color, int32_t *width, int32_t *height, int32_t *bits_per_pixel)
{
    CTX_OR_FAIL();
    return ctx->vp.GetDisplayedImage(host_pixels, size, deep_color != 0, width, height, bits_per_pixel);
}
int32_t mpcvr_flush(mpcvr_ctx *ctx) { CTX_OR_FAIL(); ctx->vp.Flush(); return MPCVR_S_OK; }
int32_t mpcvr_reset(mpcvr_ctx *ctx) { CTX_OR_FAIL(); return ctx->vp.Reset(); }

int32_t mpcvr_process_batch(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, void *const *dsts, int32_t dst_pitch)
{
    CTX_OR_FAIL();
    return ctx->vp.ProcessBatch(n, srcs, dsts, dst_pitch);
}

int32_t mpcvr_process_batch_dovi(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, void *const *dsts, int32_t dst_pitch, const mpcvr_dovi_metadata *rpus)
{
    CTX_OR_FAIL();
    return ctx->vp.ProcessBatchDovi(n, srcs, dsts, dst_pitch, rpus);
}

// EXTENSION: a batch as NV12 / P010 (include/mpcvr.h; PlanBatchYuv vp_plan.cpp, CHipVideoProcessor::ProcessBatchYuv)
static_assert(MPCVR_BATCH_YUV_DEFAULT_BUDGET == mpcvr::kBatchYuvDefaultBudget, "the header and vp_plan.h name one default budget");
// what the mpcvr_plan_batch_* functions hand back of a planned layout (each pointer optional)
static int32_t ChunkLayoutOut(bool planned, const mpcvr::ChunkLayout &lay, size_t *frame_stride, int32_t *frames_per_chunk, int32_t *chunks)
{
    if (!planned) return MPCVR_E_INVALIDARG;
    if (frame_stride) *frame_stride = lay.frameStride;
    if (frames_per_chunk) *frames_per_chunk = lay.framesPerChunk;
    if (chunks) *chunks = lay.chunks;
    return MPCVR_S_OK;
}

int32_t mpcvr_plan_batch_yuv(int32_t window_w, int32_t window_h, int32_t n, size_t budget_bytes,
                             int32_t *surface_pitch, size_t *frame_stride, int32_t *frames_per_chunk, int32_t *chunks)
{
    mpcvr::BatchYuvLayout lay;
    const bool planned = mpcvr::PlanBatchYuv(window_w, window_h, n, budget_bytes, &lay);
    if (planned && surface_pitch) *surface_pitch = lay.surfacePitch;
    return ChunkLayoutOut(planned, lay, frame_stride, frames_per_chunk, chunks);
}

int32_t mpcvr_set_batch_yuv_budget(mpcvr_ctx *ctx, size_t bytes) { CTX_OR_FAIL(); return ctx->vp.SetBatchYuvBudget(bytes); }

int32_t mpcvr_process_batch_yuv(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, int32_t out_cformat, uint32_t extfmt,
                                void *const *y_planes, int32_t y_pitch, void *const *uv_planes, int32_t uv_pitch)
{
    CTX_OR_FAIL();
    return ctx->vp.ProcessBatchYuv(n, srcs, out_cformat, extfmt, y_planes, y_pitch, uv_planes, uv_pitch);
}

// EXTENSION: the histogram of max(R, G, B) of rendered frames and what a host derives from it (include/mpcvr.h; k_measure_maxrgb
// vp_measure.hip, MeasureSurface hip_video_processor_ext.cpp, the host functions vp_plan.cpp)
static_assert(MPCVR_HIST_BINS == mpcvr::kHistBins, "the header and vp_measure.h name one histogram size");
int32_t mpcvr_process_batch_yuv_stats(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, int32_t out_cformat, uint32_t extfmt,
                                      void *const *y_planes, int32_t y_pitch, void *const *uv_planes, int32_t uv_pitch, uint32_t *hist_dev)
{
    CTX_OR_FAIL();
    if (!hist_dev) return MPCVR_E_POINTER;
    return ctx->vp.ProcessBatchYuv(n, srcs, out_cformat, extfmt, y_planes, y_pitch, uv_planes, uv_pitch, hist_dev);
}

int32_t mpcvr_measure_pass(const void *src, int32_t src_pitch, int32_t src_fmt, int32_t w, int32_t h, const mpcvr_rect *rect, uint32_t *hist_dev,
                           void *stream)
{
    return mpcvr::MeasureSurface(src, src_pitch, src_fmt, w, h, rect, hist_dev, (hipStream_t)stream, false);
}

int32_t mpcvr_measure_backbuffer(mpcvr_ctx *ctx, uint32_t *hist_dev) { CTX_OR_FAIL(); return ctx->vp.MeasureBackBuffer(hist_dev); }

int32_t mpcvr_light_level_from_histogram(const uint32_t hist[MPCVR_HIST_BINS], int32_t src_fmt, mpcvr_light_level *out)
{
    if (!hist || !out) return MPCVR_E_POINTER;
    if (src_fmt != MPCVR_OUT_BGRA8 && src_fmt != MPCVR_OUT_RGB10A2) return MPCVR_E_INVALIDARG;
    mpcvr::LightLevelFromHistogram(hist, src_fmt == MPCVR_OUT_RGB10A2 ? 1023 : 255, out);
    return MPCVR_S_OK;
}

int32_t mpcvr_histogram_percentile(const uint32_t hist[MPCVR_HIST_BINS], uint32_t ppm, int32_t *code)
{
    if (!hist || !code) return MPCVR_E_POINTER;
    if (ppm < 1 || ppm > 1000000) return MPCVR_E_INVALIDARG;
    const int c = mpcvr::HistogramPercentile(hist, ppm);
    if (c < 0) return MPCVR_E_INVALIDARG;
    *code = c;
    return MPCVR_S_OK;
}

// EXTENSION: rendered frames as float tensors (include/mpcvr.h; k_tensor vp_tensor.hip, the arithmetic vp_tensor_core.h, TensorSurface and
// CHipVideoProcessor::RenderTensor / ProcessBatchTensor hip_video_processor_ext.cpp, PlanTensorValue / PlanBatchTensor vp_plan.cpp)
static_assert(MPCVR_TENSOR_F32 == mpcvr::TN_F32 && MPCVR_TENSOR_F16 == mpcvr::TN_F16 && MPCVR_TENSOR_BF16 == mpcvr::TN_BF16 &&
              MPCVR_TENSOR_PLANAR == mpcvr::TN_PLANAR && MPCVR_TENSOR_INTERLEAVED == mpcvr::TN_INTERLEAVED, "the header and vp_tensor_core.h name one set of tensor formats");
int32_t mpcvr_plan_tensor_value(int32_t dtype, int32_t src_fmt, uint32_t code, float scale, float bias, uint32_t *bits)
{
    if (!bits) return MPCVR_E_POINTER;
    return mpcvr::PlanTensorValue(dtype, src_fmt, code, scale, bias, bits) ? MPCVR_S_OK : MPCVR_E_INVALIDARG;
}

int32_t mpcvr_tensor_pass(const void *src, int32_t src_pitch, int32_t src_fmt, int32_t w, int32_t h, const mpcvr_tensor_desc *desc, void *dst, void *stream)
{
    return mpcvr::TensorSurface(src, src_pitch, src_fmt, w, h, desc, dst, (hipStream_t)stream, false);
}

int32_t mpcvr_render_tensor(mpcvr_ctx *ctx, int32_t field, const mpcvr_tensor_desc *desc, void *dst)
{
    CTX_OR_FAIL();
    if (!desc || !dst) return MPCVR_E_POINTER;
    return ctx->vp.RenderTensor(field, *desc, dst);
}

int32_t mpcvr_plan_batch_tensor(int32_t window_w, int32_t window_h, int32_t n, size_t budget_bytes,
                                int32_t *surface_pitch, size_t *frame_stride, int32_t *frames_per_chunk, int32_t *chunks)
{
    mpcvr::BatchYuvLayout lay;
    const bool planned = mpcvr::PlanBatchTensor(window_w, window_h, n, budget_bytes, &lay);
    if (planned && surface_pitch) *surface_pitch = lay.surfacePitch;
    return ChunkLayoutOut(planned, lay, frame_stride, frames_per_chunk, chunks);
}

int32_t mpcvr_process_batch_tensor(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, const mpcvr_tensor_desc *desc, void *const *dsts)
{
    CTX_OR_FAIL();
    return ctx->vp.ProcessBatchTensor(n, srcs, desc, dsts);
}

// EXTENSION: a model's float tensor as the sample (include/mpcvr.h; k_sample_from_tensor vp_tensor_in.hip, the arithmetic vp_tensor_core.h,
// SampleSurface and CHipVideoProcessor::CopySampleTensor / ProcessBatchFromTensors hip_video_processor_ext.cpp, PlanSampleCode / PlanBatchSamples vp_plan.cpp)
int32_t mpcvr_plan_sample_code(int32_t dtype, int32_t cformat, uint32_t element_bits, float scale, float bias, uint32_t *code)
{
    if (!code) return MPCVR_E_POINTER;
    return mpcvr::PlanSampleCode(dtype, cformat, element_bits, scale, bias, code) ? MPCVR_S_OK : MPCVR_E_INVALIDARG;
}

int32_t mpcvr_sample_pass(const void *tensor, const mpcvr_tensor_desc *desc, int32_t w, int32_t h, int32_t cformat, void *sample, int32_t pitch, void *stream)
{
    return mpcvr::SampleSurface(tensor, desc, w, h, cformat, sample, pitch, (hipStream_t)stream, false);
}

int32_t mpcvr_copy_sample_tensor(mpcvr_ctx *ctx, const void *tensor, const mpcvr_tensor_desc *desc)
{
    CTX_OR_FAIL();
    return ctx->vp.CopySampleTensor(tensor, desc);
}

int32_t mpcvr_plan_batch_from_tensors(int32_t pitch, int32_t h, int32_t n, size_t budget_bytes, size_t *frame_stride, int32_t *frames_per_chunk, int32_t *chunks)
{
    mpcvr::ChunkLayout lay;
    return ChunkLayoutOut(mpcvr::PlanBatchSamples(pitch, h, n, budget_bytes, &lay), lay, frame_stride, frames_per_chunk, chunks);
}

int32_t mpcvr_process_batch_from_tensors(mpcvr_ctx *ctx, int32_t n, const void *const *tensors, const mpcvr_tensor_desc *desc, void *const *dsts, int32_t dst_pitch)
{
    CTX_OR_FAIL();
    return ctx->vp.ProcessBatchFromTensors(n, tensors, desc, dsts, dst_pitch);
}

// EXTENSION: motion-adaptive deinterlacing at field rate (include/mpcvr.h; k_deint vp_deint.hip, the arithmetic vp_deint_core.h, DeintSurface and
// CHipVideoProcessor::CopySampleFields / ProcessBatchDeint hip_video_processor_ext.cpp, PlanDeintPlanes / PlanBatchDeint vp_plan.cpp)
static_assert(MPCVR_DEINT_ADAPTIVE_EXT == mpcvr::DI_ADAPTIVE && MPCVR_DEINT_ADAPTIVE_NOCHECK_EXT == mpcvr::DI_ADAPTIVE_NOCHECK, "the header and vp_deint_core.h name one set of modes");
int32_t mpcvr_plan_deint_planes(int32_t cformat, int32_t w, int32_t h, int32_t pitch, int32_t *planes, mpcvr_deint_plane out[3])
{
    if (!planes || !out) return MPCVR_E_POINTER;
    mpcvr::DeintPlane pl[mpcvr::kDeintMaxPlanes];
    int n = 0;
    if (!mpcvr::PlanDeintPlanes(cformat, w, h, pitch, &n, pl)) return MPCVR_E_INVALIDARG;
    for (int i = 0; i < n; i++) out[i] = mpcvr_deint_plane{pl[i].offset, pl[i].pitch, pl[i].comps, pl[i].lines, pl[i].bytes, pl[i].cs, pl[i].mask};
    *planes = n;
    return MPCVR_S_OK;
}

int32_t mpcvr_deint_plane_host(const void *prev, const void *cur, const void *next, int64_t src_pitch, int32_t comps, int32_t lines, int32_t bytes, int32_t cs,
                               int32_t mask, int32_t keep, int32_t first, int32_t mode, void *dst, int64_t dst_pitch)
{
    if (!prev || !cur || !next || !dst) return MPCVR_E_POINTER;
    if ((bytes != 1 && bytes != 2) || (cs != 1 && cs != 2) || comps < cs || comps % cs || lines < 2 || (keep != 0 && keep != 1) || (first != 0 && first != 1) ||
        (mode != mpcvr::DI_ADAPTIVE && mode != mpcvr::DI_ADAPTIVE_NOCHECK) || mask < 0 || mask > (bytes == 1 ? 0xff : 0xffff) ||
        src_pitch < (int64_t)comps * bytes || dst_pitch < (int64_t)comps * bytes || ((src_pitch | dst_pitch) & (bytes - 1)) ||
        (((uintptr_t)prev | (uintptr_t)cur | (uintptr_t)next | (uintptr_t)dst) & (uintptr_t)(bytes - 1)))
        return MPCVR_E_INVALIDARG;
    mpcvr::DeintPlaneHost((const uint8_t *)prev, (const uint8_t *)cur, (const uint8_t *)next, src_pitch, comps, lines, bytes, cs, mask, keep, first, mode,
                          (uint8_t *)dst, dst_pitch);
    return MPCVR_S_OK;
}

int32_t mpcvr_deint_pass(const void *prev, const void *cur, const void *next, int32_t cformat, int32_t w, int32_t h, int32_t pitch,
                         int32_t keep, int32_t first, int32_t mode, void *dst, int32_t dst_pitch, void *stream)
{
    return mpcvr::DeintSurface(prev, cur, next, cformat, w, h, pitch, keep, first, mode, dst, dst_pitch, (hipStream_t)stream, false);
}

int32_t mpcvr_copy_sample_fields(mpcvr_ctx *ctx, const void *prev, const void *cur, const void *next, int32_t field_order, int32_t field, int32_t mode)
{
    CTX_OR_FAIL();
    return ctx->vp.CopySampleFields(prev, cur, next, field_order, field, mode);
}

int32_t mpcvr_plan_batch_deint(int32_t pitch, int32_t lines, int32_t n_out, size_t budget_bytes, size_t *frame_stride, int32_t *frames_per_chunk, int32_t *chunks)
{
    mpcvr::ChunkLayout lay;
    return ChunkLayoutOut(mpcvr::PlanBatchDeint(pitch, lines, n_out, budget_bytes, &lay), lay, frame_stride, frames_per_chunk, chunks);
}

int32_t mpcvr_process_batch_deint(mpcvr_ctx *ctx, int32_t n, const void *const *frames, int32_t field_order, int32_t fields_per_frame, int32_t mode,
                                  void *const *dsts, int32_t dst_pitch)
{
    CTX_OR_FAIL();
    return ctx->vp.ProcessBatchDeint(n, frames, field_order, fields_per_frame, mode, dsts, dst_pitch);
}

// EXTENSION: a 3D colour LUT over rendered frames (include/mpcvr.h; k_lut3d vp_lut3d.hip, the arithmetic vp_lut3d_core.h, Lut3dSurface and
// CHipVideoProcessor::RenderLut3d / ProcessBatchLut3d hip_video_processor_ext.cpp, PlanLut3dEntries / PlanLut3dValue vp_plan.cpp)
int32_t mpcvr_plan_lut3d_entries(const float *rgb, int32_t n, uint16_t *entries)
{
    if (!rgb || !entries) return MPCVR_E_POINTER;
    if (n < mpcvr::kLut3dMinN || n > mpcvr::kLut3dMaxN) return MPCVR_E_INVALIDARG;
    mpcvr::PlanLut3dEntries(rgb, n, entries);
    return MPCVR_S_OK;
}

int32_t mpcvr_plan_lut3d_value(int32_t src_fmt, int32_t dst_fmt, const uint16_t *entries_host, int32_t n, uint32_t texel, uint32_t *out)
{
    if (!entries_host || !out) return MPCVR_E_POINTER;
    return mpcvr::PlanLut3dValue(src_fmt, dst_fmt, entries_host, n, texel, out) ? MPCVR_S_OK : MPCVR_E_INVALIDARG;
}

int32_t mpcvr_lut3d_pass(const void *src, int32_t src_pitch, int32_t src_fmt, int32_t w, int32_t h, const void *lut_dev, int32_t n, void *dst,
                         int32_t dst_pitch, int32_t dst_fmt, void *stream)
{
    return mpcvr::Lut3dSurface(src, src_pitch, src_fmt, w, h, lut_dev, n, dst, dst_pitch, dst_fmt, (hipStream_t)stream, false);
}

int32_t mpcvr_render_lut3d(mpcvr_ctx *ctx, int32_t field, const void *lut_dev, int32_t n, void *dst, int32_t dst_pitch, int32_t dst_fmt)
{
    CTX_OR_FAIL();
    if (!lut_dev || !dst) return MPCVR_E_POINTER;
    return ctx->vp.RenderLut3d(field, lut_dev, n, dst, dst_pitch, dst_fmt);
}

int32_t mpcvr_plan_batch_lut3d(int32_t window_w, int32_t window_h, int32_t n, size_t budget_bytes,
                               int32_t *surface_pitch, size_t *frame_stride, int32_t *frames_per_chunk, int32_t *chunks)
{
    mpcvr::BatchYuvLayout lay;
    const bool planned = mpcvr::PlanBatchTensor(window_w, window_h, n, budget_bytes, &lay);      // (the same surface of 32-bit texels)
    if (planned && surface_pitch) *surface_pitch = lay.surfacePitch;
    return ChunkLayoutOut(planned, lay, frame_stride, frames_per_chunk, chunks);
}

int32_t mpcvr_process_batch_lut3d(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, const void *lut_dev, int32_t lut_n, void *const *dsts,
                                  int32_t dst_pitch, int32_t dst_fmt)
{
    CTX_OR_FAIL();
    return ctx->vp.ProcessBatchLut3d(n, srcs, lut_dev, lut_n, dsts, dst_pitch, dst_fmt);
}

// EXTENSION: debanding of rendered frames (include/mpcvr.h; k_deband vp_deband.hip, the arithmetic vp_deband_core.h, DebandSurface and
// CHipVideoProcessor::RenderDeband / ProcessBatchDeband hip_video_processor_ext.cpp, PlanDebandDefaults / PlanDebandHost vp_plan.cpp)
int32_t mpcvr_deband_params_default(int32_t src_fmt, mpcvr_deband_params *params)
{
    if (!params) return MPCVR_E_POINTER;
    mpcvr::DebandArgs a;
    if (!mpcvr::PlanDebandDefaults(src_fmt, &a)) return MPCVR_E_INVALIDARG;
    *params = mpcvr_deband_params{a.range, a.iterations, a.threshold, a.dither};
    return MPCVR_S_OK;
}

int32_t mpcvr_deband_host(const void *src_host, int64_t src_pitch, int32_t src_fmt, int32_t w, int32_t h, const mpcvr_deband_params *params,
                          uint32_t seed, void *dst_host, int64_t dst_pitch, int32_t dst_fmt)
{
    if (!src_host || !params || !dst_host) return MPCVR_E_POINTER;
    const mpcvr::DebandArgs a{params->range, params->iterations, params->threshold, params->dither};
    return mpcvr::PlanDebandHost(src_host, src_pitch, src_fmt, w, h, a, seed, dst_host, dst_pitch, dst_fmt) ? MPCVR_S_OK : MPCVR_E_INVALIDARG;
}

int32_t mpcvr_plan_deband(int32_t src_fmt, const mpcvr_deband_params *params, int32_t w, int32_t h, int32_t *halo, int32_t *placement)
{
    if (!params) return MPCVR_E_POINTER;
    if ((src_fmt != MPCVR_OUT_BGRA8 && src_fmt != MPCVR_OUT_RGB10A2) || w < 1 || h < 1 || w > 32768 || h > 32768 ||
        !mpcvr::DebandArgsValid(mpcvr::DebandArgs{params->range, params->iterations, params->threshold, params->dither}, src_fmt == MPCVR_OUT_RGB10A2))
        return MPCVR_E_INVALIDARG;
    const int R = params->range * params->iterations;
    if (halo) *halo = R;
    if (placement) *placement = mpcvr::DebandPlaceFor(R, w, h);
    return MPCVR_S_OK;
}

int32_t mpcvr_deband_pass(const void *src, int32_t src_pitch, int32_t src_fmt, int32_t w, int32_t h, const mpcvr_deband_params *params,
                          uint32_t seed, void *dst, int32_t dst_pitch, int32_t dst_fmt, void *stream)
{
    return mpcvr::DebandSurface(src, src_pitch, src_fmt, w, h, params, seed, dst, dst_pitch, dst_fmt, (hipStream_t)stream, false);
}

int32_t mpcvr_render_deband(mpcvr_ctx *ctx, int32_t field, const mpcvr_deband_params *params, uint32_t seed, void *dst, int32_t dst_pitch, int32_t dst_fmt)
{
    CTX_OR_FAIL();
    if (!params || !dst) return MPCVR_E_POINTER;
    return ctx->vp.RenderDeband(field, params, seed, dst, dst_pitch, dst_fmt);
}

int32_t mpcvr_plan_batch_deband(int32_t window_w, int32_t window_h, int32_t n, size_t budget_bytes,
                                int32_t *surface_pitch, size_t *frame_stride, int32_t *frames_per_chunk, int32_t *chunks)
{
    mpcvr::BatchYuvLayout lay;
    const bool planned = mpcvr::PlanBatchTensor(window_w, window_h, n, budget_bytes, &lay);      // (the same surface of 32-bit texels)
    if (planned && surface_pitch) *surface_pitch = lay.surfacePitch;
    return ChunkLayoutOut(planned, lay, frame_stride, frames_per_chunk, chunks);
}

int32_t mpcvr_process_batch_deband(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, const mpcvr_deband_params *params, uint32_t seed,
                                   void *const *dsts, int32_t dst_pitch, int32_t dst_fmt)
{
    CTX_OR_FAIL();
    return ctx->vp.ProcessBatchDeband(n, srcs, params, seed, dsts, dst_pitch, dst_fmt);
}

// EXTENSION: sharpening of rendered frames (include/mpcvr.h; k_sharpen vp_sharpen.hip, the arithmetic vp_sharpen_core.h, SharpenSurface and
// CHipVideoProcessor::RenderSharpen / ProcessBatchSharpen hip_video_processor_ext.cpp, PlanSharpenDefaults / PlanSharpenHost vp_plan.cpp)
static mpcvr::SharpenArgs SharpenArgsOf(const mpcvr_sharpen_params &p)
{
    return mpcvr::SharpenArgs{p.radius, p.amount, p.threshold, p.overshoot, p.mode, p.dither};
}

int32_t mpcvr_sharpen_params_default(int32_t src_fmt, mpcvr_sharpen_params *params)
{
    if (!params) return MPCVR_E_POINTER;
    mpcvr::SharpenArgs a;
    if (!mpcvr::PlanSharpenDefaults(src_fmt, &a)) return MPCVR_E_INVALIDARG;
    *params = mpcvr_sharpen_params{a.radius, a.amount, a.threshold, a.overshoot, a.mode, a.dither};
    return MPCVR_S_OK;
}

int32_t mpcvr_sharpen_host(const void *src_host, int64_t src_pitch, int32_t src_fmt, int32_t w, int32_t h, const mpcvr_sharpen_params *params,
                           uint32_t seed, void *dst_host, int64_t dst_pitch, int32_t dst_fmt)
{
    if (!src_host || !params || !dst_host) return MPCVR_E_POINTER;
    return mpcvr::PlanSharpenHost(src_host, src_pitch, src_fmt, w, h, SharpenArgsOf(*params), seed, dst_host, dst_pitch, dst_fmt) ? MPCVR_S_OK : MPCVR_E_INVALIDARG;
}

int32_t mpcvr_plan_sharpen(int32_t src_fmt, const mpcvr_sharpen_params *params, int32_t w, int32_t h, int32_t *halo, int32_t *lds_bytes)
{
    if (!params) return MPCVR_E_POINTER;
    if ((src_fmt != MPCVR_OUT_BGRA8 && src_fmt != MPCVR_OUT_RGB10A2) || w < 1 || h < 1 || w > 32768 || h > 32768 ||
        !mpcvr::SharpenArgsValid(SharpenArgsOf(*params), src_fmt == MPCVR_OUT_RGB10A2))
        return MPCVR_E_INVALIDARG;
    if (halo) *halo = params->radius;
    if (lds_bytes) *lds_bytes = mpcvr::SharpenLdsBytes(params->radius, params->mode);
    return MPCVR_S_OK;
}

int32_t mpcvr_sharpen_pass(const void *src, int32_t src_pitch, int32_t src_fmt, int32_t w, int32_t h, const mpcvr_sharpen_params *params,
                           uint32_t seed, void *dst, int32_t dst_pitch, int32_t dst_fmt, void *stream)
{
    return mpcvr::SharpenSurface(src, src_pitch, src_fmt, w, h, params, seed, dst, dst_pitch, dst_fmt, (hipStream_t)stream, false);
}

int32_t mpcvr_render_sharpen(mpcvr_ctx *ctx, int32_t field, const mpcvr_sharpen_params *params, uint32_t seed, void *dst, int32_t dst_pitch, int32_t dst_fmt)
{
    CTX_OR_FAIL();
    if (!params || !dst) return MPCVR_E_POINTER;
    return ctx->vp.RenderSharpen(field, params, seed, dst, dst_pitch, dst_fmt);
}

int32_t mpcvr_plan_batch_sharpen(int32_t window_w, int32_t window_h, int32_t n, size_t budget_bytes,
                                 int32_t *surface_pitch, size_t *frame_stride, int32_t *frames_per_chunk, int32_t *chunks)
{
    mpcvr::BatchYuvLayout lay;
    const bool planned = mpcvr::PlanBatchTensor(window_w, window_h, n, budget_bytes, &lay);      // (the same surface of 32-bit texels)
    if (planned && surface_pitch) *surface_pitch = lay.surfacePitch;
    return ChunkLayoutOut(planned, lay, frame_stride, frames_per_chunk, chunks);
}

int32_t mpcvr_process_batch_sharpen(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, const mpcvr_sharpen_params *params, uint32_t seed,
                                    void *const *dsts, int32_t dst_pitch, int32_t dst_fmt)
{
    CTX_OR_FAIL();
    return ctx->vp.ProcessBatchSharpen(n, srcs, params, seed, dsts, dst_pitch, dst_fmt);
}

int32_t mpcvr_get_param_blob(mpcvr_ctx *ctx, void *buf, size_t *size) { CTX_OR_FAIL(); return ctx->vp.GetParamBlob(buf, size); }
int32_t mpcvr_get_fused_tables(mpcvr_ctx *ctx, void *buf, size_t *size) { CTX_OR_FAIL(); return ctx->vp.GetFusedTables(buf, size); }
int32_t mpcvr_set_param_blob(mpcvr_ctx *ctx, const void *buf, size_t size) { CTX_OR_FAIL(); return ctx->vp.SetParamBlob(buf, size); }
int32_t mpcvr_broadcast_param_blob_begin(mpcvr_ctx *ctx, void *nccl_comm, int32_t root, int32_t rank) { CTX_OR_FAIL(); return ctx->vp.BroadcastParamBlobBegin(nccl_comm, root, rank); }
int32_t mpcvr_broadcast_param_blob_end(mpcvr_ctx *ctx) { CTX_OR_FAIL(); return ctx->vp.BroadcastParamBlobEnd(); }
int32_t mpcvr_broadcast_param_blob(mpcvr_ctx *ctx, void *nccl_comm, int32_t root, int32_t rank)
{
    CTX_OR_FAIL();
    const int32_t hr = ctx->vp.BroadcastParamBlobBegin(nccl_comm, root, rank);
    return hr < 0 ? hr : ctx->vp.BroadcastParamBlobEnd();
}

int32_t mpcvr_get_color_matrix(mpcvr_ctx *ctx, float out12[12]) { CTX_OR_FAIL(); if (!out12) return MPCVR_E_POINTER; return ctx->vp.GetColorMatrix(out12); }
int32_t mpcvr_get_extfmt(mpcvr_ctx *ctx, uint32_t *extfmt) { CTX_OR_FAIL(); if (!extfmt) return MPCVR_E_POINTER; return ctx->vp.GetExtFmt(extfmt); }
int32_t mpcvr_get_frame_bytes(mpcvr_ctx *ctx, size_t *bytes, int32_t *pitch) { CTX_OR_FAIL(); return ctx->vp.GetFrameBytes(bytes, pitch); }

int32_t mpcvr_get_path_info(mpcvr_ctx *ctx, char *buf, size_t buf_size)
{
    CTX_OR_FAIL();
    if (!buf || !buf_size) return MPCVR_E_POINTER;
    const std::string s = ctx->vp.GetPathInfo();
    std::snprintf(buf, buf_size, "%s", s.c_str());
    return MPCVR_S_OK;
}

int32_t mpcvr_get_last_batch_info(mpcvr_ctx *ctx, char *buf, size_t buf_size)
{
    CTX_OR_FAIL();
    if (!buf || !buf_size) return MPCVR_E_POINTER;
    std::snprintf(buf, buf_size, "%s", ctx->vp.GetLastBatchInfo().c_str());
    return MPCVR_S_OK;
}

const char *mpcvr_last_error(mpcvr_ctx *ctx) { return ctx ? ctx->vp.LastError() : "null context"; }
const char *mpcvr_version(void) { return "mpcvr-mi355x 0.1 (gfx950)"; }

int32_t mpcvr_get_last_process_ms(mpcvr_ctx *ctx, float *ms) { CTX_OR_FAIL(); return ctx->vp.GetLastProcessMs(ms); }
int32_t mpcvr_get_last_timings(mpcvr_ctx *ctx, float *copy_host_ms, float *upload_ms, float *process_ms, float *readback_ms)
{
    CTX_OR_FAIL();
    return ctx->vp.GetLastTimings(copy_host_ms, upload_ms, process_ms, readback_ms);
}

}  // extern "C"

// ---- host-side parameter maths without a context (no GPU needed) --------------------------------
// What the reference computes on the CPU before it ever touches the device: format table, extended
// format defaults, colour / gamut matrices, resize weights, tap tables and the pass plan.
#include "vp_plan.h"
#include "vp_plan_tables.h"

extern "C" {

int32_t mpcvr_plan_frame_layout(int32_t cformat, int32_t width, int32_t height, int32_t *pitch, size_t *bytes)
{
    const mpcvr::FmtConvParams *f = mpcvr::GetFmtConvParams(cformat);
    if (!f) return MPCVR_E_NOTIMPL;
    const int p = mpcvr::DefaultPitch(*f, width);
    if (pitch) *pitch = p;
    if (bytes) *bytes = (size_t)p * mpcvr::SourceLines(*f, height);
    return MPCVR_S_OK;
}

int32_t mpcvr_plan_color_matrix(int32_t cformat, int32_t rect_w, int32_t rect_h, uint32_t extfmt,
                                float brightness, float contrast, float hue, float saturation,
                                float out12[12], uint32_t *extfmt_out)
{
    const mpcvr::FmtConvParams *f = mpcvr::GetFmtConvParams(cformat);
    if (!f) return MPCVR_E_NOTIMPL;
    if (!out12) return MPCVR_E_POINTER;
    const mpcvr::ExtFmt ex = mpcvr::SpecifyExtendedFormat(mpcvr::ExtFmt{extfmt}, *f, rect_w, rect_h);
    mpcvr::ProcAmp pa;
    pa.brightness = brightness; pa.contrast = contrast; pa.hue = hue; pa.saturation = saturation;
    mpcvr::ComputeColorMatrix(ex, *f, pa, out12);
    if (extfmt_out) *extfmt_out = ex.value;
    return MPCVR_S_OK;
}

int32_t mpcvr_plan_gamut_2020_to_709(float out9[9])
{
    if (!out9) return MPCVR_E_POINTER;
    mpcvr::ComputeGamut2020to709(out9);
    return MPCVR_S_OK;
}

int32_t mpcvr_plan_pq_lut(float lum_scale, float out4096[4096])
{
    static_assert(mpcvr::kPqLutSize == 4096, "header documents 4096 entries");
    if (!out4096) return MPCVR_E_POINTER;
    mpcvr::BuildPqSdrLut(lum_scale, out4096);
    return MPCVR_S_OK;
}

int32_t mpcvr_plan_final_pass_multiplier(int32_t quant, int32_t maxv, uint32_t *multiplier)
{
    if (!multiplier) return MPCVR_E_POINTER;
    *multiplier = mpcvr::FinalPassMultiplier(quant, maxv);
    return MPCVR_S_OK;
}

int32_t mpcvr_plan_correction_matrices(float fix_bt2020_16[16], float fix_ycgco_16[16], float gamut9[9])
{
    if (!fix_bt2020_16 || !fix_ycgco_16 || !gamut9) return MPCVR_E_POINTER;
    mpcvr::CorrectionMatrices(fix_bt2020_16, fix_ycgco_16, gamut9);
    return MPCVR_S_OK;
}

int32_t mpcvr_correction_pass(int32_t kind, const void *src, int32_t src_pitch, int32_t src_fmt,
                              void *dst, int32_t dst_pitch, int32_t dst_fmt, int32_t w, int32_t h, int32_t sdr_nits, void *stream)
{
    if (!src || !dst) return MPCVR_E_POINTER;
    if (kind < MPCVR_CORR_FIX_BT2020 || kind > MPCVR_CORR_CONVERT_HLG_TO_PQ || w <= 0 || h <= 0 || sdr_nits <= 0 ||
        src_pitch < w * 4 || dst_pitch < w * 4 || (src_pitch & 3) || (dst_pitch & 3) ||
        (src_fmt != MPCVR_OUT_BGRA8 && src_fmt != MPCVR_OUT_RGB10A2) || (dst_fmt != MPCVR_OUT_BGRA8 && dst_fmt != MPCVR_OUT_RGB10A2))
        return MPCVR_E_INVALIDARG;
    float fix2020[16], fixycgco[16], gamut[9];
    mpcvr::CorrectionMatrices(fix2020, fixycgco, gamut);
    const mpcvr::Surface in{const_cast<void *>(src), src_pitch, w, h, src_fmt == MPCVR_OUT_RGB10A2 ? mpcvr::SF_RGB10A2 : mpcvr::SF_BGRA8};
    const mpcvr::Surface out{dst, dst_pitch, w, h, dst_fmt == MPCVR_OUT_RGB10A2 ? mpcvr::SF_RGB10A2 : mpcvr::SF_BGRA8};
    const hipError_t e = mpcvr::LaunchCorrection(kind, in, out, kind == MPCVR_CORR_FIX_YCGCO ? fixycgco : fix2020, gamut,
                                                 10000.0f / (float)sdr_nits, (hipStream_t)stream);
    return e == hipSuccess ? MPCVR_S_OK : MPCVR_E_FAIL;
}

// EXTENSION: RGB -> NV12 / P010 for an encoder (include/mpcvr.h; PlanEncode vp_plan.cpp, k_encode420 vp_encode.hip)
int32_t mpcvr_plan_encode(int32_t out_cformat, int32_t src_fmt, uint32_t extfmt, int32_t coef9[9], int32_t off3[3], int32_t *shift,
                          int32_t *siting, uint32_t *extfmt_out)
{
    mpcvr::EncodePlan plan;
    if (!mpcvr::PlanEncode(out_cformat, src_fmt, extfmt, 0, 0, &plan)) return MPCVR_E_INVALIDARG;      // (no size: the matrix default of a small frame)
    if (coef9) std::memcpy(coef9, plan.coef, sizeof(plan.coef));
    if (off3) std::memcpy(off3, plan.off, sizeof(plan.off));
    if (shift) *shift = plan.shift;
    if (siting) *siting = plan.siting;
    if (extfmt_out) *extfmt_out = plan.extfmt;
    return MPCVR_S_OK;
}

int32_t mpcvr_encode_pass(const void *src, int32_t src_pitch, int32_t src_fmt, int32_t w, int32_t h, int32_t out_cformat, uint32_t extfmt,
                          void *y_plane, int32_t y_pitch, void *uv_plane, int32_t uv_pitch, void *stream)
{
    return mpcvr::EncodeSurface(src, src_pitch, src_fmt, w, h, out_cformat, extfmt, y_plane, y_pitch, uv_plane, uv_pitch, (hipStream_t)stream, false);
}

int32_t mpcvr_plan_dovi(const mpcvr_dovi_metadata *md, int32_t display_nits, float *cb705, int32_t *has_mmr,
                        float lms9[9], float l2k[5], int32_t *l2_enabled, uint32_t l1_nits[3], int32_t *l1_present)
{
    if (!md) return MPCVR_E_POINTER;
    if (!mpcvr::CheckDoviCurves(*md)) return MPCVR_E_INVALIDARG;
    if (cb705 || has_mmr) {
        mpcvr::DoviParams P{};
        mpcvr::PackDoviCurves(*md, &P);
        if (has_mmr) *has_mmr = P.has_mmr;
        if (cb705)
            for (int c = 0; c < 3; c++) {
                float *o = cb705 + c * 235;
                const mpcvr::DoviCurve &cv = P.curves[c];
                std::memcpy(o, cv.pivots, sizeof(float) * 7);
                std::memcpy(o + 7, cv.coeffs, sizeof(float) * 32);
                std::memcpy(o + 39, cv.mmr, sizeof(float) * 192);
                o[231] = (float)cv.methods; o[232] = (float)cv.mmr_single; o[233] = (float)cv.min_order; o[234] = (float)cv.max_order;
            }
    }
    if (lms9) mpcvr::DoviLmsMatrix(*md, lms9);
    if (l2k || l2_enabled) {
        float k[5];
        const bool on = mpcvr::DoviL2Constants(*md, display_nits, k);
        if (l2k) std::memcpy(l2k, k, sizeof(k));
        if (l2_enabled) *l2_enabled = on ? 1 : 0;
    }
    if (l1_nits || l1_present) {
        uint32_t v[3];
        const bool on = mpcvr::DoviL1Nits(*md, v);
        if (l1_nits) std::memcpy(l1_nits, v, sizeof(v));
        if (l1_present) *l1_present = on ? 1 : 0;
    }
    return MPCVR_S_OK;
}

int32_t mpcvr_plan_upscale_weights(int32_t iUpscaling, float t, float w6[6])
{
    if (!w6) return MPCVR_E_POINTER;
    return mpcvr::UpscaleWeights(iUpscaling, t, w6);      // tap count (4/6) or 0
}

int32_t mpcvr_plan_axis_taps(int32_t kind, int32_t method, int32_t src_l, int32_t src_len, int32_t n_out,
                             int32_t tex_len, uint32_t flags, int32_t cap_taps, int32_t *idx, float *w,
                             float *wsum, int32_t *ntaps, int32_t *normalise)
{
    if (!ntaps) return MPCVR_E_POINTER;
    if (n_out <= 0 || src_len <= 0 || tex_len <= 0) return MPCVR_E_INVALIDARG;
    mpcvr::HostAxisTaps h;
    if (!mpcvr::BuildAxisTaps(mpcvr::Resizer{kind, method}, src_l, src_len, n_out, tex_len, flags, &h)) return MPCVR_E_NOTIMPL;
    *ntaps = h.ntaps;
    if (normalise) *normalise = h.normalise;
    if (h.ntaps > cap_taps) return MPCVR_S_FALSE;          // caller's buffers too small: only *ntaps is valid
    if (idx) std::memcpy(idx, h.idx.data(), h.idx.size() * sizeof(int32_t));
    if (w) std::memcpy(w, h.w.data(), h.w.size() * sizeof(float));
    if (wsum && h.normalise) std::memcpy(wsum, h.wsum.data(), h.wsum.size() * sizeof(float));
    return MPCVR_S_OK;
}

// the tables of an unrotated two-pass resize of a converted src_w x src_h frame, from the planner the processor runs (BuildPlanTables): X from
// the convert output (rect at the origin), Y from m_TexResize (src_h rows).  The routing flags do not reach it: these entry points describe
// the kernels' geometry, whichever path a context with those flags would take
static bool TwoPassTables(mpcvr::Resizer rx, mpcvr::Resizer ry, int src_w, int src_h, int out_w, int out_h, int iUpscaling, uint32_t flags, mpcvr::PlanTables *t)
{
    mpcvr::PassPlan plan;
    plan.two_pass = true;
    plan.rx = plan.first_rs = rx; plan.ry = ry;
    plan.first_tex_axis = 0;
    plan.mid_h = src_h;
    mpcvr::PlanTablesInput in;
    in.srcRectW = in.texW = src_w; in.srcRectH = in.texH = src_h;
    in.outW = out_w; in.outH = out_h;
    in.iUpscaling = iUpscaling;
    in.flags = flags & ~(uint32_t)(MPCVR_FLAG_NO_FUSED | MPCVR_FLAG_NO_FAST_CONVERT | MPCVR_FLAG_NO_STRIP);
    in.heavyConvert = true;
    std::string why;
    return mpcvr::BuildPlanTables(plan, in, t, &why) && t->stripPlanned;
}

int32_t mpcvr_plan_strip(int32_t kind_x, int32_t method_x, int32_t kind_y, int32_t method_y, int32_t src_w, int32_t src_h,
                         int32_t out_w, int32_t out_h, uint32_t flags, int32_t out8[8], int32_t *yrange, int32_t *xstrip,
                         int32_t *xi_t, float *xw_t, int32_t *yi, float *yw)
{
    if (!out8) return MPCVR_E_POINTER;
    if (src_w <= 0 || src_h <= 0 || out_w <= 0 || out_h <= 0) return MPCVR_E_INVALIDARG;
    mpcvr::PlanTables t;
    if (!TwoPassTables(mpcvr::Resizer{kind_x, method_x}, mpcvr::Resizer{kind_y, method_y}, src_w, src_h, out_w, out_h, method_x, flags, &t)) return MPCVR_E_NOTIMPL;
    const mpcvr::StripPlan &sp = t.strip;
    const int strips = (out_w + sp.strip_w - 1) / sp.strip_w;
    const int per_wave = 2 * sp.acols * 8 + sp.ring * 64 * (sp.pxl == 2 ? 12 : 8);
    const int32_t o[8] = {sp.nt, sp.pxl, sp.strip_w, sp.ring, sp.acols, strips, per_wave, 0};
    std::memcpy(out8, o, sizeof(o));
    if (yrange) std::memcpy(yrange, sp.yrange.data(), sp.yrange.size() * sizeof(int32_t));
    if (xstrip) std::memcpy(xstrip, sp.xstrip.data(), sp.xstrip.size() * sizeof(int32_t));
    if (xi_t) std::memcpy(xi_t, sp.xi_t.data(), sp.xi_t.size() * sizeof(int32_t));
    if (xw_t) std::memcpy(xw_t, sp.xw_t.data(), sp.xw_t.size() * sizeof(float));
    if (yi) std::memcpy(yi, sp.yi.data(), sp.yi.size() * sizeof(int32_t));
    if (yw) std::memcpy(yw, sp.yw.data(), sp.yw.size() * sizeof(float));
    return MPCVR_S_OK;
}

int32_t mpcvr_plan_period(int32_t method, int32_t src_w, int32_t src_h, int32_t out_w, int32_t out_h, uint32_t flags,
                          int32_t out6[6], int32_t *xi_t, float *xw_t, float *yw, int32_t *xstrip, int32_t *strip_w)
{
    if (!out6) return MPCVR_E_POINTER;
    if (src_w <= 0 || src_h <= 0 || out_w <= 0 || out_h <= 0) return MPCVR_E_INVALIDARG;
    mpcvr::PlanTables t;
    const mpcvr::Resizer up{mpcvr::RS_UP, method};
    if (!TwoPassTables(up, up, src_w, src_h, out_w, out_h, method, flags, &t) || !t.period.P) return MPCVR_E_NOTIMPL;
    const mpcvr::PeriodPlan &pp = t.period;
    const int32_t o[6] = {pp.P, pp.Q, pp.nt, (out_w + pp.strip_w - 1) / pp.strip_w, pp.acols, 6 * pp.P / pp.Q};
    if (strip_w) *strip_w = pp.strip_w;
    std::memcpy(out6, o, sizeof(o));
    if (xi_t) std::memcpy(xi_t, pp.xi_t.data(), pp.xi_t.size() * sizeof(int32_t));
    if (xw_t) std::memcpy(xw_t, pp.xw_t.data(), pp.xw_t.size() * sizeof(float));
    if (yw) std::memcpy(yw, pp.yw.data(), pp.yw.size() * sizeof(float));
    if (xstrip) std::memcpy(xstrip, pp.xstrip.data(), pp.xstrip.size() * sizeof(int32_t));
    return MPCVR_S_OK;
}

int32_t mpcvr_plan_draw_tables(const mpcvr_settings *s, int32_t cformat, int32_t src_w, int32_t src_h, const mpcvr_rect *src_rect,
                               const mpcvr_rect *video_rect, int32_t window_w, int32_t window_h, int32_t rotation, int32_t flip,
                               void *buf, size_t *size)
{
    if (!s || !video_rect || !size) return MPCVR_E_POINTER;
    const mpcvr::FmtConvParams *f = mpcvr::GetFmtConvParams(cformat);
    if (!f) return MPCVR_E_NOTIMPL;
    const mpcvr_rect whole{0, 0, src_w, src_h};
    const mpcvr_rect r = src_rect ? *src_rect : whole;
    const int w1 = r.right - r.left, h1 = r.bottom - r.top;
    if (src_w <= 0 || src_h <= 0 || r.left < 0 || r.top < 0 || r.right > src_w || r.bottom > src_h || w1 <= 0 || h1 <= 0 ||
        video_rect->right <= video_rect->left || video_rect->bottom <= video_rect->top || window_w <= 0 || window_h <= 0 ||
        (rotation != 0 && rotation != 90 && rotation != 180 && rotation != 270)) return MPCVR_E_INVALIDARG;
    // a context fresh from mpcvr_set_input: default ProcAmp, the extended format's defaults, no HDR output, no Dolby Vision
    const mpcvr::PlanGeometry g{w1, h1, video_rect->left, video_rect->top, video_rect->right, video_rect->bottom, window_w, window_h,
                                rotation, flip ? 1 : 0, mpcvr::ConvertDrawEnabled(*f, mpcvr::ProcAmp(), false) ? 1 : 0, 0, 0};
    mpcvr::PassPlan plan;
    std::string why;
    if (!mpcvr::DecidePlan(s->iTexFormat, s->iChromaScaling, s->iUpscaling, s->iDownscaling, s->bInterpolateAt50pct,
                           s->bUseDither, s->output_format, s->flags, *f, g, &plan, &why)) return MPCVR_E_NOTIMPL;
    int tail = 0; float gamma = 1.0f;
    mpcvr::SelectTail(mpcvr::SpecifyExtendedFormat(mpcvr::ExtFmt{0}, *f, w1, h1), s->bConvertToSdr != 0, &tail, &gamma);
    const mpcvr::PlanTablesInput in{r.left, r.top, w1, h1, src_w, src_h, video_rect->right - video_rect->left, video_rect->bottom - video_rect->top,
                                    s->iUpscaling, s->flags, tail == mpcvr::TAIL_PQ_TO_SDR || tail == mpcvr::TAIL_HLG_TO_SDR, false};
    mpcvr::PlanTables t;
    if (!mpcvr::BuildPlanTables(plan, in, &t, &why)) return MPCVR_E_NOTIMPL;

    int32_t h[MPCVR_DRAW_TABLES_HEADER_WORDS] = {0};
    size_t at = MPCVR_DRAW_TABLES_HEADER_WORDS;
    h[0] = MPCVR_DRAW_TABLES_HEADER_WORDS;
    h[1] = t.firstAxis; h[2] = t.firstSwap; h[3] = t.firstJinc; h[4] = t.secondJinc; h[5] = t.stripPlanned; h[6] = t.period.P; h[7] = t.period.Q;
    const mpcvr::AxisPack *axes[2] = {&t.x, &t.y};
    for (int a = 0; a < 2; a++) {
        const mpcvr::AxisPack &p = *axes[a];
        int32_t *o = h + 8 + 16 * a;
        o[0] = (int32_t)at; o[1] = (int32_t)p.words.size();
        o[2] = p.ntaps; o[3] = p.normalise; o[4] = p.n_out; o[5] = p.blk_span; o[6] = p.blk8_span; o[7] = p.blk32_span; o[8] = p.other_identity;
        o[9] = (int32_t)p.offIdx; o[10] = (int32_t)p.offW; o[11] = p.normalise ? (int32_t)p.offWsum : -1; o[12] = (int32_t)p.offOther;
        o[13] = p.n_out > 0 ? (int32_t)p.offBlk : -1; o[14] = (int32_t)p.nOther;
        at += p.words.size();
    }
    int32_t *o = h + 40;
    o[0] = (int32_t)at; o[1] = (int32_t)t.stripPack.words.size();
    for (int i = 0; i < 6; i++) o[2 + i] = (int32_t)t.stripPack.stripOff[i];
    for (int i = 0; i < 4; i++) o[8 + i] = (int32_t)t.stripPack.periodOff[i];
    o[12] = t.strip.nt; o[13] = t.strip.pxl; o[14] = t.strip.strip_w; o[15] = t.strip.ring; o[16] = t.strip.acols;
    o[17] = t.period.nt; o[18] = t.period.acols; o[19] = t.period.strip_w; o[20] = t.period.own;
    at += t.stripPack.words.size();

    const size_t need = at * sizeof(int32_t);
    if (!buf) { *size = need; return MPCVR_S_OK; }
    if (*size < need) { *size = need; return MPCVR_E_INVALIDARG; }
    int32_t *out = (int32_t *)buf;
    std::memcpy(out, h, sizeof(h));
    out += MPCVR_DRAW_TABLES_HEADER_WORDS;
    for (const std::vector<int32_t> *w : {&t.x.words, &t.y.words, &t.stripPack.words}) {
        if (!w->empty()) std::memcpy(out, w->data(), w->size() * sizeof(int32_t));
        out += w->size();
    }
    *size = need;
    return MPCVR_S_OK;
}

int32_t mpcvr_plan_hdr10_params(float min_mastering, float max_mastering, float max_cll, float max_fall, float display_max,
                                int32_t selection, uint32_t out6[6])
{
    if (!out6) return MPCVR_E_POINTER;
    mpcvr::HdrToneMapParams k{min_mastering, max_mastering, max_cll, max_fall, display_max, selection};
    mpcvr::SanitiseHdr10Params(&k);
    std::memcpy(out6, &k, 20);
    out6[5] = (uint32_t)k.selection;
    return MPCVR_S_OK;
}

int32_t mpcvr_plan_pq_eotf_table(float *out, int32_t capacity, int32_t *count)
{
    constexpr int32_t n = mpcvr::kEotfLutSize + 1;
    if (count) *count = n;
    if (!out) return count ? MPCVR_S_OK : MPCVR_E_POINTER;
    if (capacity < n) return MPCVR_E_INVALIDARG;
    mpcvr::BuildPqEotfLut(out);
    return MPCVR_S_OK;
}

// DEPRECATED (kept so that a caller built against the round-3 header still links and cannot be overrun): the same function on the 4096-entry
// grid that header promised, computed from the table's definition (vp_plan.cpp BuildPqEotfLut), not cut out of the larger table
int32_t mpcvr_plan_pq_eotf_lut(float out[4096])
{
    if (!out) return MPCVR_E_POINTER;
    const double m1 = 2610.0 / (4096.0 * 4.0), m2 = (2523.0 / 4096.0) * 128.0;
    const double c1 = 3424.0 / 4096.0, c2 = (2413.0 / 4096.0) * 32.0, c3 = (2392.0 / 4096.0) * 32.0;
    for (int i = 0; i < 4096; i++) {
        const double t = (double)i / 4095.0;
        double x = std::pow(t * t, 1.0 / m2);
        x = std::fmax(x - c1, 0.0) / (c2 - c3 * x);
        const double l = x > 0.0 ? std::log2(x) / m1 : -1e9;
        out[i] = l > -150.0 ? (float)l : -150.0f;
    }
    return MPCVR_S_OK;
}

int32_t mpcvr_plan_describe(const mpcvr_settings *s, int32_t cformat, int32_t rect_w, int32_t rect_h,
                            const mpcvr_rect *video_rect, int32_t window_w, int32_t window_h,
                            char *buf, size_t buf_size)
{
    if (!s || !video_rect || !buf || !buf_size) return MPCVR_E_POINTER;
    const mpcvr::FmtConvParams *f = mpcvr::GetFmtConvParams(cformat);
    if (!f) return MPCVR_E_NOTIMPL;
    const mpcvr::PlanGeometry g{rect_w, rect_h, video_rect->left, video_rect->top, video_rect->right,
                                video_rect->bottom, window_w, window_h};
    mpcvr::PassPlan plan;
    std::string why;
    if (!mpcvr::DecidePlan(s->iTexFormat, s->iChromaScaling, s->iUpscaling, s->iDownscaling, s->bInterpolateAt50pct,
                           s->bUseDither, s->output_format, s->flags, *f, g, &plan, &why)) {
        std::snprintf(buf, buf_size, "%s", why.c_str());
        return MPCVR_E_NOTIMPL;
    }
    std::snprintf(buf, buf_size, "%s;internal=%d;swap=%d;final=%d", plan.describe().c_str(), plan.internal_fmt,
                  plan.swap_fmt, plan.final_pass ? 1 : 0);
    return MPCVR_S_OK;
}

}  // extern "C"

// verification aid: the plain tier's Dolby Vision tail over an array, stage by stage (csrc/vp_kernels.hip: k_eval_dovi_tail)
int32_t mpcvr_eval_dovi_tail(int32_t stage, const float *rgb_dev, float *out_dev, size_t n, const float lms9[9], const float l2k5[5], int32_t l2_enabled, float lum_scale, void *stream)
{
    if (!rgb_dev || !out_dev || !lms9 || !l2k5) return MPCVR_E_POINTER;
    if (stage < 0 || stage > 5) return MPCVR_E_INVALIDARG;
    float gamut[9];
    mpcvr::ComputeGamut2020to709(gamut);
    return mpcvr::LaunchEvalDoviTail(rgb_dev, out_dev, n, lms9, l2k5, gamut, l2_enabled, lum_scale, stage, (hipStream_t)stream) == hipSuccess ? MPCVR_S_OK : MPCVR_E_FAIL;
}
