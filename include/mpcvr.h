/*
 * mpcvr.h — C-ABI of the MI355X-native shader video processor (libmpcvr.so).
 *
 * Drop-in boundary for ONE path of MPC Video Renderer: CDX11VideoProcessor::Process on the shader
 * video processor (convert -> resize -> final pass/dither).  The reference has no FFI; its narrowest
 * waist is the C++ virtual class CVideoProcessor (Source/VideoProcessor.h:40-296) as implemented by
 * CDX11VideoProcessor (Source/DX11VideoProcessor.h:256-384).  Each export below names the method it
 * replaces (file:line relative to the reference tree).  Plain pointers and sizes only.
 *
 * Conventions (mirroring the reference):
 *   - return type int32_t == HRESULT sign convention: 0 = S_OK, 1 = S_FALSE ("ok, nothing done"),
 *     negative = failure (MPCVR_E_*).
 *   - the processor owns all device resources; input sample memory is borrowed for the duration of
 *     mpcvr_copy_sample; output goes to caller-owned memory.
 *   - NOT re-entrant: one caller at a time per context (the reference serialises every entry under
 *     m_RendererLock, VideoRenderer.cpp:443-444,579-586).  Work is asynchronous on the context's HIP
 *     stream unless stated otherwise.
 */
#ifndef MPCVR_H
#define MPCVR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCVR_S_OK            0
#define MPCVR_S_FALSE         1
#define MPCVR_E_FAIL          ((int32_t)0x80004005)
#define MPCVR_E_POINTER       ((int32_t)0x80004003)
#define MPCVR_E_INVALIDARG    ((int32_t)0x80070057)
#define MPCVR_E_UNEXPECTED    ((int32_t)0x8000FFFF)
#define MPCVR_E_NOTIMPL       ((int32_t)0x80004001)
#define MPCVR_E_OUTOFMEMORY   ((int32_t)0x8007000E)
#define MPCVR_E_NOT_VALID_STATE ((int32_t)0x8007139F)

/* ColorFormat_t — Source/Helper.h:86-127 (same numeric values; the formats this build accepts). */
enum mpcvr_cformat {
    MPCVR_CF_NONE = 0,
    MPCVR_CF_NV12 = 1, MPCVR_CF_P010 = 2, MPCVR_CF_P016 = 3,
    MPCVR_CF_YUY2 = 4, MPCVR_CF_UYVY = 5,
    MPCVR_CF_P210 = 6, MPCVR_CF_P216 = 7,
    MPCVR_CF_Y210 = 8, MPCVR_CF_Y216 = 9, MPCVR_CF_V210 = 10,
    MPCVR_CF_AYUV = 11, MPCVR_CF_Y410 = 12, MPCVR_CF_Y416 = 13,
    MPCVR_CF_YV12 = 14, MPCVR_CF_YV16 = 15, MPCVR_CF_YV24 = 16,
    MPCVR_CF_YUV420P8 = 17, MPCVR_CF_YUV422P8 = 18, MPCVR_CF_YUV444P8 = 19,
    MPCVR_CF_YUV420P10 = 20, MPCVR_CF_YUV420P16 = 21,
    MPCVR_CF_YUV422P10 = 22, MPCVR_CF_YUV422P16 = 23,
    MPCVR_CF_YUV444P10 = 24, MPCVR_CF_YUV444P16 = 25,
    MPCVR_CF_GBRP8 = 26, MPCVR_CF_GBRP10 = 27, MPCVR_CF_GBRP16 = 28,
    MPCVR_CF_RGB24 = 29, MPCVR_CF_XRGB32 = 30, MPCVR_CF_ARGB32 = 31, MPCVR_CF_r210 = 32,
    MPCVR_CF_RGB48 = 33, MPCVR_CF_BGR48 = 34, MPCVR_CF_BGRA64 = 35, MPCVR_CF_B64A = 36,
    MPCVR_CF_Y8 = 37, MPCVR_CF_Y10 = 38, MPCVR_CF_Y16 = 39
};

/* Settings enums — Source/IVideoRenderer.h:25-72 (identical values). */
enum { MPCVR_TEXFMT_AUTOINT = 0, MPCVR_TEXFMT_8INT = 8, MPCVR_TEXFMT_10INT = 10, MPCVR_TEXFMT_16FLOAT = 16 };
enum { MPCVR_CHROMA_Nearest = 0, MPCVR_CHROMA_Bilinear = 1, MPCVR_CHROMA_CatmullRom = 2 };
enum { MPCVR_UPSCALE_Nearest = 0, MPCVR_UPSCALE_Mitchell = 1, MPCVR_UPSCALE_CatmullRom = 2,
       MPCVR_UPSCALE_Lanczos2 = 3, MPCVR_UPSCALE_Lanczos3 = 4, MPCVR_UPSCALE_Jinc2 = 5,
       /* EXTENSION — not a reference setting (IVideoRenderer.h:54-62 ends at Jinc2): the 6-tap Spline36 kernel, BASELINE.json
        * config 4's optional run.  Same draws, tap positions and intermediate formats as the other interpolation shaders. */
       MPCVR_UPSCALE_Spline36_EXT = 6 };
enum { MPCVR_DOWNSCALE_Box = 0, MPCVR_DOWNSCALE_Bilinear = 1, MPCVR_DOWNSCALE_Hamming = 2,
       MPCVR_DOWNSCALE_Bicubic = 3, MPCVR_DOWNSCALE_BicubicSharp = 4, MPCVR_DOWNSCALE_Lanczos = 5 };

/* mpcvr_settings.bUseDither: 0 / 1 as the reference's bool (Settings_t::bUseDither, IVideoRenderer.h:117: the ordered dither of
 * ps_final_pass.hlsl).  EXTENSION — 2 is not a reference setting (the reference has no error diffusion at all): BASELINE.json config 4's
 * "error-diffusion dither".  Where the reference would run its final pass into an 8-bit target (internal format above 8 bits), the
 * frame is rendered as for a 10-bit swap chain (R10G10B10A2: no final pass behind the 10-bit internal format; behind the fp16 internal
 * format that chain's own final pass — the ordered dither from fp16 to 10 bits, as the reference runs it there — stays in front of the
 * pass) and Floyd-Steinberg error diffusion in integers takes it to B8G8R8A8 inside video rect ∩ window (definition: csrc/vp_errdiff_core.h; the serial model in oracle/ is its only check).  On a
 * 10-bit target or with the 8-bit internal format it changes nothing, like bUseDither = 1 there.
 * The pass is a chain of bands that wait for each other through device memory; its forward progress does not depend on the order in which
 * the hardware starts workgroups (bands are taken by ticket).  Should a band ever give up waiting (a bounded number of polls), the frame is
 * wrong and the pass flags it: mpcvr_synchronize, mpcvr_get_current_image and the next error-diffusion pass answer MPCVR_E_FAIL — a caller
 * that synchronises its OWN stream instead must call mpcvr_synchronize before it trusts such a frame. */
enum { MPCVR_DITHER_None = 0, MPCVR_DITHER_Ordered = 1, MPCVR_DITHER_ErrorDiffusion_EXT = 2 };

/* Render-target format: stands in for the display-driven m_SwapChainFmt decision
 * (DX11VideoProcessor.cpp:1476-1478, Preferred10BitOutput DX11VideoProcessor.h:290-292). */
enum { MPCVR_OUT_BGRA8 = 0, MPCVR_OUT_RGB10A2 = 1 };

/* mpcvr_settings.flags */
#define MPCVR_FLAG_LANCZOS3_FIXED   0x1u  /* use the D3D9 twin's tap layout instead of the D3D11 shader's (quirk Q1) */
#define MPCVR_FLAG_NO_FUSED         0x2u  /* plain pass-per-kernel path only: no fused 2x kernel, no convert+final in one kernel,
                                             no compile-time-folded kernels, every tail literal (debug / A-B; bit-exact reference) */
#define MPCVR_FLAG_NO_LUT           0x4u  /* evaluate the PQ->SDR chain in ALU instead of the 4096-entry table (fused and folded kernels) */
#define MPCVR_FLAG_NO_FAST_CONVERT  0x8u  /* fused 2x kernel off when its vectorised convert would be needed: the folded pass-per-kernel
                                             path runs instead (debug / A-B) */

#define MPCVR_FLAG_FUSED_VALU       0x10u /* fused 2x kernel with its resize taps as packed-fp32 VALU chains (k_fused_up2x) */
#define MPCVR_FLAG_FUSED_MFMA       0x20u /* accepted and ignored since round 6 (it selected an experiment kernel with the resize taps on the matrix
                                             cores: parity-green, never faster; kept under profiles/r06/experiments/matrix_core_taps/) */
#define MPCVR_FLAG_NO_STRIP         0x40u /* arbitrary-ratio resizes of 4:2:0 sources stay on the block convert + tiled two-draw
                                             kernels instead of the one-kernel strip path (k_fused_strip; debug / A-B) */
#define MPCVR_FLAG_FORCE_PERIOD     0x100u /* take k_fused_period wherever it is built (debug / A-B).  Since round 6 that is where the planner takes it
                                              anyway: the one class it used to add — SDR content with a 4-tap filter, where k_fused_strip is as fast —
                                              is no longer built (35 instantiations, a tenth of the build) */
#define MPCVR_FLAG_NO_FRAME_LANES   0x200u /* mpcvr_process strictly one frame after the other.  Default: a context that owns its stream (no
                                              mpcvr_set_stream) deals consecutive single frames to four internal streams so that one frame's drain
                                              overlaps the next one's ramp-up — frames are independent, as the reference's draws into different
                                              render targets are for the D3D11 driver (Render -> Process, DX11VideoProcessor.cpp:2730).  Results are
                                              complete after mpcvr_synchronize (or any call that reads them back); frames into the SAME target
                                              stay in order.  (debug / A-B) */
#define MPCVR_FLAG_NO_PERIOD        0x80u /* rational vertical ratios (4:3, 3:2, 2:3, 1:2, 3:1) through k_fused_strip's run-time tap tables instead
                                             of the periodic-phase kernel with its register window (k_fused_period; debug / A-B) */

/* Subset of Settings_t (IVideoRenderer.h:104-135) that reaches the shader path; same field names. */
typedef struct mpcvr_settings {
    int32_t  iTexFormat;          /* MPCVR_TEXFMT_*            default AUTOINT   */
    int32_t  iChromaScaling;      /* MPCVR_CHROMA_*            default Bilinear  */
    int32_t  iUpscaling;          /* MPCVR_UPSCALE_*           default CatmullRom*/
    int32_t  iDownscaling;        /* MPCVR_DOWNSCALE_*         default Hamming   */
    int32_t  bInterpolateAt50pct; /*                           default 1         */
    int32_t  bUseDither;          /* MPCVR_DITHER_*            default 1 (Ordered) */
    int32_t  bDeintBlend;         /* blend-deinterlace 4:2:0 samples flagged interlaced (mpcvr_set_sample_format) */
    int32_t  bConvertToSdr;       /*                           default 1         */
    int32_t  iSDRDisplayNits;     /* 25..400                   default 125       */
                                  /* (24 and 401 are MPCVR_E_INVALIDARG from mpcvr_create and mpcvr_configure, which then changes nothing) */
    int32_t  output_format;       /* MPCVR_OUT_*               default BGRA8     */
    uint32_t flags;
} mpcvr_settings;

typedef struct mpcvr_rect { int32_t left, top, right, bottom; } mpcvr_rect;

/* mem_kind for mpcvr_copy_sample */
enum { MPCVR_MEM_HOST = 0, MPCVR_MEM_DEVICE = 1, MPCVR_MEM_HOST_PINNED = 2 };

/* ProcAmp flags — DXVA2_ProcAmp_* bit values */
#define MPCVR_PROCAMP_BRIGHTNESS 0x1
#define MPCVR_PROCAMP_CONTRAST   0x2
#define MPCVR_PROCAMP_HUE        0x4
#define MPCVR_PROCAMP_SATURATION 0x8

typedef struct mpcvr_ctx mpcvr_ctx;

/* Settings_t::SetDefault — IVideoRenderer.h:140-185 */
int32_t mpcvr_settings_default(mpcvr_settings *s);

/* ctor + Init — DX11VideoProcessor.cpp:381,547.  `device` = HIP device ordinal. */
int32_t mpcvr_create(const mpcvr_settings *settings, int32_t device, mpcvr_ctx **out);
int32_t mpcvr_destroy(mpcvr_ctx *ctx);

/* Use an externally owned hipStream_t (e.g. torch's current stream) for all work.  NULL = the context's own stream, which is a
 * BLOCKING stream (hipStreamDefault): it synchronises implicitly with the legacy null stream, so work a caller queued on stream 0
 * (NULL is also that stream's handle) stays ordered against mpcvr_copy_sample / mpcvr_process.  Other streams are the caller's to
 * order (events), as usual. */
int32_t mpcvr_set_stream(mpcvr_ctx *ctx, void *hip_stream);
int32_t mpcvr_synchronize(mpcvr_ctx *ctx);

/* VerifyMediaType + InitMediaType — DX11VideoProcessor.cpp:1569,1742.
 * cformat: ColorFormat_t value; width/height: biWidth/|biHeight|; pitch: bytes per luma row of the
 * samples that will be handed to mpcvr_copy_sample (0 => the reference's rule, :1789-1803; negative for an RGB format
 * = bottom-up DIB, the way m_srcPitch goes negative for BI_RGB with biHeight > 0, :1801-1803).
 *   Pitch rules (anything else: E_INVALIDARG) — |pitch| is at least one row of pixels (width * bytes per pixel; v210: whole 16-byte groups
 *   of six pixels); even for 16-bit samples; a multiple of 4 for 32-bit texels (Y410, r210) and v210; the two chroma planes of a three-plane
 *   format lie at pitch / div_w (integer division, div_w = 2 for 4:2:0 and 4:2:2) behind pitch * height bytes of luma, and for 16-bit samples
 *   that chroma pitch must be even too (YUV420P10/16, YUV422P10/16: a luma pitch that is a multiple of 4).  A sample is pitch * lines bytes
 *   (mpcvr_get_frame_bytes).  Bytes of a row behind its pixels, and bytes behind the last plane, are never read into a pixel: they may hold
 *   anything.  For the interleaved RGB formats the pitch, not the width, drives the reference's copy loops (Helper.cpp:446-482, 541-565):
 *   RGB48 fills whole groups of four texels of |pitch| / 6 and RGB24 one texel of a remainder of three of |pitch| / 3, so the last texels of
 *   a row whose width is no multiple of 4 are black or filled depending on the pitch — as in the reference;
 *   Any legal pitch up to INT32_MAX is rendered correctly — a small frame carved out of a large pooled surface may have rows tens of MiB
 *   apart.  The fused kernels address rows and chroma planes with 32-bit offsets and step aside (mpcvr_get_path_info says what ran) where a
 *   chroma plane — or, for formats with fewer than three planes, the sum pitch * height + chroma pitch * chroma rows the library forms all
 *   the same — starts at or beyond 2 GiB, or the rows read span 4 GiB; the convert kernel and the resize draws take such a sample;
 * src_rect: rcSource (NULL or empty => whole frame, :1821-1823);
 * extfmt: DXVA2_ExtendedFormat.value from the media type (0 fields are defaulted per
 * SpecifyExtendedFormat, Helper.cpp:1169-1211).  Returns S_OK, or E_INVALIDARG/E_NOTIMPL. */
int32_t mpcvr_set_input(mpcvr_ctx *ctx, int32_t cformat, int32_t width, int32_t height, int32_t pitch,
                        const mpcvr_rect *src_rect, uint32_t extfmt);

/* SetVideoRect / SetWindowRect — DX11VideoProcessor.cpp:3426-3451.  Window rect = render-target size. */
int32_t mpcvr_set_video_rect(mpcvr_ctx *ctx, const mpcvr_rect *video_rect);
int32_t mpcvr_set_window_rect(mpcvr_ctx *ctx, const mpcvr_rect *window_rect);
/* SetRotation (DX11VideoProcessor.cpp:4052) / SetFlip (VideoProcessor.h:210): 0/90/180/270 degrees clockwise and a
 * horizontal flip of the source, applied in the first resize draw the way FillVertices (:130-179) and ResizeShaderPass
 * (:3112-3137) set it up; the caller sizes the video rect for the rotated picture.  E_INVALIDARG for other angles. */
int32_t mpcvr_set_rotation(mpcvr_ctx *ctx, int32_t degrees);
/* (extension, error-diffusion final pass only) how many polls — about a microsecond each — a band grants the band above before the pass is
 * flagged failed (the next mpcvr_process / mpcvr_synchronize answers MPCVR_E_FAIL instead of hanging); polls <= 0: the default, 2^21.  A host
 * that shares the GPU or runs under a debugger raises it; the environment variable MPCVR_ERRDIFF_SPIN (tests) overrides it per call. */
int32_t mpcvr_set_error_diffusion_patience(mpcvr_ctx *ctx, int32_t polls);
int32_t mpcvr_set_flip(mpcvr_ctx *ctx, int32_t flip);
/* m_SampleFormat as CopySample derives it from AM_SAMPLE2_PROPERTIES::dwTypeSpecificFlags (DX11VideoProcessor.cpp:2209-2219):
 * 0 progressive, 1 interlaced top field first, 2 interlaced bottom field first.  With bDeintBlend an interlaced 4:2:0
 * sample goes through the blend variant of the convert shader (:3075, Shaders.cpp:232-237). */
int32_t mpcvr_set_sample_format(mpcvr_ctx *ctx, int32_t frame_format);
/* HDR output: `enable` stands in for m_bHdrPassthroughSupport && (m_bHdrPassthrough || m_bHdrLocalToneMapping) — the
 * display is in HDR10 mode — so PQ sources pass through unconverted and HLG is converted to PQ (convertType,
 * DX11VideoProcessor.cpp:2948-2950); pick output_format RGB10A2 as the reference's swap chain does.  tone_map_type =
 * m_iHdrLocalToneMappingType (0 off, 1 ACES, 2 Reinhard, 3 Habel, 4 Moebius, 5 BT.2390, 6 ST 2094-10), display_max_nits =
 * m_iHdrDisplayMaxNits: ps_hdr10_tonemap.hlsl then runs as a post-scale step once mpcvr_set_hdr_metadata was called. */
int32_t mpcvr_set_hdr_output(mpcvr_ctx *ctx, int32_t enable, int32_t tone_map_type, float display_max_nits);
/* the values Render() passes to SetHDR10ShaderParams (:907-917, :2716-2727), sanitised the same way: min <= 0 is 0, a mastering peak <= 10 is
 * 1000, MaxCLL <= 10 is the mastering peak, MaxFALL <= 1 is MaxCLL, and a display peak outside 100 .. 10000 is drawn as 1000
 * (mpcvr_plan_hdr10_params returns the sanitised values without a GPU).  There is no upper clamp, as in the reference: keep the peaks within
 * what HDR10's 16-bit fields carry (<= 65535 nits).  The values travel with each launch: changing them, or the display peak, between two
 * mpcvr_process calls needs no mpcvr_synchronize. */
int32_t mpcvr_set_hdr_metadata(mpcvr_ctx *ctx, float min_mastering_nits, float max_mastering_nits, float max_cll, float max_fall);

/* Dolby Vision RPU of the next sample(s): the fields of MediaSideDataDOVIMetadata (Include/IMediaSideData.h:154-330) the
 * frame path reads when CopySample finds IID_MediaSideDataDOVIMetadataV2 on the sample (DX11VideoProcessor.cpp:2270-2520).
 * The reference struct is #pragma pack(1); this one has natural C alignment, the adapter copies field by field.
 * Extension blocks: the first level-1 block (+ the first level-3 block, if any) and every level-2 block, in
 * Extensions[] order. */
typedef struct mpcvr_dovi_curve {
    uint8_t  num_pivots;            /* [2, 9] */
    uint8_t  mapping_idc[8];        /* 0 polynomial, 1 mmr */
    uint8_t  poly_order[8];         /* [1, 2] */
    uint8_t  mmr_order[8];          /* [1, 3] */
    uint16_t pivots[9];             /* sorted ascending, bl_bit_depth codes */
    int64_t  poly_coef[8][3];       /* x^0, x^1, x^2 ; fixed point, coef_log2_denom fractional bits */
    int64_t  mmr_constant[8];
    int64_t  mmr_coef[8][3][7];
} mpcvr_dovi_curve;
typedef struct mpcvr_dovi_l2 {
    uint16_t target_max_pq, trim_slope, trim_offset, trim_power, trim_chroma_weight, trim_saturation_gain;
} mpcvr_dovi_l2;
typedef struct mpcvr_dovi_metadata {
    uint8_t  bl_bit_depth, coef_log2_denom;                 /* Header */
    uint16_t source_max_pq;                                 /* ColorMetadata */
    uint8_t  l1_present, l3_present;
    uint16_t l1_min_pq, l1_max_pq, l1_avg_pq, l3_min_pq_offset, l3_max_pq_offset, l3_avg_pq_offset;
    uint32_t n_l2;                                          /* <= 32 (LAV_DOVI_MAX_EXTENSIONS) */
    mpcvr_dovi_l2 l2[32];
    double   ycc_to_rgb_matrix[9], ycc_to_rgb_offset[3], rgb_to_lms_matrix[9];   /* ColorMetadata */
    mpcvr_dovi_curve curves[3];                             /* Mapping.curves, per component */
} mpcvr_dovi_metadata;
/* m_Dovi.msd = *md, m_Dovi.bValid = true: the convert pass reshapes (Y,U,V) through the curves (ShaderDoviReshape[Poly],
 * Shaders.cpp:531-589), uses ycc_to_rgb_matrix/offset as the colour matrix (SetShaderConvertColorParams :817-834), goes
 * PQ -> linear -> dovi_lms2rgb x rgb_to_lms_matrix -> PQ (Shaders.cpp:826-859) and continues as a PQ source; level-2 trims
 * are selected for the display peak of mpcvr_set_hdr_output (:2383-2469) and applied in the convert tail (SDR output) and
 * the tone-mapping step (HDR output); level 1 (+3) replaces the HDR10 metadata of that step (:2716-2720).
 * md == NULL ends Dolby Vision mode (m_Dovi = {}).  E_INVALIDARG for what CheckDoviMetadata rejects in the curves
 * (VideoProcessor.cpp:283-292); the profile checks on the RPU header (:275-281) stay with the adapter.
 * Kernels: the reshaping, the LMS step and the tail run in the 2x2-block convert (k_convert_blocks<..., DV_*>: same-size frames in
 * one kernel, straight into the render target; in front of k_fused_strip:surface / k_fused_period:surface when the frame is
 * resized); the exact-2x and the raw-sample strip kernels have no reshaping stage.  The metadata is per context: every frame of an
 * mpcvr_process_batch call runs on the RPU last set (mpcvr_process_batch_dovi takes one RPU per frame). */
int32_t mpcvr_set_dovi_metadata(mpcvr_ctx *ctx, const mpcvr_dovi_metadata *md);

/* The correction shaders (m_pPSCorrection, DX11VideoProcessor.cpp:1893-1930): same-size RGB -> RGB passes the reference runs
 * over the OUTPUT of the fixed-function D3D11 video processor (Process :3354-3357) — BT.2020 / YCgCo matrix fix-ups and the
 * PQ / HLG tone mapping that path cannot do itself.  The shader video processor of this library never needs them (its
 * convert pass does all of it before the resize); they are offered as standalone passes over one surface for a host that
 * decodes / scales elsewhere.  kind = MPCVR_CORR_*; src / dst: DEVICE surfaces of 32-bit texels, fmt = MPCVR_OUT_BGRA8 or
 * MPCVR_OUT_RGB10A2, w x h texels; sdr_nits = iSDRDisplayNits (LuminanceScale = 10000 / nits, :889-905); stream = a
 * hipStream_t or NULL.  In place (src == dst) is allowed. */
#define MPCVR_CORR_FIX_BT2020            1   /* Shaders/d3d11/ps_fix_bt2020.hlsl */
#define MPCVR_CORR_FIX_YCGCO             2   /* ps_fix_ycgco.hlsl */
#define MPCVR_CORR_FIXCONVERT_PQ_TO_SDR  3   /* ps_fixconvert_pq_to_sdr.hlsl */
#define MPCVR_CORR_FIXCONVERT_HLG_TO_SDR 4   /* ps_fixconvert_hlg_to_sdr.hlsl */
#define MPCVR_CORR_CONVERT_PQ_TO_SDR     5   /* ps_convert_pq_to_sdr.hlsl */
#define MPCVR_CORR_CONVERT_HLG_TO_PQ     6   /* ps_convert_hlg_to_pq.hlsl */
int32_t mpcvr_correction_pass(int32_t kind, const void *src, int32_t src_pitch, int32_t src_fmt,
                              void *dst, int32_t dst_pitch, int32_t dst_fmt, int32_t w, int32_t h, int32_t sdr_nits, void *stream);
/* the three matrices those shaders fold at compile time, evaluated in fp32: fix_bt2020_matrix and fix_ycgco_matrix (4x4,
 * row-major) and convert_matrix_2020_to_709 of convert/colorspace_gamut_conversion.hlsl (3x3) */
int32_t mpcvr_plan_correction_matrices(float fix_bt2020_16[16], float fix_ycgco_16[16], float gamut9[9]);

/* EXTENSION — rendered frames as NV12 / P010 for a video encoder or a 4:2:0 pipeline.  There is no reference line to cite: the reference
 * ends in a swap chain and has no RGB -> YCbCr path at all.  The pass is defined here, in integers, and anchored to this library's own
 * colour code: the sample it writes is the one mpcvr_set_input(NV12 | P010, extfmt) converts back to the same picture (to within the
 * quantisation of the codes; tests/test_encode.py measures it through the oracle).  tests/encode_model.py is the bit-exact model.
 *   Input: a DEVICE surface of w x h 32-bit texels, src_fmt = MPCVR_OUT_BGRA8 or MPCVR_OUT_RGB10A2; the channel codes R, G, B are integers
 *     in [0, maxin], maxin = 255 or 1023; the A / X bits are ignored.  w and h even, 2 .. 32768.
 *   Output: out_cformat = MPCVR_CF_NV12 (depth d = 8, one byte per component) or MPCVR_CF_P010 (d = 10, the code stored as code << 6 in 16
 *     bits, low six bits zero — this library's P010 reader takes all 16 bits): a Y plane of h rows and an interleaved (U, V) plane of h / 2
 *     rows, each with its own pointer and pitch.
 *   Colour description: extfmt is a DXVA2_ExtendedFormat value, defaulted by SpecifyExtendedFormat exactly as mpcvr_set_input defaults
 *     it for a w x h frame of out_cformat (mpcvr_plan_encode has no size: it defaults the matrix as for a frame of at most 1024 x 576,
 *     BT.601 — name the matrix to plan what a larger surface gets); its matrix, nominal-range and chroma-siting fields mean what they mean
 *     there.  A description that plans as RGB (value == 0 after the defaults) is MPCVR_E_INVALIDARG.
 *   Coefficients: M, c (3x3, 3) = what mpcvr_plan_color_matrix returns for (out_cformat, extfmt) with a neutral ProcAmp; T = 255 for NV12,
 *     65535 / 64 for P010.  On the host, in double, N = inverse(M) by the adjugate;
 *       coef[i][j] = rint(N[i][j] * T / maxin * 2^S),   off[i] = rint(-(N c)[i] * T * 2^S),   S = 16.
 *     Everything on the device is 32-bit integer arithmetic, shifts are arithmetic.
 *   Luma, one per pixel:   Y = clamp((coef[0] . (R, G, B) + off[0] + 2^(S-1)) >> S, 0, 2^d - 1).
 *   Chroma, one (U, V) pair per 2x2 block (2i, 2j): weighted sums SR, SG, SB of the codes by siting, taps beyond the surface replicating the
 *     edge texel —
 *       siting 0, centre (MPEG-1):        the four texels of the block, W = 4;
 *       siting 1, left (MPEG-2):          horizontal [1 2 1] centred on column 2i, over rows 2j and 2j + 1, W = 8;
 *       siting 2, top-left (co-sited):    [1 2 1] x [1 2 1] centred on (2i, 2j), W = 16;
 *     C = clamp((coef[k] . (SR, SG, SB) + W * off[k] + (W << (S-1))) >> (S + log2 W), 0, 2^d - 1), k = 1 (U), 2 (V).
 *     The chroma field of extfmt selects the siting as the convert path reads it for 4:2:0 input (csrc/hip_video_processor.cpp,
 *     P->chroma_loc, Shaders.cpp:121-137): 7 -> top-left, 1 -> centre, anything else -> left.
 *   Range of the arithmetic: the largest accumulator is 1.07e9 (P010 out, top-left siting, full range), under 2^31 - 1 for every
 *     matrix x range x format pair (tests/test_encode.py computes the bound from the planned integers), so S = 16 holds for all of them.
 *   No dithering: an RGB10A2 surface written as NV12 is rounded. */
/* the integers above, usable without a GPU.  coef9: rows Y, U, V, columns R, G, B.  Any out pointer may be NULL.  MPCVR_E_INVALIDARG for
 * an out_cformat that is neither NV12 nor P010 (RGB and gray formats included), another src_fmt, or an RGB description. */
int32_t mpcvr_plan_encode(int32_t out_cformat, int32_t src_fmt, uint32_t extfmt, int32_t coef9[9], int32_t off3[3], int32_t *shift,
                          int32_t *siting, uint32_t *extfmt_out);
/* One standalone pass over one device surface, like mpcvr_correction_pass; stream = a hipStream_t or NULL.  One kernel launch
 * (k_encode420, csrc/vp_encode.hip).  src, y_plane, uv_plane and the three pitches must be multiples of 4 (the render-target rule of
 * mpcvr_process; 8-byte stores and 16-byte loads are taken where pointers and pitches allow them), src_pitch >= 4 w, y_pitch and uv_pitch
 * >= one row of components (w bytes for NV12, 2 w for P010).  No byte outside the planes' pixels is written: not the pitch padding, nothing
 * in front of or behind a plane.  Refusals, with nothing launched: a NULL pointer MPCVR_E_POINTER; MPCVR_E_INVALIDARG for odd or
 * out-of-range w / h, the formats and descriptions mpcvr_plan_encode refuses, a pointer or pitch that breaks the rules above, and planes
 * that overlap each other or the source (a plane counts as the bytes from its first pixel to the last pixel of its last row). */
int32_t mpcvr_encode_pass(const void *src, int32_t src_pitch, int32_t src_fmt, int32_t w, int32_t h, int32_t out_cformat, uint32_t extfmt,
                          void *y_plane, int32_t y_pitch, void *uv_plane, int32_t uv_pitch, void *stream);
/* mpcvr_render, then the pass over the whole window: Process into the context-owned back buffer with the letterbox cleared to black, the
 * encode queued behind it in stream order (a frame rendered this way runs on the context stream, not on a frame lane; the pixels are the
 * same).  The planes are complete after mpcvr_synchronize; mpcvr_get_backbuffer and mpcvr_get_displayed_image afterwards see the RGB frame
 * a plain mpcvr_render leaves.  The source format is the context's output_format.  An odd window width or height, and everything
 * mpcvr_encode_pass refuses about the planes, is answered (MPCVR_E_INVALIDARG / MPCVR_E_POINTER) before anything is drawn.  S_FALSE, with
 * nothing drawn or written, when there is no sample (as mpcvr_render). */
int32_t mpcvr_render_yuv(mpcvr_ctx *ctx, int32_t field, int32_t out_cformat, uint32_t extfmt, void *y_plane, int32_t y_pitch,
                         void *uv_plane, int32_t uv_pitch);

/* EXTENSION — measuring what was rendered: the histogram of max(R, G, B), and MaxCLL / MaxFALL (CTA-861.3) from it.  The reference's
 * statistics are an on-screen overlay; there is no reference line to cite.  The definition is the integer text below, modelled bit for bit
 * by tests/measure_model.py.
 *   Input: a DEVICE surface of w x h 32-bit texels, src_fmt = MPCVR_OUT_BGRA8 (maxin = 255) or MPCVR_OUT_RGB10A2 (maxin = 1023), w and h in
 *   1 .. 32768 (odd sizes allowed), src and src_pitch multiples of 4, src_pitch >= 4 w; the A / X bits are ignored.
 *   rect = [left, right) x [top, bottom), non-empty and inside the surface, any parity and alignment; NULL = the whole surface.
 *   Output: uint32_t hist[MPCVR_HIST_BINS] in DEVICE memory, 4-byte aligned.  After the pass hist[c] = the number of texels of rect with
 *   max(R, G, B) == c (for BGRA8 the bins 256 .. 1023 are 0).  The pass OVERWRITES the 1024 words whatever they held and writes no other byte.
 * Counts are exact (the largest is 32768^2 = 2^30): every counter on the way is a 32-bit integer, so the result does not depend on the
 * order of the additions and is bit-reproducible.  The histogram is complete in stream order behind the call.
 * Refusals, with nothing launched and nothing written: MPCVR_E_POINTER for a NULL src or hist_dev; MPCVR_E_INVALIDARG for another src_fmt,
 * w or h out of range, a pointer or pitch that breaks the rules above, a rect that is empty or leaves the surface, and a histogram that
 * overlaps the surface (the surface counts as the bytes from its first pixel to the last pixel of its last row).
 * The same histogram serves SDR frames: black-frame detection, scene cuts, percentile peaks (mpcvr_histogram_percentile). */
#define MPCVR_HIST_BINS 1024
int32_t mpcvr_measure_pass(const void *src, int32_t src_pitch, int32_t src_fmt, int32_t w, int32_t h,
                           const mpcvr_rect *rect, uint32_t *hist_dev, void *stream);
/* The pass over the frame the last mpcvr_render / mpcvr_render_yuv left in the context's back buffer, over video rect ∩ window: the active
 * picture without the letterbox, as CTA-861.3 wants for the frame-average.  Queued on the context stream behind whatever the frame lanes
 * still write, and every later frame, lanes included, runs behind it; the histogram is complete after mpcvr_synchronize.  MPCVR_S_FALSE,
 * with nothing written, when no frame has been rendered yet (or the window changed since); an empty active area gives 1024 zeros and S_OK.
 * MPCVR_E_POINTER for a NULL hist_dev, MPCVR_E_INVALIDARG for one that is not 4-byte aligned or overlaps the back buffer. */
int32_t mpcvr_measure_backbuffer(mpcvr_ctx *ctx, uint32_t *hist_dev);
/* What a host derives from a histogram (HOST memory; no GPU, no context).  pixels = sum of hist; min_code / max_code = the smallest /
 * largest non-empty bin (-1 for an empty histogram, the nits are then 0); max_nits = L(max_code); avg_nits = (sum over c ascending of
 * hist[c] * L(c)) / pixels in double, with L(c) = 10000 * EOTF_ST2084(c / maxin) evaluated in double with the constants of
 * Shaders/convert/st2084.hlsl.  The codes mean something for every surface; the NITS only for a PQ surface (a context with
 * mpcvr_set_hdr_output enabled, whose frames are HDR10).  For a stream, MaxCLL = the maximum of max_nits over its frames and MaxFALL = the
 * maximum of avg_nits: the host keeps the two running maxima.  MPCVR_E_POINTER for a NULL pointer, MPCVR_E_INVALIDARG for another src_fmt. */
typedef struct mpcvr_light_level { uint64_t pixels; int32_t min_code, max_code; double max_nits, avg_nits; } mpcvr_light_level;
int32_t mpcvr_light_level_from_histogram(const uint32_t hist[MPCVR_HIST_BINS], int32_t src_fmt, mpcvr_light_level *out);
/* *code = the smallest c with hist[0] + ... + hist[c] >= ceil(ppm * pixels / 10^6), in 64-bit integers; ppm in 1 .. 1000000 (1000000: the
 * largest non-empty bin).  MPCVR_E_POINTER for a NULL pointer, MPCVR_E_INVALIDARG for ppm out of range or an empty histogram. */
int32_t mpcvr_histogram_percentile(const uint32_t hist[MPCVR_HIST_BINS], uint32_t ppm, int32_t *code);

/* EXTENSION — the rendered frame as the float tensor a model takes: fp32 / fp16 / bf16, C,H,W or H,W,C, RGB or BGR, value = code * scale
 * + bias per channel (1 / 255 and 0, or a dataset's mean / std folded in).  The reference has no float output; there is no reference line
 * to cite.  The definition is the text below, modelled bit for bit by tests/tensor_model.py (arithmetic: csrc/vp_tensor_core.h, which the
 * kernel and mpcvr_plan_tensor_value both compile).
 *   Input, as for mpcvr_encode_pass / mpcvr_measure_pass: a DEVICE surface of w x h 32-bit texels, src_fmt = MPCVR_OUT_BGRA8 (codes 0 ..
 *   255) or MPCVR_OUT_RGB10A2 (0 .. 1023), the A / X bits ignored; src and src_pitch multiples of 4, src_pitch >= 4 w; w and h in 1 ..
 *   32768, odd sizes allowed.  There is no rectangle: a caller crops by offsetting src.
 *   Arithmetic, per channel k = R, G, B of the picture (whatever the channel order), c = the channel's code, an integer:
 *       t = fp32(c) * scale[k], rounded to fp32;   v = t + bias[k], rounded to fp32
 *   — two IEEE round-to-nearest-even operations, NOT a fused multiply-add.  F32 stores v.  F16 stores v rounded to nearest even to binary16:
 *   overflow goes to +-inf, fp16 subnormals are kept.  BF16 stores (u + 0x7FFF + ((u >> 16) & 1)) >> 16 of v's bits u (nearest even).
 *   scale[k] and bias[k] must be finite, and 0 or of magnitude in [2^-100, 2^100]; otherwise MPCVR_E_INVALIDARG.  With that no fp32
 *   subnormal, infinity or NaN can arise: t is 0 or in [2^-100, 1023 * 2^100], and t + bias[k] is a sum of two multiples of 2^-123 below
 *   2^111, so it is 0 or at least 2^-123 — results do not depend on a flush-to-zero mode.
 *   Output: element size es = 4, 2, 2 bytes for F32, F16, BF16.  dst, row_pitch and (planar) plane_pitch are multiples of es — not of 4: a
 *   contiguous fp16 tensor of odd width is accepted.  Pitches are positive; row_pitch >= w es (planar) or 3 w es (interleaved).
 *   PLANAR: channel k of the tensor starts at dst + k plane_pitch, row y at + y row_pitch, column x at + x es.  INTERLEAVED: row y at
 *   dst + y row_pitch, pixel x holds its three elements at 3 x es.  channel_order says which of R, G, B is channel 0, 1, 2 of the tensor.
 *   No byte outside the elements is written: not the pitch padding, nothing in front of, between or behind planes.  Vector loads and
 *   stores are taken where pointers and pitches allow them (source on 16 bytes; tensor on 16 bytes for F32, 8 for F16 / BF16).
 * Refusals, with nothing launched and nothing written: MPCVR_E_POINTER for a NULL src, desc or dst; MPCVR_E_INVALIDARG for another src_fmt,
 * dtype, layout or channel_order, reserved != 0, w or h out of range, a pointer or pitch that breaks the rules above (a pitch beyond 2^47
 * bytes included), a scale or bias outside the set above, and a plane (first element to last element of its last row; for INTERLEAVED the
 * whole tensor is one plane) that overlaps another plane or the source. */
enum { MPCVR_TENSOR_F32 = 0, MPCVR_TENSOR_F16 = 1, MPCVR_TENSOR_BF16 = 2 };
enum { MPCVR_TENSOR_PLANAR = 0 /* C,H,W */, MPCVR_TENSOR_INTERLEAVED = 1 /* H,W,C */ };
enum { MPCVR_TENSOR_RGB = 0, MPCVR_TENSOR_BGR = 1 };      /* channel 0,1,2 of the tensor */
typedef struct mpcvr_tensor_desc {
    int32_t dtype, layout, channel_order, reserved;        /* reserved must be 0 */
    int64_t row_pitch;      /* bytes between rows */
    int64_t plane_pitch;    /* bytes between channel planes; PLANAR only, ignored otherwise */
    float   scale[3], bias[3];                             /* for R, G, B of the picture, whatever the channel order */
} mpcvr_tensor_desc;
/* Host, no GPU: *bits = the stored bits of one element (the low 16 for F16 / BF16) for a channel code of a src_fmt surface.
 * MPCVR_E_POINTER for a NULL bits; MPCVR_E_INVALIDARG for another dtype or src_fmt, a code beyond 255 / 1023, a scale or bias outside the
 * set above. */
int32_t mpcvr_plan_tensor_value(int32_t dtype, int32_t src_fmt, uint32_t code, float scale, float bias, uint32_t *bits);
/* One standalone pass over one device surface, like mpcvr_encode_pass; stream = a hipStream_t or NULL.  One kernel launch (k_tensor,
 * csrc/vp_tensor.hip). */
int32_t mpcvr_tensor_pass(const void *src, int32_t src_pitch, int32_t src_fmt, int32_t w, int32_t h, const mpcvr_tensor_desc *desc,
                          void *dst, void *stream);
/* mpcvr_render, then the pass over the whole window, ordered exactly as mpcvr_render_yuv: Process into the context-owned back buffer with
 * the letterbox cleared to black, on the context stream (not on a frame lane; the pixels are the same), the pass queued behind it, and
 * everything queued later, lanes included, behind the pass.  The tensor is complete after mpcvr_synchronize; mpcvr_get_backbuffer and
 * mpcvr_get_displayed_image afterwards see the RGB frame a plain mpcvr_render leaves.  The source format is the context's output_format
 * (bUseDither = 0 with MPCVR_OUT_RGB10A2 gives a model 10-bit codes without dither noise).  Everything mpcvr_tensor_pass refuses about
 * desc and dst is answered before anything is drawn.  S_FALSE, with nothing drawn or written, when there is no sample (as mpcvr_render). */
int32_t mpcvr_render_tensor(mpcvr_ctx *ctx, int32_t field, const mpcvr_tensor_desc *desc, void *dst);

/* EXTENSION — the way back: the float tensor a model leaves on the device (super-resolution, denoising, interpolation, generation) written
 * as a planar RGB sample, MPCVR_CF_GBRP8 / GBRP10 / GBRP16, which the convert path reads directly — the scalers, the ordered dither, the
 * error-diffusion pass and mpcvr_render_yuv then stand behind a float picture.  The reference has no float input; there is no reference
 * line to cite.  The definition is the text below, modelled bit for bit by tests/tensor_in_model.py (arithmetic: csrc/vp_tensor_core.h,
 * SampleCode, which the kernel and mpcvr_plan_sample_code both compile).
 *   The tensor is described by mpcvr_tensor_desc, unchanged: dtype, layout, channel_order, row_pitch and plane_pitch mean what they mean
 *   for mpcvr_tensor_pass, only that the tensor is READ; scale[k] and bias[k] (k = R, G, B of the picture, whatever the channel order) apply
 *   to the tensor's value.  w and h in 1 .. 32768, odd sizes allowed.  tensor, row_pitch and (planar) plane_pitch are multiples of the element
 *   size es; row_pitch >= w es (planar) or 3 w es (interleaved); pitches are positive and at most 2^47.
 *   Arithmetic, per channel, x = the element, maxcode = 255 / 1023 / 65535 for GBRP8 / GBRP10 / GBRP16:
 *     widening   x is widened exactly to fp32 (fp16 subnormals are kept: they are normal fp32 numbers; bf16 = bits << 16).  A widened value
 *                of magnitude below 2^-126 — an fp32 or bf16 subnormal, +0 or -0 — is taken as +0: the result does not depend on a
 *                denormal mode.
 *     two roundings   t = x * scale[k], rounded to fp32;  u = t + bias[k], rounded to fp32 — two IEEE round-to-nearest-even operations,
 *                NOT a fused multiply-add.  scale[k] and bias[k] must be finite, and 0 or of magnitude in [2^-100, 2^100], as for
 *                mpcvr_tensor_pass.  A subnormal t, kept or flushed to 0, cannot change the code: with bias[k] = 0, u = t and |t| < 2^-126
 *                < 0.5 gives code 0 either way; otherwise |bias[k]| >= 2^-100, where fp32 numbers are at least 2^-123 apart, and |t| <
 *                2^-126 is under half of that, so t + bias[k] rounds to bias[k] either way.  (A subnormal u is below 0.5: code 0.)
 *     code       0 if not (u > 0): NaN, -inf, negatives, inf * 0.  maxcode if u >= maxcode: +inf included.  Otherwise u rounded to the
 *                nearest integer, ties to even.
 *     stored     GBRP8 one byte; GBRP10 / GBRP16 a 16-bit word, for GBRP10 with bits 10 .. 15 zero.
 *   The sample is exactly what mpcvr_set_input(GBRP*, w, h, pitch) declares: planes G, B, R in that order, plane p at sample + p * pitch *
 *   h, row y at + y * pitch.  sample is a multiple of the component size (1 or 2); pitch >= w * component size, and even for the 16-bit
 *   formats.  channel_order says which of R, G, B tensor channel 0, 1, 2 is.  No byte outside the pixels is written: not the pitch
 *   padding, nothing in front of, between or behind planes.  All addressing is 64-bit: planes and rows may lie more than 4 GiB apart.
 *   Vector loads and stores are taken where pointers and pitches allow them (tensor on 16 bytes for F32, 8 for F16 / BF16; sample and
 *   pitch on 4 x the component size).
 * Refusals, with nothing launched and nothing written: MPCVR_E_POINTER for a NULL tensor, desc or sample; MPCVR_E_INVALIDARG for another
 * cformat, dtype, layout or channel_order, reserved != 0, a size, pointer or pitch outside the rules above, a scale or bias outside the
 * set, a plane of the tensor (first element to last element of its last row; INTERLEAVED: the whole tensor) that overlaps a plane of the
 * sample (first pixel to last pixel of its last row), and sample planes that overlap each other. */
/* Host, no GPU: *code = the code of one element (element_bits: the fp32 bits, or the 16 bits of F16 / BF16 in the low half) in a sample of
 * cformat.  MPCVR_E_POINTER for a NULL code; MPCVR_E_INVALIDARG for another dtype or cformat, element_bits beyond 16 bits for F16 / BF16,
 * a scale or bias outside the set above. */
int32_t mpcvr_plan_sample_code(int32_t dtype, int32_t cformat, uint32_t element_bits, float scale, float bias, uint32_t *code);
/* One standalone pass over one device tensor, like mpcvr_tensor_pass; stream = a hipStream_t or NULL.  One kernel launch
 * (k_sample_from_tensor, csrc/vp_tensor_in.hip). */
int32_t mpcvr_sample_pass(const void *tensor, const mpcvr_tensor_desc *desc, int32_t w, int32_t h, int32_t cformat, void *sample,
                          int32_t pitch, void *stream);
/* The tensor becomes the current sample of a context whose input (mpcvr_set_input) is GBRP8 / GBRP10 / GBRP16 of the tensor's width and
 * height, at the input's pitch; any other input answers MPCVR_E_INVALIDARG, MPCVR_E_NOT_VALID_STATE before mpcvr_set_input.  The call
 * takes an upload slot exactly as mpcvr_copy_sample(MPCVR_MEM_HOST) does — the slot ring, its device buffer, the event behind the
 * sample's last reader — with the pass in the place of the host-to-device copy, queued on the context stream: the caller's tensor must be
 * complete in that stream's order in front of the call and is free in that stream's order behind it.  The frame lanes, mpcvr_process,
 * mpcvr_render, mpcvr_render_yuv and mpcvr_render_tensor then work as for any host sample.  Everything mpcvr_sample_pass refuses about
 * tensor and desc is answered before anything is touched: the previous sample stays current. */
int32_t mpcvr_copy_sample_tensor(mpcvr_ctx *ctx, const void *tensor, const mpcvr_tensor_desc *desc);

/* EXTENSION — motion-adaptive deinterlacing of a sample at field rate: from the frames prev, cur, next one progressive frame per FIELD of
 * cur, which the convert path, the scalers, tone mapping and every batch call then take like any progressive sample.  The reference hands
 * bob and adaptive deinterlacing to the fixed-function D3D11 video processor (m_iVPDeinterlacing, m_bDeintDouble), which DESIGN.md §7 rules
 * out of scope, and its own shader path has only the blend (bDeintBlend, 4:2:0, frame rate): there is no reference line to cite.  The filter
 * is the well-known edge-directed spatial prediction held inside a temporal band (the Yadif scheme), spelled out here in integers so that no
 * outside code is needed and no bit is left open; it is modelled bit for bit by tests/deint_model.py (arithmetic: csrc/vp_deint_core.h,
 * DeintComponent, which the kernel and mpcvr_deint_plane_host both compile).
 *   Planes.  A sample is deinterlaced plane by plane.  A plane is `lines` rows of `comps` unsigned components of `bytes` (1 or 2) each; the
 *   horizontal neighbour step is cs: 1 for the Y, U, V, G, B, R and gray planes, 2 for the interleaved UV plane of the bi-planar formats
 *   (the neighbours of a U are U's).  Plane offsets and pitches are those of a sample as mpcvr_set_input declares it for (cformat, w, h,
 *   pitch), pitch = 0 meaning the default pitch as there (mpcvr_plan_deint_planes):
 *     bi-planar (NV12, P010, P016, P210, P216)   Y at 0: h lines of w components at pitch;  UV at pitch * h: h / div_h lines of w components
 *                                                (w / 2 pairs) at pitch, cs = 2
 *     three planes (YV12, YV16, YV24, YUV420P8 / 422P8 / 444P8, YUV420P10 / 16, YUV422P10 / 16, YUV444P10 / 16, GBRP8 / 10 / 16)
 *                                                plane 0 as Y above;  planes 1 and 2: h / div_h lines of w / div_w components at pitch / div_w
 *                                                (integer division), at pitch * h and at pitch * h + (pitch / div_w) * (h / div_h)
 *     gray (Y8, Y10, Y16)                        the one plane
 *   (div_w, div_h = 2, 2 for 4:2:0; 2, 1 for 4:2:2; 1, 1 otherwise.)  Every packed format — YUY2, UYVY, Y210, Y216, v210, AYUV, Y410, Y416
 *   and the interleaved RGB formats — is refused with MPCVR_E_INVALIDARG, and so is a sample one of whose planes has fewer than 2 lines.
 *   Components are whole 8- or 16-bit integers; mask = 0xff / 0xffff.  For the planar 10-bit formats (YUV4xxP10, GBRP10, Y10) a word is
 *   masked to bits 0 .. 9 on load (mask = 0x3ff): the library never reads bits 10 .. 15 there, and the output has them zero — in the kept
 *   lines too.  P010 and P210 use all 16 bits, as the library's reader does.
 *   Arguments.  keep (0 / 1) is the parity of the lines that belong to the field being shown: they are copied from cur.  first (0 / 1) says
 *   whether that field is the temporally first field of cur.  mode is MPCVR_DEINT_ADAPTIVE_EXT (with the spatial interlacing check) or
 *   MPCVR_DEINT_ADAPTIVE_NOCHECK_EXT.
 *   Per missing component — line y with (y & 1) != keep, column x — in signed 32-bit integers, >> an arithmetic shift:
 *     A, B       the frames holding the missing-parity field just before and just after the shown field: (prev, cur) if first, else (cur, next)
 *     ym, yp     y - 1 if y - 1 >= 0, else y + 1;   y + 1 if y + 1 < lines, else y - 1.   up = cur[ym], dn = cur[yp]
 *     columns    an index x + k cs is clamped into the component's own channel: to [x mod cs, comps - cs + (x mod cs)]
 *     c = up[x], e = dn[x], d = (A[y][x] + B[y][x]) >> 1
 *     t0 = |A[y][x] - B[y][x]|;  t1 = (|prev[ym][x] - c| + |prev[yp][x] - e|) >> 1;  t2 the same with next;  diff = max(t0 >> 1, t1, t2)
 *     score(j) = sum over k = -1, 0, 1 of |up[x + (k + j) cs] - dn[x + (k - j) cs]|;   pred(j) = (up[x + j cs] + dn[x - j cs]) >> 1
 *     best = score(0) - 1, sp = pred(0); then for s = -1 and after it s = +1: if score(s) < best { best = score(s), sp = pred(s); and only
 *                then, if score(2 s) < best { best = score(2 s), sp = pred(2 s) } }
 *     check      with mode 0, and only where y - 2 >= 0 and y + 2 < lines: b = (A[y-2][x] + B[y-2][x]) >> 1, f = (A[y+2][x] + B[y+2][x]) >> 1,
 *                mx = max(d - e, d - c, min(b - c, f - e)), mn = min(d - e, d - c, max(b - c, f - e)), diff = max(diff, mn, -mx)
 *     out = min(max(sp, d - diff), d + diff)
 *   diff >= 0 always, and out lies between sp and d: it stays in the component's range without a clamp.  With prev == cur == next and
 *   mode 1 the output is cur (d = the missing line itself, diff = 0); with mode 0 it is not, on pictures with vertical detail.
 *   The three sources are only read and may alias each other: a caller passes prev = cur at a stream's first frame and next = cur at its
 *   last.  No byte outside the destination's pixels is written; source bytes between a row's pixels and the pitch are never read into a
 *   pixel; all addressing is 64-bit.  Vector loads and stores are taken where pointers, plane offsets and pitches allow them (on 4 cs
 *   bytes-per-component bytes), chosen per launch.
 * Why this filter: it needs no motion vectors and no state beyond three frames, every tap is a neighbour in a plane (so it runs plane by
 * plane in the sample's own format, in front of the unchanged convert path), and its integer form leaves nothing to a float mode. */
enum { MPCVR_DEINT_ADAPTIVE_EXT = 0, MPCVR_DEINT_ADAPTIVE_NOCHECK_EXT = 1 };
typedef struct mpcvr_deint_plane { size_t offset; int32_t pitch, comps, lines, bytes, cs, mask; } mpcvr_deint_plane;
/* Host, no GPU: the planes of a sample, *planes of them (1 .. 3) in out[].  MPCVR_E_POINTER for a NULL planes or out; MPCVR_E_INVALIDARG
 * for exactly what the pass refuses about format, size and pitch (the rules of mpcvr_set_input; a plane of fewer than 2 lines). */
int32_t mpcvr_plan_deint_planes(int32_t cformat, int32_t w, int32_t h, int32_t pitch, int32_t *planes, mpcvr_deint_plane out[3]);
/* Host, no GPU: one plane in HOST memory, rows src_pitch / dst_pitch bytes apart, by the definition above — compiled from the per-component
 * function the kernel compiles.  dst must not overlap a source.  MPCVR_E_POINTER for a NULL pointer; MPCVR_E_INVALIDARG for bytes or cs
 * outside {1, 2}, comps no positive multiple of cs, lines < 2, a mask outside the component, keep, first or mode outside their sets,
 * a pitch below a row, or a pointer or pitch that is no multiple of bytes. */
int32_t mpcvr_deint_plane_host(const void *prev, const void *cur, const void *next, int64_t src_pitch, int32_t comps, int32_t lines,
                               int32_t bytes, int32_t cs, int32_t mask, int32_t keep, int32_t first, int32_t mode, void *dst, int64_t dst_pitch);
/* One standalone pass over three DEVICE samples of (cformat, w, h, pitch) into a fourth of (cformat, w, h, dst_pitch); pitch and dst_pitch
 * each obey mpcvr_set_input's pitch rules for the format (0: the default pitch).  stream = a hipStream_t or NULL.  One k_deint launch
 * (csrc/vp_deint.hip) per distinct (bytes, cs) among the planes: one for the three-plane and gray formats, two for the bi-planar ones.
 * Refusals, with nothing launched and nothing written: MPCVR_E_POINTER for a NULL pointer; MPCVR_E_INVALIDARG for a format, size or pitch
 * outside the rules, a sample that is no multiple of the component size, a keep, first or mode outside its set, and a destination plane
 * (first pixel to last pixel of its last row) that overlaps a plane of a source or another destination plane. */
int32_t mpcvr_deint_pass(const void *prev, const void *cur, const void *next, int32_t cformat, int32_t w, int32_t h, int32_t pitch,
                         int32_t keep, int32_t first, int32_t mode, void *dst, int32_t dst_pitch, void *stream);
/* Field `field` (0 the first, 1 the second) of cur, deinterlaced, becomes the current sample.  field_order is 1 for top field first, 2 for
 * bottom field first (the values of mpcvr_set_sample_format): first = (field == 0), keep = field for top field first, 1 - field for bottom
 * field first.  prev, cur, next are DEVICE samples of the context's input layout (mpcvr_set_input); the input must be a format the pass
 * takes.  The call takes an upload slot exactly as mpcvr_copy_sample_tensor does, with k_deint in the place of the copy, queued on the
 * context stream and recorded with the same events: frame lanes wait for it as for an upload, and the three samples are free in that
 * stream's order behind the call.  It neither reads nor changes the context's sample format: the sample now IS a progressive frame, so a
 * caller leaves mpcvr_set_sample_format at 0 (or bDeintBlend off).  Every refusal — MPCVR_E_NOT_VALID_STATE before mpcvr_set_input,
 * MPCVR_E_INVALIDARG for a field_order or field outside its set, and whatever mpcvr_deint_pass refuses — comes before anything is touched:
 * the previous sample stays current. */
int32_t mpcvr_copy_sample_fields(mpcvr_ctx *ctx, const void *prev, const void *cur, const void *next, int32_t field_order, int32_t field, int32_t mode);

/* EXTENSION — a 3D colour LUT applied to a rendered frame: the colour decision a broadcast or grading pipeline carries as a .cube file
 * (an HLG -> SDR or PQ -> SDR conversion, a camera log to Rec.709, a show look, a display or encoder calibration), tetrahedral
 * interpolation in integers.  The reference has no LUT; there is no reference line to cite.  The definition is the integer text below,
 * modelled bit for bit by tests/lut3d_model.py (arithmetic: csrc/vp_lut3d_core.h, which the kernel and mpcvr_plan_lut3d_value both compile).
 *   Surfaces: src is a DEVICE surface of w x h 32-bit texels, w and h in 1 .. 32768, src_fmt = MPCVR_OUT_BGRA8 (maxin = 255) or
 *     MPCVR_OUT_RGB10A2 (maxin = 1023); the A / X bits of src are ignored.  dst is w x h 32-bit texels, dst_fmt chosen independently of
 *     src_fmt from the same two formats, its largest code maxout; the A / X bits of dst are written as all ones.  Pointers and pitches are
 *     multiples of 4 and pitches >= 4 w (the render-target rule of mpcvr_process); 16-byte loads and stores are taken where pointers and
 *     pitches allow them.
 *   The table: lut is in DEVICE memory, 8-byte aligned: n^3 entries of four uint16_t {R, G, B, pad}, n in 2 .. 65.  The entry of node
 *     (r, g, b) sits at index (b n + g) n + r — R runs fastest, the order of a .cube file.  pad is ignored.  An entry component E in
 *     0 .. 65535 stands for E / 65535 of the destination's range.
 *   Per texel, everything in 32-bit unsigned integers.  For each source code c of (R, G, B):
 *       t = c (n - 1),   i = min(t / maxin, n - 2),   f = t - i maxin     (f lies in 0 .. maxin).
 *     Order the three channels so that f(1) >= f(2) >= f(3).  A tie needs no rule: it gives the vertex the two orders disagree about the
 *     weight zero, so either order gives the same answer (tests/test_lut3d.py evaluates tied inputs under every admissible order).
 *       V0 = lut[iR, iG, iB],   V1 = V0 stepped by +1 along the axis of f(1),   V2 = V1 stepped by +1 along the axis of f(2),
 *       V3 = lut[iR + 1, iG + 1, iB + 1];
 *       w0 = maxin - f(1),   w1 = f(1) - f(2),   w2 = f(2) - f(3),   w3 = f(3)     (they sum to maxin).
 *     For each output channel k:
 *       acc = sum over j of w_j V_j[k]     (at most 1023 * 65535 = 67,042,305),
 *       v = (acc + (maxin >> 1)) / maxin,   out = (v maxout + 32767) / 65535.
 *     Both divisions are by compile-time constants.  No dithering: an RGB10A2 source written as BGRA8 is rounded, as in mpcvr_encode_pass.
 *   With the identity table E[i] = (2 i 65535 + (n - 1)) / (2 (n - 1)) per axis, out == c whenever maxin == maxout, and across depths
 *     out == (2 c maxout + maxin) / (2 maxin), for every code and every n (tests/test_lut3d.py).
 *   In place: dst == src with dst_pitch == src_pitch is allowed; every texel is read before it is written, by the same lane.
 * Refusals, with nothing launched and nothing written: MPCVR_E_POINTER for a NULL src, lut_dev or dst; MPCVR_E_INVALIDARG for another
 * src_fmt or dst_fmt, n, w or h out of range, a pointer or pitch that breaks the rules above, any other overlap of dst with src, and any
 * overlap of the table with dst (a surface counts as the bytes from its first pixel to the last pixel of its last row).  No byte outside
 * dst's pixels is ever written: not the pitch padding, nothing in front of or behind the surface. */
/* Host, no GPU: n^3 float triplets in .cube order (R fastest) -> the 8-byte entries: each component rint(clamp(x, 0, 1) * 65535)
 * evaluated in double (ties to even), NaN -> 0, pad = 0.  MPCVR_E_POINTER for a NULL pointer, MPCVR_E_INVALIDARG for n outside 2 .. 65. */
int32_t mpcvr_plan_lut3d_entries(const float *rgb, int32_t n, uint16_t *entries);
/* Host, no GPU: *out = the destination texel of one source texel through a table in HOST memory, bit for bit what the kernel writes.
 * MPCVR_E_POINTER for a NULL pointer, MPCVR_E_INVALIDARG for another format or n. */
int32_t mpcvr_plan_lut3d_value(int32_t src_fmt, int32_t dst_fmt, const uint16_t *entries_host, int32_t n, uint32_t texel, uint32_t *out);
/* One standalone pass over one device surface, like mpcvr_encode_pass; stream = a hipStream_t or NULL.  One kernel launch (k_lut3d,
 * csrc/vp_lut3d.hip).  The table is read from LDS or from where it lies, by its size; the bytes are the same. */
int32_t mpcvr_lut3d_pass(const void *src, int32_t src_pitch, int32_t src_fmt, int32_t w, int32_t h, const void *lut_dev, int32_t n,
                         void *dst, int32_t dst_pitch, int32_t dst_fmt, void *stream);
/* mpcvr_render, then the pass from the back buffer over the whole window into dst, ordered exactly as mpcvr_render_tensor: Process into
 * the context-owned back buffer with the letterbox cleared to black, on the context stream (not on a frame lane; the pixels are the
 * same), the pass queued behind it, and everything queued later, lanes included, behind the pass.  dst is complete after
 * mpcvr_synchronize; the back buffer is only read: mpcvr_get_backbuffer and mpcvr_get_displayed_image afterwards see the RGB frame a plain
 * mpcvr_render leaves.  The source format is the context's output_format — MPCVR_OUT_RGB10A2 lets the table see 10-bit codes, with
 * dst_fmt free.  Everything mpcvr_lut3d_pass refuses about the table and dst is answered before anything is drawn.  S_FALSE, with nothing
 * drawn or written, when there is no sample (as mpcvr_render). */
int32_t mpcvr_render_lut3d(mpcvr_ctx *ctx, int32_t field, const void *lut_dev, int32_t n, void *dst, int32_t dst_pitch, int32_t dst_fmt);

/* EXTENSION — debanding of a rendered frame: hashed four-tap smoothing in integers, the step madVR and mpv users know as "deband".  An
 * 8-bit source with a sky or a fade upscaled 2x, or a PQ -> SDR tone map that stretches the shadows, leaves plateaus a few codes high and
 * tens of pixels wide, which the ordered dither and the error-diffusion pass quantise faithfully.  The pass replaces a texel by the mean of
 * four texels around it where that mean is close to it, and quantises last: render MPCVR_OUT_RGB10A2 with the dither off, deband, and let
 * the pass write 8 bits with its own dither.  The reference has no deband; there is no reference line to cite.  The definition is the
 * integer text below, modelled bit for bit by tests/deband_model.py (arithmetic: csrc/vp_deband_core.h, which the kernel and
 * mpcvr_deband_host both compile).
 *   Surfaces: src and dst are w x h 32-bit texels, w and h in 1 .. 32768, each MPCVR_OUT_BGRA8 (largest code 255) or MPCVR_OUT_RGB10A2
 *     (1023), chosen independently: maxin and maxout.  The A / X bits of src are ignored, those of dst written as all ones.  Pointers and
 *     pitches are multiples of 4 and pitches >= 4 w (the rules of mpcvr_lut3d_pass); 16-byte loads and stores are taken where pointers and
 *     pitches allow them.  NOT in place: the pass reads neighbours, so any overlap of dst with src is refused.
 *   Parameters (mpcvr_deband_params): range 1 .. 64, iterations 1 .. 4, range * iterations <= 64 — that product is the halo R, the farthest
 *     a tap lies from its texel in x and in y; threshold 0 .. 4 maxin in QUARTER codes of the source; dither 0 or 1.  A uint32_t seed is
 *     passed beside the struct.  mpcvr_deband_params_default: range 16, iterations 2, threshold 16 for RGB10A2 and 4 for BGRA8 (one 8-bit
 *     code either way), dither 1.
 *   The hash, in 32-bit unsigned wrap-around arithmetic:
 *       H(x, y, k, seed):  h = x + y 0x9E3779B1 + k 0x85EBCA77 + seed 0xC2B2AE3D;
 *                          h ^= h >> 16;  h *= 0x7feb352d;  h ^= h >> 15;  h *= 0x846ca68b;  h ^= h >> 16.
 *   Per texel (x, y), the same for the three channels unless said:
 *     1. cur = 4 c, c the channel's source code.
 *     2. For k = 1 .. iterations:  r = range k,  h = H(x, y, k, seed),
 *          dx = (((h & 0xffff) (2 r + 1)) >> 16) - r,   dy = (((h >> 16) (2 r + 1)) >> 16) - r      (each in -r .. r);
 *        the four taps are the SOURCE codes at (x + dx, y + dy), (x - dy, y + dx), (x - dx, y - dy), (x + dy, y - dx), each coordinate
 *        clamped to the surface; s = their sum, per channel; per channel: if |s - cur| k <= threshold then cur = s.
 *     3. den = 4 maxin;  d = den / 2 with dither 0,  d = ((H(x, y, 0, seed) >> 8) den) >> 24 with dither 1 (one value for the texel's three
 *        channels, 0 .. den - 1; this one product needs 34 bits and is NOT wrapped: it is the high word of (H & 0xffffff00) den);
 *        out = (cur maxout + d) / den, which never exceeds maxout; the division is by a compile-time constant.
 *   Consequences (tests/test_deband.py asserts them):
 *     - threshold == 0 and dither 0: out == c at equal depths, out == (2 c maxout + maxin) / (2 maxin) across depths — an iteration can
 *       only replace cur by an equal s;
 *     - a flat surface is returned unchanged for every threshold (s == cur everywhere), at equal depths with dither 0;
 *     - a surface of two levels A, B per channel with |A - B| > threshold is returned unchanged at equal depths with dither 0: a tap set
 *       that crosses the edge m times (m of its four taps lie on the other side) gives |s - cur| = m |A - B| (s and cur are both sums of
 *       four codes), so m = 0 leaves cur as it is and m >= 1 is refused for every k.
 * Refusals, with nothing launched and nothing written: MPCVR_E_POINTER for a NULL src, params or dst; MPCVR_E_INVALIDARG for another
 * src_fmt or dst_fmt, w or h out of range, a parameter outside the rules above, a pointer or pitch that breaks them, and any overlap of
 * dst with src (a surface counts as the bytes from its first pixel to the last pixel of its last row).  No byte outside dst's pixels is ever
 * written: not the pitch padding, nothing in front of or behind the surface. */
typedef struct mpcvr_deband_params {
    int32_t range;          /* 1 .. 64: iteration k takes its taps up to range * k texels away */
    int32_t iterations;     /* 1 .. 4, range * iterations <= 64 */
    int32_t threshold;      /* 0 .. 4 * maxin, quarter codes of the source */
    int32_t dither;         /* 0: round to nearest, 1: hashed dither on the output quantisation */
} mpcvr_deband_params;
/* Host, no GPU: the defaults for a source of src_fmt.  MPCVR_E_POINTER for NULL, MPCVR_E_INVALIDARG for another format. */
int32_t mpcvr_deband_params_default(int32_t src_fmt, mpcvr_deband_params *params);
/* Host, no GPU: the whole pass over surfaces in HOST memory, bit for bit what the kernel writes (the core needs neighbours, so it takes a
 * surface where mpcvr_plan_lut3d_value takes a texel).  The refusals of mpcvr_deband_pass. */
int32_t mpcvr_deband_host(const void *src_host, int64_t src_pitch, int32_t src_fmt, int32_t w, int32_t h, const mpcvr_deband_params *params,
                          uint32_t seed, void *dst_host, int64_t dst_pitch, int32_t dst_fmt);
/* Host, no GPU: *halo = R = range * iterations and *placement = where a launch over a w x h surface reads its taps from: 1 = a tile plus
 * halo staged in LDS, 0 = 4-byte loads from the surface (the environment variable MPCVR_DEBAND_TAPS = lds | global,
 * read per launch, overrides the rule where the placement is possible, and this call answers with it).  Each pointer optional.
 * MPCVR_E_POINTER for NULL params, MPCVR_E_INVALIDARG for what mpcvr_deband_pass refuses about the format, the parameters and the extent. */
int32_t mpcvr_plan_deband(int32_t src_fmt, const mpcvr_deband_params *params, int32_t w, int32_t h, int32_t *halo, int32_t *placement);
/* One standalone pass over one device surface, like mpcvr_lut3d_pass; stream = a hipStream_t or NULL.  One kernel launch (k_deband,
 * csrc/vp_deband.hip); the bytes do not depend on the placement. */
int32_t mpcvr_deband_pass(const void *src, int32_t src_pitch, int32_t src_fmt, int32_t w, int32_t h, const mpcvr_deband_params *params,
                          uint32_t seed, void *dst, int32_t dst_pitch, int32_t dst_fmt, void *stream);
/* mpcvr_render, then the pass from the back buffer over the whole window into dst, ordered exactly as mpcvr_render_lut3d: Process into the
 * context-owned back buffer with the letterbox cleared to black, on the context stream, the pass queued behind it, and everything queued
 * later, lanes included, behind the pass.  dst is complete after mpcvr_synchronize; the back buffer is only read.  The source format is the
 * context's output_format.  Everything mpcvr_deband_pass refuses is answered before anything is drawn.  S_FALSE, with nothing drawn or
 * written, when there is no sample (as mpcvr_render). */
int32_t mpcvr_render_deband(mpcvr_ctx *ctx, int32_t field, const mpcvr_deband_params *params, uint32_t seed, void *dst, int32_t dst_pitch, int32_t dst_fmt);

/* EXTENSION — sharpening of a rendered frame: a binomial unsharp mask in integers, with soft coring and an overshoot limiter; the step users
 * of the reference load into its post-scale shader slot (LumaSharpen, adaptive sharpen, CAS).  A 2x Lanczos or Jinc upscale leaves edges a
 * few texels wide; the pass adds the difference between the picture and its binomial blur back, leaves differences below a threshold alone
 * (noise is not detail) and keeps every channel within the range of its 3 x 3 neighbourhood plus an allowed overshoot (no halos).  The
 * reference has no sharpener; there is no reference line to cite.  The definition is the integer text below, modelled bit for bit by
 * tests/sharpen_model.py (arithmetic: csrc/vp_sharpen_core.h, which the kernel and mpcvr_sharpen_host both compile).
 *   Surfaces: the rules of mpcvr_deband_pass.  src and dst are w x h 32-bit texels, w and h in 1 .. 32768, each MPCVR_OUT_BGRA8 (largest
 *     code 255) or MPCVR_OUT_RGB10A2 (1023), chosen independently: maxin and maxout.  The A / X bits of src are ignored, those of dst
 *     written as all ones.  Pointers and pitches are multiples of 4 and pitches >= 4 w; 16-byte loads and stores are taken where pointers
 *     and pitches allow them.  NOT in place: any overlap of dst with src is refused.  Source bytes between a row's pixels and the pitch
 *     never reach a pixel.  All address arithmetic is 64-bit.
 *   Parameters (mpcvr_sharpen_params, a uint32_t seed beside it): radius r 1 .. 3; amount a 0 .. 256 in 1/64 (64 adds the detail once);
 *     threshold t 0 .. 4 maxin in QUARTER codes of the source (the coring); overshoot o 0 .. maxin in source codes; mode
 *     MPCVR_SHARPEN_RGB_EXT or MPCVR_SHARPEN_LUMA_EXT; dither 0 or 1.  mpcvr_sharpen_params_default: radius 2, amount 32, mode 1, dither 1,
 *     threshold 4 for BGRA8 and 16 for RGB10A2 (one 8-bit code), overshoot 2 for BGRA8 and 8 for RGB10A2 (two 8-bit codes).
 *   Per texel (x, y), every neighbour coordinate clamped to the surface, everything in signed 32-bit integers.  b_j = C(2 r, j + r) for
 *   j = -r .. r (1 2 1, 1 4 6 4 1, 1 6 15 20 15 6 1: sum 4^r per axis);  S = 16^r.
 *     1. The field f: mode 0, each channel's code, and steps 2 - 4 run per channel; mode 1, f = L = (54 R + 183 G + 19 B + 128) >> 8, one
 *        field for the texel, in 0 .. maxin (the weights sum to 256).
 *     2. Blur = sum_j sum_i b_j b_i f(x + i, y + j) <= S maxin;  d = S f(x, y) - Blur,  |d| <= S maxin <= 4,190,208.
 *     3. Soft coring: T = t (S / 4);  e = d - min(max(d, -T), T): zero inside +-T, continuous outside.
 *     4. Per channel c of the texel: v = 64 S c + a e (in mode 1 e is the luma's).  |a e| <= 1,072,693,248 and 64 S c <= 268,173,312, so
 *        |v| < 2^31.
 *     5. The limiter, per channel: mn and mx the least and greatest source code of that channel over the 3 x 3 neighbourhood (clamped
 *        coordinates, the centre included);  lo = max(mn - o, 0),  hi = min(mx + o, maxin);  v = min(max(v, 64 S lo), 64 S hi).
 *     6. Quarter codes: q = (v + 8 S) >> (4 r + 4), in 0 .. 4 maxin (v >= 0 here).
 *     7. The output stage is step 3 of the deband definition verbatim, and the same function: den = 4 maxin; dd = den / 2 with dither 0,
 *        dd = ((H(x, y, 0, seed) >> 8) den) >> 24 with dither 1 (the hash of mpcvr_deband_pass, one value for the texel's three channels,
 *        the 34-bit product taken as a high word); out = (q maxout + dd) / den.
 *   Consequences (tests/test_sharpen.py asserts them; the first five at equal depths with dither 0 — across depths "unchanged" reads
 *   out = (2 c maxout + maxin) / (2 maxin)):
 *     - a = 0 returns the code; t = 4 maxin returns the code (|d| never exceeds T);
 *     - a flat surface comes back unchanged for every parameter set;
 *     - a surface of two levels A <= B per channel (every channel at its A on the same texels) comes back unchanged at o = 0 for every a, r
 *       and mode, whatever the edge's shape: where the 3 x 3 neighbourhood holds one level, lo = hi; where it holds both, the code is A or
 *       B and the detail points away from the other level (in mode 1 because L rises with every channel; with a channel that runs the
 *       other way it would not); with overshoot o every output lies in A - o .. B + o;
 *     - a gray surface (R = G = B) whose code is affine in x and y comes back unchanged wherever no tap clamps, r texels in from every
 *       border: the binomial weights are symmetric, so Blur = S f;
 *     - on a gray surface mode 0 and mode 1 give identical texels, dither included (L of a gray texel is its code);
 *     - at o = 0 every output channel lies within the least and greatest code of its own 3 x 3 source neighbourhood.
 *   What it does to an edge (the model, tests/test_sharpen.py): a 10-bit row stepping 100 -> 900, blurred by the 9-tap binomial (C(8, j),
 *   sum 256, floor division), has 4 texels strictly between 180 and 820 (its 10 - 90 % width); at radius 2, amount 64, threshold 0 the pass
 *   leaves 2.  With o = 0 no code is below 100 or above 900; with o = 16 the extremes are 91 and 908.
 * Refusals, with nothing launched and nothing written: MPCVR_E_POINTER for a NULL src, params or dst; MPCVR_E_INVALIDARG for another
 * src_fmt or dst_fmt, w or h out of range, a parameter outside the rules above, a pointer or pitch that breaks them, and any overlap of
 * dst with src (a surface counts as the bytes from its first pixel to the last pixel of its last row).  No byte outside dst's pixels is ever
 * written: not the pitch padding, nothing in front of or behind the surface. */
#define MPCVR_SHARPEN_RGB_EXT 0
#define MPCVR_SHARPEN_LUMA_EXT 1
typedef struct mpcvr_sharpen_params {
    int32_t radius;         /* 1 .. 3: the blur is the (2 r + 1)-tap binomial in x and in y */
    int32_t amount;         /* 0 .. 256, in 1/64: 64 adds the detail once */
    int32_t threshold;      /* 0 .. 4 * maxin, quarter codes of the source: detail below it is left alone */
    int32_t overshoot;      /* 0 .. maxin, source codes: how far a channel may leave the range of its 3 x 3 neighbourhood */
    int32_t mode;           /* MPCVR_SHARPEN_RGB_EXT: per channel, MPCVR_SHARPEN_LUMA_EXT: the luma's detail added to every channel */
    int32_t dither;         /* 0: round to nearest, 1: hashed dither on the output quantisation */
} mpcvr_sharpen_params;
/* Host, no GPU: the defaults for a source of src_fmt.  MPCVR_E_POINTER for NULL, MPCVR_E_INVALIDARG for another format. */
int32_t mpcvr_sharpen_params_default(int32_t src_fmt, mpcvr_sharpen_params *params);
/* Host, no GPU: the whole pass over surfaces in HOST memory, bit for bit what the kernel writes.  The refusals of mpcvr_sharpen_pass. */
int32_t mpcvr_sharpen_host(const void *src_host, int64_t src_pitch, int32_t src_fmt, int32_t w, int32_t h, const mpcvr_sharpen_params *params,
                           uint32_t seed, void *dst_host, int64_t dst_pitch, int32_t dst_fmt);
/* Host, no GPU: what a launch over a w x h surface decides by rule.  *halo = r, the texels a workgroup stages around its tile on every
 * side; *lds_bytes = the LDS of one workgroup (the staged image and the row sums: DESIGN.md section 4.15), which depends on r and the mode.
 * Each pointer optional.  MPCVR_E_POINTER for NULL params, MPCVR_E_INVALIDARG for what mpcvr_sharpen_pass refuses about the format, the
 * parameters and the extent. */
int32_t mpcvr_plan_sharpen(int32_t src_fmt, const mpcvr_sharpen_params *params, int32_t w, int32_t h, int32_t *halo, int32_t *lds_bytes);
/* One standalone pass over one device surface, like mpcvr_deband_pass; stream = a hipStream_t or NULL.  One kernel launch (k_sharpen,
 * csrc/vp_sharpen.hip).  The environment variable MPCVR_SHARPEN_STAGING = dword, read per launch, makes the kernel stage its tile with
 * 4-byte loads where it would take 16-byte ones (A/B runs); the bytes written do not depend on it. */
int32_t mpcvr_sharpen_pass(const void *src, int32_t src_pitch, int32_t src_fmt, int32_t w, int32_t h, const mpcvr_sharpen_params *params,
                           uint32_t seed, void *dst, int32_t dst_pitch, int32_t dst_fmt, void *stream);
/* mpcvr_render, then the pass from the back buffer over the whole window into dst, ordered exactly as mpcvr_render_deband: Process into the
 * context-owned back buffer with the letterbox cleared to black, on the context stream, the pass queued behind it, and everything queued
 * later, lanes included, behind the pass.  dst is complete after mpcvr_synchronize; the back buffer is only read.  The source format is the
 * context's output_format.  Everything mpcvr_sharpen_pass refuses is answered before anything is drawn.  S_FALSE, with nothing drawn or
 * written, when there is no sample (as mpcvr_render). */
int32_t mpcvr_render_sharpen(mpcvr_ctx *ctx, int32_t field, const mpcvr_sharpen_params *params, uint32_t seed, void *dst, int32_t dst_pitch, int32_t dst_fmt);

/* Configure — DX11VideoProcessor.cpp:3800-4050: diff each field, rebuild only what changed. */
int32_t mpcvr_configure(mpcvr_ctx *ctx, const mpcvr_settings *settings);

/* SetProcAmpValues — DX11VideoProcessor.cpp:4506-4537; ranges Helper.cpp:182-187
 * (brightness -100..100, contrast 0..2, hue -180..180, saturation 0..2). */
int32_t mpcvr_set_procamp(mpcvr_ctx *ctx, uint32_t flags, float brightness, float contrast,
                          float hue, float saturation);

/* CopySample / MemCopyToTexSrcVideo — DX11VideoProcessor.cpp:2202,1213-1252.
 * data: one media sample (planes back to back); pitch: the row pitch given to mpcvr_set_input (negative for a bottom-up
 * RGB DIB, whose `data` still points at the lowest address, DX11VideoProcessor.cpp:1243-1248).
 * MPCVR_MEM_HOST: copied into one of three pinned staging buffers and uploaded on a copy stream, so the upload of
 * sample n+1 overlaps the processing of sample n (CopyPlane10to16's <<6 / CopyFrameV210 / CopyFrameRGB* run on the
 * device); the caller's buffer is free again when the call returns.  MPCVR_MEM_HOST_PINNED: the buffer is page-locked
 * (hipHostMalloc / hipHostRegister) and is DMA'd from directly; it must stay untouched until mpcvr_synchronize has
 * returned, or until the third following copy_sample OF A HOST SAMPLE (MPCVR_MEM_HOST or MPCVR_MEM_HOST_PINNED: that one
 * takes this sample's upload slot and waits for it; an MPCVR_MEM_DEVICE sample takes no slot and does not count) has
 * returned.  A sample that is never drawn is uploaded all the same, and the same rule holds for its buffer.  A page-locked
 * buffer handed over as MPCVR_MEM_HOST is staged like any other.  A host sample may be drawn any number of times (several
 * targets, mpcvr_render, the snapshot): its slot is reused behind all of them.
 * MPCVR_MEM_DEVICE: zero-copy — the pointer is used in place and must stay valid until
 * the following process/render call has completed (mirrors the IMediaSampleD3D11 branch :2528-2569).
 * Which bits of a sample are read (the same on every route, tier and mem_kind; tests/test_sample_bits*.py):
 *   8- and 16-bit components (NV12, YV12 .. YUV444P16, P016 / P216, Y216, Y416, GBRP8 / 16, Y8 / Y16, RGB24 / 48, BGR48): every bit;
 *   P010, P210, Y210: all 16 bits of a word, the six under the 10-bit code included (the reference's texture is 16-bit UNORM);
 *   YUV420P10 / 422P10 / 444P10, GBRP10, Y10: bits 0..9 of a word — bits 10..15 are dropped, a word of 1024 + k reads as k
 *     (CopyPlane10to16 stores word << 6 into 16 bits, Helper.cpp:789-803);
 *   Y410, r210, v210: the three 10-bit fields of a dword; Y410's alpha bits, r210's two pad bits, bits 30..31 of a v210 dword and the
 *     v210 fields past the width in a row's last six-pixel group are ignored;
 *   AYUV, Y416, XRGB32 / ARGB32, BGRA64, b64a: the three colour components; the A / X component is ignored.
 *   Bytes between a row's pixels and the pitch are never read into a pixel.
 * Refusals — a NULL data: MPCVR_E_POINTER; a pitch that is not the media type's: MPCVR_E_UNEXPECTED (:2545); a mem_kind
 * that is none of the three: MPCVR_E_INVALIDARG — are answered before anything is touched: the sample handed over
 * before stays current and the next mpcvr_process draws it.  After mpcvr_flush there is no current sample
 * (mpcvr_process: MPCVR_E_NOT_VALID_STATE) until the next copy_sample. */
int32_t mpcvr_copy_sample(mpcvr_ctx *ctx, const void *data, int32_t pitch, int32_t mem_kind);

/* Process — DX11VideoProcessor.cpp:3285-3424.  dst: DEVICE pointer to a window_w x window_h render
 * target, 4 bytes per pixel (B8G8R8A8 or R10G10B10A2), dst_pitch bytes per row.  src_rect must be
 * NULL or the input's source rect (the reference overrides it with the convert texture, :3316-3319);
 * dst_rect NULL => the context's video rect.  Pixels outside dst_rect are not written, and neither is any byte outside the
 * window's pixels: the bytes between window_w * 4 and dst_pitch of a row, and everything in front of and behind the target.
 * A render target is made of dwords: dst_dev and dst_pitch must be multiples of 4 (any multiple: a sub-allocated, pitch-padded
 * surface is served; the 8- and 16-byte stores are taken where target and pitch allow them).  MPCVR_E_INVALIDARG otherwise, with
 * nothing launched and the target untouched.  Any such dst_pitch up to INT32_MAX is rendered correctly, with the same pixels: the fused
 * kernels address target rows with 32-bit offsets and step aside, per call, where dst_pitch * (max(dst_rect top, 0) + dst_rect height)
 * reaches 4 GiB — the convert kernel and the resize draws then write the frame, in stream order (such a frame takes no lane), and
 * mpcvr_get_path_info, read after the call, names what ran.  The same holds for every dsts[i] / dst_pitch of mpcvr_process_frames,
 * mpcvr_process_batch and mpcvr_process_batch_dovi (the targets of a batch may lie any distance apart).
 * Exact 2x: the kernels that filter with the weights of the NOMINAL phases (the exact-2x kernel, the fused Jinc2m kernel, the Jinc2m phase
 * tables) are planned only where, on either axis, sum_k |w_real - w_nominal| x the target's quantisation (255 / 1023) is at most 0.5 codes
 * (w_real: the weights at the reference's fp32 texture coordinate); above that the any-ratio kernel / the per-pixel Jinc2m kernel draw the
 * frame with the real weights.  Lanczos3: 3840 -> 7680 is 0.08 codes of 8 bits and 0.31 of 10, a 15360- or 16380-wide source 0.31 and 1.25,
 * a power of two 0 (measured worst case per side of the threshold: DESIGN.md section 4.2). */
int32_t mpcvr_process(mpcvr_ctx *ctx, void *dst_dev, int32_t dst_pitch, const mpcvr_rect *src_rect,
                      const mpcvr_rect *dst_rect, int32_t second_field);

/* n frames the reference's way — mpcvr_copy_sample(samples[i], pitch, mem_kind) then mpcvr_process(dsts_dev[i], dst_pitch, NULL, NULL, 0), frame
 * after frame (ProcessSample -> CopySample -> Render -> Process, DX11VideoProcessor.cpp:2143-2200, :2730) — behind one call, so that a caller
 * in a scripting language measures the path and not its own foreign-function calls.  Not a batch: every frame is its own launch (or lands
 * on the context's frame lanes); stops at the first failure and returns it (a dsts_dev[i] or dst_pitch that is not a multiple of 4:
 * MPCVR_E_INVALIDARG at that frame, the frames in front of it drawn). */
int32_t mpcvr_process_frames(mpcvr_ctx *ctx, int32_t n, const void *const *samples, int32_t pitch, int32_t mem_kind, void *const *dsts_dev, int32_t dst_pitch);

/* Render minus Present — DX11VideoProcessor.cpp:2599-2813: Process into the context-owned back buffer. */
int32_t mpcvr_render(mpcvr_ctx *ctx, int32_t field);
/* Device pointer / pitch of the context-owned back buffer written by mpcvr_render. */
int32_t mpcvr_get_backbuffer(mpcvr_ctx *ctx, void **dev_ptr, int32_t *pitch, int32_t *width, int32_t *height);

/* GetCurentImage — DX11VideoProcessor.cpp:3493-3608: source-rect-sized BGRX snapshot into host memory.
 * Two-call size protocol (VideoRenderer.cpp:979-988): host_bgra == NULL => *size receives the bytes
 * needed (rect_w*rect_h*4); otherwise *size must be >= that.  Synchronous. */
int32_t mpcvr_get_current_image(mpcvr_ctx *ctx, void *host_bgra, size_t *size);
/* GetDisplayedImage — DX11VideoProcessor.cpp:3610-3683: the back buffer of the last mpcvr_render as it is (nothing is drawn again), as
 * the pixels of a top-down DIB in host memory: a B8G8R8A8 buffer as it is; an R10G10B10A2 one as BGR32 (the top eight bits of each channel,
 * ConvertR10G10B10A2toBGR32, Helper.cpp:805) or, with deep_color != 0 (m_bAllowDeepColorBitmaps), as BGR48 (ConvertR10G10B10A2toBGR48, :836).
 * Rows are ((width * bits + 31) & ~31) / 8 bytes apart (CalcDibRowPitch).  The BITMAPINFOHEADER and the LocalAlloc block around the pixels
 * are the caller's: host_pixels == NULL => *size, *width, *height and *bits_per_pixel are reported (any of the last three may be NULL);
 * otherwise *size must be >= the size reported.  MPCVR_E_NOT_VALID_STATE before the first mpcvr_render.  Synchronous. */
int32_t mpcvr_get_displayed_image(mpcvr_ctx *ctx, void *host_pixels, size_t *size, int32_t deep_color, int32_t *width, int32_t *height, int32_t *bits_per_pixel);

/* Flush (DX11VideoProcessor.cpp:4074) / Reset (:3453). */
int32_t mpcvr_flush(mpcvr_ctx *ctx);
int32_t mpcvr_reset(mpcvr_ctx *ctx);

/* Extension (not in the reference): n frames in one launch sequence to escape the launch-bound
 * regime.  srcs[i]: DEVICE sample pointers (layout/pitch as declared by mpcvr_set_input);
 * dsts[i]: DEVICE render targets (dst_pitch each; every dsts[i] and dst_pitch a multiple of 4, else MPCVR_E_INVALIDARG and nothing is
 * drawn — see mpcvr_process.  The targets of one batch may differ in alignment: every frame runs through the stores the worst-aligned allows).
 * The frames of a batch are independent of each other: on every path that can, the whole batch runs as one launch per
 * draw (fused 2x / strip / periodic kernel: one launch; same-size frames: one k_convert_stream launch; pass-per-kernel path:
 * block convert / X draw / Y draw with a frame dimension and batched intermediates, <= 4 GiB; Dolby Vision: the block convert's
 * frame dimension, one RPU per call here, one per frame in mpcvr_process_batch_dovi; the HDR10 tone-mapping step: one launch behind
 * batched post-scale textures; quarter turns, flips outside the strip kernels' reach and Jinc2m in its one- and two-draw forms: every
 * draw kernel has a frame dimension; bUseDither = 2: ONE error-diffusion launch behind the batch's 10-bit frames), otherwise frame by
 * frame (samples that do not start on a dword or need a repack of their own outside the v210 / interleaved-RGB batch textures).
 * mpcvr_get_last_batch_info reports the kernel launches a batch took.  The targets of one batch must therefore not overlap in memory; completion is
 * in stream order for the batch as a whole.
 * Round 6: on a context that OWNS its stream (no mpcvr_set_stream) consecutive batches whose plan is one launch with no intermediate
 * surface (exact 2x, the strip / periodic kernel reading the samples, the fused Jinc2m kernel, the same-size block convert; no Dolby Vision,
 * no repack) take turns on two internal lanes, so that two launches are in flight and fill each other's ramp-up and tail (4K -> 8K: +4 %,
 * 1080p -> 1440p: +16 %; MPCVR_NO_BATCH_LANES=1 in the environment turns it off).
 * Batches and single frames that write overlapping memory stay in the order they were queued, whatever pointers they were given: a target
 * counts as the bytes from its first pixel to the last pixel of its last row, dst_dev .. dst_dev + (window_h - 1) * dst_pitch + window_w * 4
 * (a window further down in one surface, the same surface from another base; rows of two targets that interleave in one surface count as
 * overlapping).  Targets that merely touch run side by side.  Everything that can observe
 * a result (mpcvr_synchronize, the snapshot, a plan change, mpcvr_set_stream) waits for the lanes.  MPCVR_FLAG_NO_FRAME_LANES (or a caller's
 * stream) keeps every batch in stream order; mpcvr_get_last_batch_info names the lane ("lane=0|1", -1 = the context stream) and how many
 * writers still in flight on other lanes the batch was ordered behind ("waits=<n>"). */
int32_t mpcvr_process_batch(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, void *const *dsts,
                            int32_t dst_pitch);
/* mpcvr_process_batch for a Dolby Vision stream: rpus[i] is the RPU of frame i — the reference reads it from every sample in
 * CopySample (IID_MediaSideDataDOVIMetadataV2, DX11VideoProcessor.cpp:2270-2520).  The result is what n rounds of
 * mpcvr_set_dovi_metadata(&rpus[i]) + mpcvr_process(srcs[i] -> dsts[i]) produce, level-1 / level-2 blocks staying as last seen
 * like there, and the context ends up holding the last frame's RPU.  Frames are cut into runs that share a plan and a kernel variant
 * (level-2 trims for this display present or not); a run is ONE launch per stage where the block convert's Dolby Vision variants
 * run (same-size frames; convert + resize kernels): they read frame z's curves, LMS matrix, trims and ycc_to_rgb matrix from
 * device tables indexed by the frame.  A run behind the HDR10 tone-mapping step (its level-1 constants travel by value), and
 * whatever the per-pixel convert serves, goes frame by frame with each RPU's constants uploaded in stream order.
 * E_INVALIDARG, and nothing drawn, when any RPU of the batch fails the checks of mpcvr_set_dovi_metadata, or when a dsts[i] or
 * dst_pitch is not a multiple of 4 (see mpcvr_process). */
int32_t mpcvr_process_batch_dovi(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, void *const *dsts,
                                 int32_t dst_pitch, const mpcvr_dovi_metadata *rpus);

/* EXTENSION — a batch written as NV12 / P010 (mpcvr_process_batch for a transcoder; the pass itself: mpcvr_encode_pass above).
 * The planes of frame i hold, byte for byte, what
 *     mpcvr_process_batch(srcs -> n window-sized RGB targets of the context's output_format, black outside the video rect), then
 *     mpcvr_encode_pass(target i, output_format, window_w, window_h, out_cformat, extfmt, y_planes[i], y_pitch, uv_planes[i], uv_pitch)
 * leave — without the host owning the RGB memory, and with ONE k_encode420 launch per chunk of frames (its frame dimension) where the
 * composition takes n.  The RGB frames live in a context-owned surface laid out by mpcvr_plan_batch_yuv:
 *     surface_pitch    = (4 window_w + 15) & ~15          (every lane of the pass with four columns takes its 16-byte load)
 *     frame_stride     = surface_pitch * window_h rounded up to 256
 *     frames_per_chunk = clamp(budget_bytes / frame_stride, 1, n),      chunks = ceil(n / frames_per_chunk)
 * budget_bytes = 0 means the default, MPCVR_BATCH_YUV_DEFAULT_BUDGET (4 GiB: what a sweep over 256 MiB, 1 GiB and 4 GiB favours — 32 frames
 * of 8K in one chunk run 6-7 % ahead of four chunks and 23-24 % ahead of sixteen; profiles/r13/batch_yuv.txt).  mpcvr_plan_batch_yuv needs no GPU; any out pointer may be NULL;
 * MPCVR_E_INVALIDARG for n <= 0 or a window width / height that is odd or outside 2 .. 32768.
 * mpcvr_set_batch_yuv_budget: the bytes one such surface may take (0 = the default again; the library's other batched
 * intermediates stop at 4 GiB, and nothing above that was measured).  A context that owns its stream keeps one surface per batch lane it uses.
 * Each chunk runs what mpcvr_process_batch runs for its frames (every route, bUseDither = 2 included; a context holding one Dolby Vision
 * RPU works as there, one RPU per frame is not offered) into the surface, then the pass, on the same stream.  The letterbox is black as in
 * mpcvr_render_yuv: the surface is cleared when it is allocated and when the window or the video rect changes, not per call.
 * Order: on a caller's stream (mpcvr_set_stream), with MPCVR_FLAG_NO_FRAME_LANES or MPCVR_NO_BATCH_LANES=1, and for chunks whose route
 * is no lane route, everything runs in stream order on the context stream.  On a context that owns its stream the chunks whose route
 * mpcvr_process_batch would put on a lane take turns on the two batch lanes, across the chunks of a call and across calls, each lane with
 * a surface of its own: the render of one chunk runs beside the pass of the one before.  The planes count as the bytes written (first
 * pixel to the last pixel of the last row, as for render targets): single frames, RGB batches and further calls that write memory a plane
 * in flight covers stay behind it in the order they were queued.  The lanes order WRITES, not readers: the planes are complete after
 * mpcvr_synchronize, and a caller that feeds them back as samples synchronises first.
 * Refusals, answered before anything is drawn, allocated or written: MPCVR_E_NOT_VALID_STATE before mpcvr_set_input; MPCVR_E_POINTER for
 * a NULL array or entry; MPCVR_E_INVALIDARG for n <= 0, an odd window width or height, whatever mpcvr_encode_pass refuses about formats,
 * description, pitches and pointers, and any two planes of the batch (2 n of them) that overlap each other.
 * mpcvr_get_last_batch_info afterwards: "launches" counts the passes too, and ";yuv_chunks=<k>;yuv_lanes=<lane,lane,...>" follow (the lane
 * of each chunk, -1 = the context stream; the first 64 chunks). */
#define MPCVR_BATCH_YUV_DEFAULT_BUDGET ((size_t)4 << 30)
int32_t mpcvr_plan_batch_yuv(int32_t window_w, int32_t window_h, int32_t n, size_t budget_bytes,
                             int32_t *surface_pitch, size_t *frame_stride, int32_t *frames_per_chunk, int32_t *chunks);
int32_t mpcvr_set_batch_yuv_budget(mpcvr_ctx *ctx, size_t bytes);
int32_t mpcvr_process_batch_yuv(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, int32_t out_cformat, uint32_t extfmt,
                                void *const *y_planes, int32_t y_pitch, void *const *uv_planes, int32_t uv_pitch);
/* EXTENSION — mpcvr_process_batch_yuv plus the histograms of mpcvr_measure_pass: hist_dev holds n rows of MPCVR_HIST_BINS words in DEVICE
 * memory, frame i at hist_dev + 1024 i.  Row i is what mpcvr_measure_pass over video rect ∩ window gives on the RGB target i that
 * mpcvr_process_batch leaves (an empty active area: zeros); the planes are byte for byte those of mpcvr_process_batch_yuv.  Per chunk ONE
 * measure launch with a frame dimension reads the chunk's frames in the context-owned surface, on the chunk's stream behind its k_encode420
 * launch: "launches" of mpcvr_get_last_batch_info grows by exactly one per chunk.  The rows of a chunk are bytes it writes for the caller:
 * the lanes order on them as on the planes, so two calls into one histogram buffer stay in the order they were queued.  The rows are
 * complete after mpcvr_synchronize.  Refusals beyond those of mpcvr_process_batch_yuv, before anything is drawn: MPCVR_E_POINTER for a NULL
 * hist_dev; MPCVR_E_INVALIDARG for one that is not 4-byte aligned or whose n rows overlap a plane of the batch. */
int32_t mpcvr_process_batch_yuv_stats(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, int32_t out_cformat, uint32_t extfmt,
                                      void *const *y_planes, int32_t y_pitch, void *const *uv_planes, int32_t uv_pitch,
                                      uint32_t *hist_dev /* n rows of 1024 words, frame i at hist_dev + 1024 i */);
/* EXTENSION — a batch written as float tensors (mpcvr_process_batch for a model; the pass itself: mpcvr_tensor_pass above).  dsts[i] is
 * the tensor of frame i, all n described by one desc.  Frame i holds, byte for byte, what
 *     mpcvr_process_batch(srcs -> n window-sized RGB targets of the context's output_format, black outside the video rect), then
 *     mpcvr_tensor_pass(target i, output_format, window_w, window_h, desc, dsts[i])
 * leave, with ONE k_tensor launch per chunk of frames (its frame dimension) where the composition takes n.  The machinery is that of
 * mpcvr_process_batch_yuv: the RGB frames live in the same context-owned surfaces (one per batch lane used), laid out by
 * mpcvr_plan_batch_tensor — the three formulas of mpcvr_plan_batch_yuv without the evenness condition (window width and height 1 .. 32768,
 * otherwise MPCVR_E_INVALIDARG) — under the same budget: mpcvr_set_batch_yuv_budget serves both calls.  Chunks, routes, the letterbox and
 * the order are as described there: the chunks of lane routes take turns on the two batch lanes, each with the lane's surface, everything
 * else runs on the context stream.  Every plane of every frame (three per PLANAR frame, one per INTERLEAVED frame) counts as bytes the
 * chunk writes: single frames, batches and further calls that write memory a plane in flight covers stay behind it in queue order.  The
 * tensors are complete after mpcvr_synchronize.
 * Refusals, answered before anything is drawn, allocated or written: MPCVR_E_NOT_VALID_STATE before mpcvr_set_input; MPCVR_E_POINTER for
 * a NULL array, entry or desc; MPCVR_E_INVALIDARG for n <= 0, whatever mpcvr_tensor_pass refuses about desc and a dsts[i], and any two
 * planes of the batch that overlap each other.
 * mpcvr_get_last_batch_info afterwards: "launches" counts one pass per chunk, and ";tensor_chunks=<k>;tensor_lanes=<lane,lane,...>"
 * follow (the lane of each chunk, -1 = the context stream; the first 64 chunks). */
int32_t mpcvr_plan_batch_tensor(int32_t window_w, int32_t window_h, int32_t n, size_t budget_bytes,
                                int32_t *surface_pitch, size_t *frame_stride, int32_t *frames_per_chunk, int32_t *chunks);
int32_t mpcvr_process_batch_tensor(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, const mpcvr_tensor_desc *desc, void *const *dsts);
/* EXTENSION — a batch FROM float tensors (the pass itself: mpcvr_sample_pass above).  The input is GBRP8 / GBRP10 / GBRP16; tensors[i] is
 * the tensor of frame i, all n described by one desc, dsts[i] its render target.  Target i holds, byte for byte, what
 *     mpcvr_sample_pass(tensors[i], desc, w, h, cformat, sample i of the caller's, pitch), n times, then
 *     mpcvr_process_batch(samples -> dsts, dst_pitch)
 * leave, with ONE k_sample_from_tensor launch per chunk of frames (its frame dimension) where the composition takes n, and no samples of
 * the caller's: they live in a context-owned surface, frame i of a chunk at i * frame_stride, frame_stride = 3 * pitch * h rounded up
 * to 256 (mpcvr_plan_batch_from_tensors; pitch and h are the input's).  A chunk is what fits the budget of mpcvr_set_batch_yuv_budget
 * (0: the default), at least one frame, at most n — the library's one chunk rule.  Every chunk runs in stream order on the context
 * stream: the pass, then the chunk's mpcvr_process_batch work, so the surface's reuse by the next chunk and the next call is ordered;
 * the batch lanes are not used.  The tensors are free in stream order behind the call; the targets are complete after mpcvr_synchronize.
 * Refusals, answered before anything is drawn, allocated or written: MPCVR_E_NOT_VALID_STATE before mpcvr_set_input; MPCVR_E_POINTER for
 * a NULL array, entry or desc; MPCVR_E_INVALIDARG for n <= 0, another input format, whatever mpcvr_sample_pass refuses about desc and a
 * tensors[i], and whatever mpcvr_process_batch refuses about dsts and dst_pitch.
 * mpcvr_get_last_batch_info afterwards: "launches" counts one pass per chunk, and ";sample_chunks=<k>" follows. */
int32_t mpcvr_plan_batch_from_tensors(int32_t pitch, int32_t h, int32_t n, size_t budget_bytes,
                                      size_t *frame_stride, int32_t *frames_per_chunk, int32_t *chunks);
int32_t mpcvr_process_batch_from_tensors(mpcvr_ctx *ctx, int32_t n, const void *const *tensors, const mpcvr_tensor_desc *desc,
                                         void *const *dsts, int32_t dst_pitch);
/* EXTENSION — a batch at field rate (the pass itself: mpcvr_deint_pass above).  frames[] holds n + 2 DEVICE samples of the context's input
 * layout: interior frame i = 1 .. n is deinterlaced with frames[i - 1] and frames[i + 1] as its neighbours (a caller repeats the first and
 * the last frame of a stream at the ends).  fields_per_frame is 1 (field 0 of every frame: frame rate) or 2 (both fields: field rate);
 * dsts[] holds n * fields_per_frame render targets, target (i - 1) * fields_per_frame + f showing field f of frame i, with keep and first
 * from field_order as for mpcvr_copy_sample_fields.  Target k holds, byte for byte, what
 *     mpcvr_deint_pass(frames[i - 1], frames[i], frames[i + 1], ..., keep, first, mode, sample k of the caller's, pitch), n * fields_per_frame times, then
 *     mpcvr_process_batch(samples -> dsts, dst_pitch)
 * leave, with ONE pass per chunk of output frames — its frame dimension: one k_deint launch per distinct (bytes, cs) among the planes,
 * reading a device table of (prev, cur, next, sample, keep, first) per output frame sent through the frame tables' ring — and no samples
 * of the caller's: they live in the context-owned sample surface of mpcvr_process_batch_from_tensors, output frame i of a chunk at i *
 * frame_stride, frame_stride = pitch * lines rounded up to 256 (mpcvr_plan_batch_deint; pitch and lines are the input's, lines as
 * mpcvr_get_frame_bytes counts them: bytes / pitch).  A chunk is what fits the budget of mpcvr_set_batch_yuv_budget (0: the default), at
 * least one frame, at most all — the library's one chunk rule.  Every chunk runs in stream order on the context stream: the pass, then the
 * chunk's mpcvr_process_batch work; the batch lanes are not used.  The samples are free in stream order behind the call; the targets are
 * complete after mpcvr_synchronize.  As for mpcvr_copy_sample_fields the sample format stays progressive.
 * Refusals, answered before anything is drawn, allocated or written: MPCVR_E_NOT_VALID_STATE before mpcvr_set_input; MPCVR_E_POINTER for
 * a NULL array or entry; MPCVR_E_INVALIDARG for n <= 0, a fields_per_frame, field_order or mode outside its set, an input format the pass
 * does not take, a sample that is no multiple of the component size, and whatever mpcvr_process_batch refuses about dsts and dst_pitch.
 * mpcvr_get_last_batch_info afterwards: "launches" counts the pass launches, and ";deint_chunks=<k>" follows. */
int32_t mpcvr_plan_batch_deint(int32_t pitch, int32_t lines, int32_t n_out, size_t budget_bytes,
                               size_t *frame_stride, int32_t *frames_per_chunk, int32_t *chunks);
int32_t mpcvr_process_batch_deint(mpcvr_ctx *ctx, int32_t n, const void *const *frames /* n + 2 device samples */, int32_t field_order,
                                  int32_t fields_per_frame /* 1 or 2 */, int32_t mode, void *const *dsts /* n * fields_per_frame targets */,
                                  int32_t dst_pitch);
/* EXTENSION — a batch through a 3D LUT (the pass itself: mpcvr_lut3d_pass above).  dsts[i] is the render target of frame i, all n of
 * dst_pitch and dst_fmt.  Target i holds, byte for byte, what
 *     mpcvr_process_batch(srcs -> n window-sized RGB targets of the context's output_format, black outside the video rect), then
 *     mpcvr_lut3d_pass(target i, output_format, window_w, window_h, lut_dev, lut_n, dsts[i], dst_pitch, dst_fmt), n times
 * leave, with ONE k_lut3d launch per chunk of frames (its frame dimension) where the composition takes n, and no intermediate targets of
 * the caller's.  The machinery is that of mpcvr_process_batch_tensor: the RGB frames live in the same context-owned surfaces (one per batch
 * lane used), laid out by mpcvr_plan_batch_lut3d — the formulas of mpcvr_plan_batch_tensor — under the budget of
 * mpcvr_set_batch_yuv_budget.  Chunks, routes, the letterbox and the order are as described for mpcvr_process_batch_yuv; every target
 * counts as bytes the chunk writes: single frames, batches and further calls that write memory a target in flight covers stay behind it
 * in queue order.  The intended use is a context whose output_format is MPCVR_OUT_RGB10A2, so that the table sees 10-bit codes, with
 * dst_fmt free.  The targets are complete after mpcvr_synchronize.
 * Refusals, answered before anything is drawn, allocated or written: MPCVR_E_NOT_VALID_STATE before mpcvr_set_input; MPCVR_E_POINTER for
 * a NULL array, entry or table; MPCVR_E_INVALIDARG for n <= 0, whatever mpcvr_lut3d_pass refuses about the table, dst_pitch, dst_fmt and
 * a dsts[i] (a target that overlaps the table included), and any two targets that overlap each other.
 * mpcvr_get_last_batch_info afterwards: "launches" counts one pass per chunk, and ";lut3d_chunks=<k>;lut3d_lanes=<lane,lane,...>"
 * follow (the lane of each chunk, -1 = the context stream; the first 64 chunks), then ";lut3d_table=lds" or ";lut3d_table=global":
 * where the pass read the table from. */
int32_t mpcvr_plan_batch_lut3d(int32_t window_w, int32_t window_h, int32_t n, size_t budget_bytes,
                               int32_t *surface_pitch, size_t *frame_stride, int32_t *frames_per_chunk, int32_t *chunks);
int32_t mpcvr_process_batch_lut3d(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, const void *lut_dev, int32_t lut_n,
                                  void *const *dsts, int32_t dst_pitch, int32_t dst_fmt);
/* EXTENSION — a batch through the deband pass (the pass itself: mpcvr_deband_pass above).  dsts[i] is the render target of frame i, all n
 * of dst_pitch and dst_fmt.  Target i holds, byte for byte, what
 *     mpcvr_process_batch(srcs -> n window-sized RGB targets of the context's output_format, black outside the video rect), then
 *     mpcvr_deband_pass(target i, output_format, window_w, window_h, params, seed + i (mod 2^32), dsts[i], dst_pitch, dst_fmt), n times
 * leave, with ONE k_deband launch per chunk of frames (its frame dimension) where the composition takes n, and no intermediate targets of
 * the caller's.  The machinery is that of mpcvr_process_batch_lut3d: the RGB frames live in the context-owned surfaces laid out by
 * mpcvr_plan_batch_deband — the formulas of mpcvr_plan_batch_tensor — under the budget of mpcvr_set_batch_yuv_budget; chunks, routes, the
 * letterbox and the order are as described for mpcvr_process_batch_yuv.  The targets are complete after mpcvr_synchronize.
 * Refusals, answered before anything is drawn, allocated or written: MPCVR_E_NOT_VALID_STATE before mpcvr_set_input; MPCVR_E_POINTER for
 * a NULL array, entry or params; MPCVR_E_INVALIDARG for n <= 0, whatever mpcvr_deband_pass refuses about the parameters, dst_pitch,
 * dst_fmt and a dsts[i], and any two targets that overlap each other.
 * mpcvr_get_last_batch_info afterwards: "launches" counts one pass per chunk, and ";deband_chunks=<k>;deband_lanes=<lane,lane,...>"
 * follow (the lane of each chunk, -1 = the context stream; the first 64 chunks), then ";deband_taps=lds" or ";deband_taps=global":
 * where the pass read its taps from. */
int32_t mpcvr_plan_batch_deband(int32_t window_w, int32_t window_h, int32_t n, size_t budget_bytes,
                                int32_t *surface_pitch, size_t *frame_stride, int32_t *frames_per_chunk, int32_t *chunks);
int32_t mpcvr_process_batch_deband(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, const mpcvr_deband_params *params, uint32_t seed,
                                   void *const *dsts, int32_t dst_pitch, int32_t dst_fmt);
/* EXTENSION — a batch through the sharpen pass (the pass itself: mpcvr_sharpen_pass above).  dsts[i] is the render target of frame i, all n
 * of dst_pitch and dst_fmt.  Target i holds, byte for byte, what
 *     mpcvr_process_batch(srcs -> n window-sized RGB targets of the context's output_format, black outside the video rect), then
 *     mpcvr_sharpen_pass(target i, output_format, window_w, window_h, params, seed + i (mod 2^32), dsts[i], dst_pitch, dst_fmt), n times
 * leave, with ONE k_sharpen launch per chunk of frames (its frame dimension) where the composition takes n, and no intermediate targets of
 * the caller's.  The machinery is that of mpcvr_process_batch_deband: the RGB frames live in the context-owned surfaces laid out by
 * mpcvr_plan_batch_sharpen — the formulas of mpcvr_plan_batch_tensor — under the budget of mpcvr_set_batch_yuv_budget; chunks, routes, the
 * letterbox and the order are as described for mpcvr_process_batch_yuv.  The targets are complete after mpcvr_synchronize.
 * Refusals, answered before anything is drawn, allocated or written: MPCVR_E_NOT_VALID_STATE before mpcvr_set_input; MPCVR_E_POINTER for
 * a NULL array, entry or params; MPCVR_E_INVALIDARG for n <= 0, whatever mpcvr_sharpen_pass refuses about the parameters, dst_pitch,
 * dst_fmt and a dsts[i], and any two targets that overlap each other.
 * mpcvr_get_last_batch_info afterwards: "launches" counts one pass per chunk, and ";sharpen_chunks=<k>;sharpen_lanes=<lane,lane,...>"
 * follow (the lane of each chunk, -1 = the context stream; the first 64 chunks). */
int32_t mpcvr_plan_batch_sharpen(int32_t window_w, int32_t window_h, int32_t n, size_t budget_bytes,
                                 int32_t *surface_pitch, size_t *frame_stride, int32_t *frames_per_chunk, int32_t *chunks);
int32_t mpcvr_process_batch_sharpen(mpcvr_ctx *ctx, int32_t n, const void *const *srcs, const mpcvr_sharpen_params *params, uint32_t seed,
                                    void *const *dsts, int32_t dst_pitch, int32_t dst_fmt);

/* Multi-GPU: the parameter blob (colour matrix, luminance scale, gamut matrix, resize phase weights,
 * dither table) a rank-0 context computes and every other rank adopts after an RCCL broadcast.
 * Two-call size protocol. */
int32_t mpcvr_get_param_blob(mpcvr_ctx *ctx, void *buf, size_t *size);
int32_t mpcvr_set_param_blob(mpcvr_ctx *ctx, const void *buf, size_t size);
/* The same exchange done by the library over RCCL ("one ncclBroadcast (RCCL, root 0) at context creation") for hosts
 * without Python: `nccl_comm` is an ncclComm_t the host created (ncclCommInitRank in a process-per-GPU host, ncclCommInitAll when
 * one process drives several devices), `rank` this context's rank in it.  The broadcast runs on the context's stream; the
 * library resolves librccl at the first call (it is not a link-time dependency).
 *   one process per GPU:       mpcvr_broadcast_param_blob(ctx, comm, 0, rank);
 *   one process, N devices:    ncclGroupStart(); for d: mpcvr_broadcast_param_blob_begin(ctx[d], comm[d], 0, d); ncclGroupEnd();
 *                              for d: mpcvr_broadcast_param_blob_end(ctx[d]);            (examples/c_multi_gpu_rccl.c)
 * There is no reference line to cite: the reference is single-GPU (Source/DX11Helper.cpp:81-112). */
int32_t mpcvr_broadcast_param_blob_begin(mpcvr_ctx *ctx, void *nccl_comm, int32_t root, int32_t rank);
int32_t mpcvr_broadcast_param_blob_end(mpcvr_ctx *ctx);
int32_t mpcvr_broadcast_param_blob(mpcvr_ctx *ctx, void *nccl_comm, int32_t root, int32_t rank);

/* Introspection used by tests / stats (GetVPInfo analogue, DX11VideoProcessor.cpp:4100+). */
int32_t mpcvr_get_color_matrix(mpcvr_ctx *ctx, float out12[12]);     /* cm_r, cm_g, cm_b, cm_c */
int32_t mpcvr_get_extfmt(mpcvr_ctx *ctx, uint32_t *extfmt);           /* after SpecifyExtendedFormat */
int32_t mpcvr_get_frame_bytes(mpcvr_ctx *ctx, size_t *bytes, int32_t *pitch);
/* The table image the exact-2x fused kernel stages into LDS, as baked for the current plan (two-call size protocol): 1024 uint16
 * (the dither table's fp16 bits) | 1024 uint32 ((uint32_t)(d * 1024 + 0.5) << 14) | 4096 float pairs {lut[i], lut[min(i+1, 4095)] - lut[i]}
 * of the plan's PQ -> SDR or HLG -> SDR table (zeros where the plan has none). */
int32_t mpcvr_get_fused_tables(mpcvr_ctx *ctx, void *buf, size_t *size);
int32_t mpcvr_get_path_info(mpcvr_ctx *ctx, char *buf, size_t buf_size); /* e.g. "fused_up2x" / "fused_jinc2x" / "passes:convert,resizeX,resizeY+final" */
/* How the last mpcvr_process_batch / mpcvr_process_batch_dovi call ran: "frames=<n>;launches=<kernel launches>;lane=<lane>;waits=<n>;uploads=<frame tables copied to the device in the stream>[;dovi_runs=<frames>:<tables|frames>,...]".
 * A batch on a whole-batch route launches a handful of kernels whatever n is (one per stage and <= 4 GiB chunk of intermediates); a
 * frame-by-frame one at least n.  dovi_runs: the runs mpcvr_process_batch_dovi cut the frames into and whether a run read its RPUs from the
 * per-frame tables or went frame by frame.  After mpcvr_process_batch_yuv ";yuv_chunks=<k>;yuv_lanes=<lane,lane,...>" follow and the launches
 * include one pass per chunk; after every other batch call the string is as above. */
int32_t mpcvr_get_last_batch_info(mpcvr_ctx *ctx, char *buf, size_t buf_size);
/* Once the context has launched the exact-2x fused kernel, ";up2x=bp" or ";up2x=generic" follows these fields (in front of the fields of
 * the extension calls): the form of the context's last such launch since the last batch call began, single frames included (bp: the bi-planar twin, which loads and converts every chroma texel once; generic: the kernel
 * every launch may take; MPCVR_UP2X_NO_BP=1 in the environment keeps to it).  A batch call that launches none reports neither.
 * Host, no GPU: 1 when the twin's carried chroma row is the row the generic kernel would load in every iteration of a launch over
 * source rows rect_t .. rect_t + h - 1 of a sample with ch chroma rows, for the siting coefficients (vk1, vk2, vk3) of
 * 4 v'(sy) = vk1 sy + vk2 (sy & ~1) + vk3; 0 otherwise (the launch then runs the generic kernel). */
int32_t mpcvr_plan_up2x_row_carry(int32_t vk1, int32_t vk2, int32_t vk3, int32_t rect_t, int32_t h, int32_t ch);
const char *mpcvr_last_error(mpcvr_ctx *ctx);
const char *mpcvr_version(void);

/* Timing of the last process/render on the context stream (hipEvent pair), milliseconds.
 * Mirrors m_RenderStats.paintticks (DX11VideoProcessor.cpp:2790).  Synchronises the stream.  Single frames that overlap on the
 * context's frame lanes are timed one in eight (the first always): two timestamped events around every 45 us kernel cost the per-frame
 * path 1.5 % at 4K -> 8K and 10-40 % on 1080p same-size frames; the figure is the most recent TIMED frame's (MPCVR_LANE_TIMING_EVERY=1
 * times them all; batches and frames off the lanes always are). */
int32_t mpcvr_get_last_process_ms(mpcvr_ctx *ctx, float *ms);
/* The renderer's other per-frame timers (FrameStats.h:145-173): copy_host_ms = wall time the last mpcvr_copy_sample spent on the host
 * (copyticks, DX11VideoProcessor.cpp:2594), upload_ms = its host-to-device transfer on the copy stream (hipEvent pair; absent for
 * device samples), process_ms = mpcvr_get_last_process_ms, readback_ms = the device-to-host copy of the last mpcvr_get_current_image.
 * -1 where nothing of the kind has been timed yet; any pointer may be NULL.  Synchronises the events it reads. */
int32_t mpcvr_get_last_timings(mpcvr_ctx *ctx, float *copy_host_ms, float *upload_ms, float *process_ms, float *readback_ms);

/* ---- host-side parameter maths, usable without a context or a GPU --------------------------------
 * The CPU work the reference does before touching the device.  Each mirrors a reference host function. */
/* pitch / byte size of one media sample — DX11VideoProcessor.cpp:1789-1803 (m_srcPitch, m_srcLines) */
int32_t mpcvr_plan_frame_layout(int32_t cformat, int32_t width, int32_t height, int32_t *pitch, size_t *bytes);
/* SpecifyExtendedFormat (Helper.cpp:1169-1211) + SetShaderConvertColorParams (DX11VideoProcessor.cpp:813-887)
 * -> mp_get_csp_matrix (csputils.cpp:392-509).  ProcAmp in DXVA2 units. */
int32_t mpcvr_plan_color_matrix(int32_t cformat, int32_t rect_w, int32_t rect_h, uint32_t extfmt,
                                float brightness, float contrast, float hue, float saturation,
                                float out12[12], uint32_t *extfmt_out);
/* GetColorspaceGamutConversionMatrix(BT.2020 -> BT.709) — csputils.cpp:549-557 */
int32_t mpcvr_plan_gamut_2020_to_709(float out9[9]);
/* the fused path's tone-map LUT: i/4095 -> Hable(ST2084ToLinear(x, lum_scale)) / hable(4.8) */
int32_t mpcvr_plan_pq_lut(float lum_scale, float out4096[4096]);
/* the fused path's integer form of ps_final_pass.hlsl:29: floor(k*quant/maxv + j/1024) == (k*M + (j << 14)) >> 24;
 * writes M (0 = not representable, the float epilogue is used) */
int32_t mpcvr_plan_final_pass_multiplier(int32_t quant, int32_t maxv, uint32_t *multiplier);
/* Dolby Vision host maths.  cb: the PS_DOVI_CURVE cbuffer of SetShaderDoviCurves (:1055-1141) as 3 x 235 floats — per
 * component pivots[7], coeffs[8][4], mmr[48][4], then {methods, mmr_single, min_order, max_order} as float values;
 * lms9: dovi_lms2rgb x rgb_to_lms_matrix (Shaders.cpp:826-842); l2k: {ChromaWeight, SaturationGain, TrimSlope, TrimOffset,
 * TrimPower} of SetDolbyVisionDynamicParams (:954-960) for a display of display_nits, *l2_enabled = L2Enabled;
 * l1_nits: {min, max, avg} as CopySample stores them (:2347-2372), *l1_present.  Any out pointer may be NULL. */
int32_t mpcvr_plan_dovi(const mpcvr_dovi_metadata *md, int32_t display_nits, float *cb705, int32_t *has_mmr,
                        float lms9[9], float l2k[5], int32_t *l2_enabled, uint32_t l1_nits[3], int32_t *l1_present);
/* ps_interpolation_{spline4,lanczos2,lanczos3}.hlsl weights for phase t; returns the tap count (4/6) or 0 */
int32_t mpcvr_plan_upscale_weights(int32_t iUpscaling, float t, float w6[6]);
/* tap table of one TextureResizeShader draw (DX11VideoProcessor.cpp:332-377): kind 0 = point sample,
 * 1 = upscale shader `method` (MPCVR_UPSCALE_*), 2 = ps_convolution with MPCVR_DOWNSCALE_* `method`.
 * idx/w: [n_out*cap_taps >= n_out*ntaps], dense with stride *ntaps; S_FALSE when cap_taps is too small. */
int32_t mpcvr_plan_axis_taps(int32_t kind, int32_t method, int32_t src_l, int32_t src_len, int32_t n_out,
                             int32_t tex_len, uint32_t flags, int32_t cap_taps, int32_t *idx, float *w,
                             float *wsum, int32_t *ntaps, int32_t *normalise);
/* Geometry of the arbitrary-ratio fused kernel (k_fused_strip) for an unrotated two-pass resize src_w x src_h -> out_w x out_h
 * with the given per-axis draws (kind / method as in mpcvr_plan_axis_taps): out8 = {taps per output the kernel runs (4/6/8),
 * pixels per lane, output columns per strip, rows of the LDS window, columns of a converted source row, strips, LDS bytes per
 * wavefront, 0}.  yrange: [out_h][2] {smallest, largest} source row per output row; xstrip: [strips][2] likewise per strip;
 * xi_t / xw_t: [taps][out_w] and yi / yw: [out_h][taps], the zero-padded, pre-normalised tables the kernel reads.  Any table
 * pointer may be NULL.  MPCVR_E_NOTIMPL: the tables do not fit the kernel (more than 16 taps, window above 31 rows). */
int32_t mpcvr_plan_strip(int32_t kind_x, int32_t method_x, int32_t kind_y, int32_t method_y, int32_t src_w, int32_t src_h,
                         int32_t out_w, int32_t out_h, uint32_t flags, int32_t out8[8], int32_t *yrange, int32_t *xstrip,
                         int32_t *xi_t, float *xw_t, int32_t *yi, float *yw);
/* Geometry of the periodic-phase fused kernel (k_fused_period) for an unrotated two-pass UPSCALE-shader resize (`method` =
 * MPCVR_UPSCALE_*; also what a downscale of at most 2x takes with bInterpolateAt50pct, DX11VideoProcessor.cpp:3108):
 * out6 = {P, Q (output : source rows), taps per output as the kernel runs them (4 / 5 = Lanczos3 with its shared texel folded /
 * 6), strips of *strip_w output columns (the width that fills the convert passes best, <= 128), columns of a converted source row, output rows per body of six source rows}.
 * xi_t / xw_t: [taps][out_w]; yw: [out_h][8]; xstrip: [strips][2]; any may be NULL.  MPCVR_E_NOTIMPL: the vertical ratio is not
 * 4:3 / 3:2 / 2:3 / 1:2 / 3:1 or the table's tap rows are not the periodic pattern the kernel hard-codes. */
int32_t mpcvr_plan_period(int32_t method, int32_t src_w, int32_t src_h, int32_t out_w, int32_t out_h, uint32_t flags,
                          int32_t out6[6], int32_t *xi_t, float *xw_t, float *yw, int32_t *xstrip, int32_t *strip_w);
/* Every table the resize draws of one plan read, as a context fresh from mpcvr_set_input (default ProcAmp, no HDR output, no Dolby Vision)
 * with these settings, source, rects, rotation and flip would build and upload them.  src_rect NULL: the whole frame.  Two-call size
 * protocol: buf = NULL stores the byte size in *size.  buf holds 4-byte words: a header of MPCVR_DRAW_TABLES_HEADER_WORDS int32, then the
 * first draw's axis pack, the second draw's, and the strip pack.  Header (offsets within a pack in words, -1: the pack has no such table):
 *   [0] header words  [1] screen axis of the first draw's taps  [2] first draw swaps the texture axes (rotation 90 / 270)
 *   [3] / [4] first / second draw runs the 2-D Jinc2m shader (no tables)  [5] strip tables planned  [6] [7] periodic rows P : Q (0: none)
 *   [8 + 16 a ...], a = 0 / 1 (first / second draw): pack offset in buf, pack words (0: no tables), ntaps, normalise, n_out, blk_span,
 *       blk8_span, blk32_span, other_identity, then the offsets of idx [n_out][ntaps], w, wsum [n_out], other, the block pack
 *       (blk_lo | pad to 64 words | idx_t [ntaps][n_out] | w_t | blk8_lo | blk32_lo), and the entries of `other`
 *   [40 ...]: strip pack offset in buf, words, the offsets of yrange | xstrip | xi_t | xw_t | yi | yw, of the periodic kernel's
 *       xi_t | xw_t | yw | xstrip, then the strip plan's {taps, pixels per lane, strip width, ring, columns} and the periodic plan's
 *       {taps, columns, strip width, lane ownership}
 * Every table of an axis pack starts on a 256-byte boundary of the pack.  MPCVR_E_NOTIMPL: a resize ratio outside the supported range. */
#define MPCVR_DRAW_TABLES_HEADER_WORDS 64
int32_t mpcvr_plan_draw_tables(const mpcvr_settings *s, int32_t cformat, int32_t src_w, int32_t src_h, const mpcvr_rect *src_rect,
                               const mpcvr_rect *video_rect, int32_t window_w, int32_t window_h, int32_t rotation, int32_t flip,
                               void *buf, size_t *size);
/* HDRParamsConstantBuffer_t as SetHDR10ShaderParams fills it (DX11VideoProcessor.cpp:907-923: defaults and clamps of the HDR10
 * metadata, the display's peak and the tone-mapping operator): five floats + the selection as words */
int32_t mpcvr_plan_hdr10_params(float min_mastering, float max_mastering, float max_cll, float max_fall, float display_max,
                                int32_t selection, uint32_t out6[6]);
/* log2 of ST2084ToLinear(x, 1) at x = (i/N)^2, i = 0 .. N: the PQ EOTF table of the Dolby Vision block convert (N = 8192 in this
 * build).  Two calls: out = NULL stores the number of floats (N + 1) in *count; then `capacity` floats of room — MPCVR_E_INVALIDARG when
 * that is fewer than the table has, nothing is written.  (Replaces mpcvr_plan_pq_eotf_lut(float[4096]) of round 3, whose table grew in
 * place in round 4: a caller that sizes its buffer from an old header can no longer be overrun.) */
int32_t mpcvr_plan_pq_eotf_table(float *out, int32_t capacity, int32_t *count);
/* DEPRECATED, one more release: the round-3 entry point with its fixed float[4096] — the same function on that 4096-point grid
 * (x = (i/4095)^2), so that a caller built against the old header links and is neither overrun nor handed a table of another size.
 * New code: mpcvr_plan_pq_eotf_table. */
int32_t mpcvr_plan_pq_eotf_lut(float out[4096]);
/* which draws Process() would issue (UpdateTexParams :1143, UpdatePostScaleTexures :2894, ResizeShaderPass :3103) */
int32_t mpcvr_plan_describe(const mpcvr_settings *s, int32_t cformat, int32_t rect_w, int32_t rect_h,
                            const mpcvr_rect *video_rect, int32_t window_w, int32_t window_h,
                            char *buf, size_t buf_size);

/* A measurement aid (bench.py: roofline.empirical_shape_peak_GBps), not part of the video path: one launch that reads src_bytes (a multiple of
 * 16, 16-byte aligned DEVICE buffers) once and writes fan * src_bytes — the fused kernels' traffic shape (a 4K P010 sample in, an 8K
 * B8G8R8A8 target out is 1 : 5.33) with no arithmetic.  dst holds fan * src_bytes bytes; stream = a hipStream_t or NULL. */
int32_t mpcvr_bandwidth_probe(const void *src_dev, void *dst_dev, size_t src_bytes, int32_t fan, void *stream);
/* ... and the exact-2x kernel's own shape over a whole batch in one launch (round 6): n (<= 64) bi-planar 16-bit 4:2:0 samples of src_w x src_h
 * (P010: src_w * src_h * 3 bytes each) and n targets of 2 src_w x 2 src_h x 4 bytes; a wavefront owns a strip of 120 source columns x
 * seg_rows source rows, reads two luma rows and a chroma row per step (240 contiguous bytes each) and writes four target rows (960 contiguous
 * bytes each, one 16-byte piece per lane), like csrc/vp_fused_up2x.h.  mode 0: read + write, 1: write only, 2: read only.  strip_cols (even, <= 128):
 * source columns per wavefront — 120 is the kernel's, 128 the 1 KiB-aligned variant of the same pattern.  The pointer arrays are
 * HOST arrays of DEVICE pointers (16-byte aligned). */
int32_t mpcvr_bandwidth_probe_up2x(int32_t mode, int32_t n, const void *const *srcs_dev, void *const *dsts_dev, int32_t src_w, int32_t src_h,
                                   int32_t seg_rows, int32_t strip_cols, void *stream);

/* A verification aid, not part of the video path: the transcendentals of the pass-per-kernel tier (csrc/vp_crmath.h — HLSL's
 * pow(x, y) = exp2(y * log2(x)) as d3dcompiler lowers it, Shaders/convert/st2084.hlsl:9-25, with every step the correctly rounded fp32
 * function) evaluated on the device over n floats: fn = 0 log2f(x), 1 exp2f(x), 2 expf(x), 3 powf(x, y), 4 sinf(x), 5 cosf(x) (the last two:
 * the windowed sinc / jinc weights of the resize shaders, ps_interpolation_lanczos3.hlsl:50-59, ps_resize_onepass_jinc2.hlsl:44-101); y_dev is read by fn = 3 only.
 * The tests hold the result to a CPU evaluation of the same definition bit for bit.  DEVICE buffers; stream = a hipStream_t or NULL. */
int32_t mpcvr_eval_transcendental(int32_t fn, const float *x_dev, const float *y_dev, float *out_dev, size_t n, void *stream);
/* ... and the pass-per-kernel tier's Dolby Vision tail (csrc/vp_device.h: PQ EOTF -> LMS matrix -> PQ OETF, Shaders.cpp:844-859; level-2 trims
 * :766-773; ST2084ToLinear * scale; Hable; 2020 -> 709; pow 1/2.2, :870-923) over n PQ-coded RGB triples, cut off after `stage` (0 .. 5 in that
 * order): the tests hold every stage to the oracle's bit for bit.  lms9 / l2k5 as mpcvr_plan_dovi returns them.  DEVICE buffers of 3 n floats. */
int32_t mpcvr_eval_dovi_tail(int32_t stage, const float *rgb_dev, float *out_dev, size_t n, const float lms9[9], const float l2k5[5], int32_t l2_enabled,
                             float lum_scale, void *stream);
/* ... and the same functions compiled for the host, over HOST buffers (no GPU needed: the CPU suite's check of the definition) */
int32_t mpcvr_eval_transcendental_host(int32_t fn, const float *x, const float *y, float *out, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* MPCVR_H */
