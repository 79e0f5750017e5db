"""Host-side mirror of the reference's video-processor interface over the C-ABI (include/mpcvr.h).

`VideoProcessor` follows CVideoProcessor / CDX11VideoProcessor (Source/VideoProcessor.h:171-236,
Source/DX11VideoProcessor.h:256-384): same method names, argument meaning and HRESULT-style error
behaviour, so the parity tests read like calls into the reference.  All arithmetic happens in
libmpcvr.so (hand-written HIP for gfx950); there is NO CPU fallback — a missing library or a missing
GPU raises.  PyTorch only supplies device memory and streams.
"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmpcvr.so")

S_OK, S_FALSE = 0, 1
E_FAIL = -2147467259          # 0x80004005
E_POINTER = -2147467261       # 0x80004003
E_INVALIDARG = -2147024809    # 0x80070057
E_UNEXPECTED = -2147418113    # 0x8000FFFF
E_NOTIMPL = -2147467263       # 0x80004001
E_OUTOFMEMORY = -2147024882   # 0x8007000E
E_NOT_VALID_STATE = -2147019873  # 0x8007139F

# ColorFormat_t (Source/Helper.h:86-127)
CF_NV12, CF_P010, CF_P016 = 1, 2, 3
CF_YUY2, CF_UYVY = 4, 5
CF_P210, CF_P216 = 6, 7
CF_Y210, CF_Y216, CF_V210, CF_AYUV, CF_Y410, CF_Y416 = 8, 9, 10, 11, 12, 13
CF_GBRP8, CF_GBRP10, CF_GBRP16 = 26, 27, 28
CF_Y8, CF_Y10, CF_Y16 = 37, 38, 39
CF_RGB24, CF_XRGB32, CF_ARGB32, CF_r210, CF_RGB48, CF_BGR48, CF_BGRA64, CF_B64A = 29, 30, 31, 32, 33, 34, 35, 36
CF_YV12, CF_YV16, CF_YV24 = 14, 15, 16
CF_YUV420P8, CF_YUV422P8, CF_YUV444P8 = 17, 18, 19
CF_YUV420P10, CF_YUV420P16, CF_YUV422P10, CF_YUV422P16, CF_YUV444P10, CF_YUV444P16 = 20, 21, 22, 23, 24, 25

# Settings enums (Source/IVideoRenderer.h:25-72)
TEXFMT_AUTOINT, TEXFMT_8INT, TEXFMT_10INT, TEXFMT_16FLOAT = 0, 8, 10, 16
CHROMA_Nearest, CHROMA_Bilinear, CHROMA_CatmullRom = 0, 1, 2
UPSCALE_Nearest, UPSCALE_Mitchell, UPSCALE_CatmullRom, UPSCALE_Lanczos2, UPSCALE_Lanczos3, UPSCALE_Jinc2 = range(6)
UPSCALE_Spline36_EXT = 6          # extension: not a reference setting (IVideoRenderer.h:54-62)
DOWNSCALE_Box, DOWNSCALE_Bilinear, DOWNSCALE_Hamming, DOWNSCALE_Bicubic, DOWNSCALE_BicubicSharp, DOWNSCALE_Lanczos = range(6)
OUT_BGRA8, OUT_RGB10A2 = 0, 1
DITHER_None, DITHER_Ordered, DITHER_ErrorDiffusion_EXT = 0, 1, 2     # bUseDither; 2 is an extension (error diffusion, include/mpcvr.h)
FLAG_LANCZOS3_FIXED, FLAG_NO_FUSED, FLAG_NO_LUT, FLAG_NO_FAST_CONVERT, FLAG_FUSED_VALU, FLAG_FUSED_MFMA, FLAG_NO_STRIP = 1, 2, 4, 8, 16, 32, 64
FLAG_NO_PERIOD = 128
FLAG_FORCE_PERIOD = 256
FLAG_NO_FRAME_LANES = 512     # mpcvr_process strictly frame after frame (default: two overlapping lanes when the context owns its stream)
MEM_HOST, MEM_DEVICE, MEM_HOST_PINNED = 0, 1, 2
PROCAMP_BRIGHTNESS, PROCAMP_CONTRAST, PROCAMP_HUE, PROCAMP_SATURATION = 1, 2, 4, 8

# DXVA2_ExtendedFormat codes used by the reference (Helper.cpp:1215-1223)
CHROMA_LOC_MPEG1, CHROMA_LOC_MPEG2, CHROMA_LOC_COSITED = 1, 5, 7
RANGE_0_255, RANGE_16_235 = 1, 2
MATRIX_BT709, MATRIX_BT601, MATRIX_SMPTE240M, MATRIX_BT2020, MATRIX_YCGCO = 1, 2, 3, 4, 7
PRIM_BT709, PRIM_BT2020 = 2, 9
TRC_22, TRC_709, TRC_SRGB, TRC_PQ, TRC_HLG = 4, 5, 7, 15, 16


def make_extfmt(chroma=0, nominal_range=0, matrix=0, lighting=0, primaries=0, transfer=0, sample_format=0):
    """Pack DXVA2_ExtendedFormat.value (dxva2api.h bit layout, LSB first)."""
    return ((sample_format & 0xff) | ((chroma & 0xf) << 8) | ((nominal_range & 0x7) << 12) |
            ((matrix & 0x7) << 15) | ((lighting & 0xf) << 18) | ((primaries & 0x1f) << 22) |
            ((transfer & 0x1f) << 27))


class Settings(C.Structure):
    """mpcvr_settings == the subset of Settings_t (IVideoRenderer.h:104-135) that reaches this path."""
    _fields_ = [("iTexFormat", C.c_int32), ("iChromaScaling", C.c_int32), ("iUpscaling", C.c_int32),
                ("iDownscaling", C.c_int32), ("bInterpolateAt50pct", C.c_int32), ("bUseDither", C.c_int32),
                ("bDeintBlend", C.c_int32), ("bConvertToSdr", C.c_int32), ("iSDRDisplayNits", C.c_int32),
                ("output_format", C.c_int32), ("flags", C.c_uint32)]

    def copy(self, **kw):
        s = Settings()
        C.memmove(C.byref(s), C.byref(self), C.sizeof(Settings))
        for k, v in kw.items():
            setattr(s, k, v)
        return s


class Rect(C.Structure):
    _fields_ = [("left", C.c_int32), ("top", C.c_int32), ("right", C.c_int32), ("bottom", C.c_int32)]


class DoviCurve(C.Structure):          # mpcvr_dovi_curve
    _fields_ = [
        ("num_pivots", C.c_uint8), ("mapping_idc", C.c_uint8 * 8), ("poly_order", C.c_uint8 * 8),
        ("mmr_order", C.c_uint8 * 8), ("pivots", C.c_uint16 * 9),
        ("poly_coef", (C.c_int64 * 3) * 8), ("mmr_constant", C.c_int64 * 8), ("mmr_coef", ((C.c_int64 * 7) * 3) * 8),
    ]


class DoviL2(C.Structure):             # mpcvr_dovi_l2
    _fields_ = [(n, C.c_uint16) for n in ("target_max_pq", "trim_slope", "trim_offset", "trim_power",
                                          "trim_chroma_weight", "trim_saturation_gain")]


class DoviMetadata(C.Structure):       # mpcvr_dovi_metadata
    _fields_ = [
        ("bl_bit_depth", C.c_uint8), ("coef_log2_denom", C.c_uint8), ("source_max_pq", C.c_uint16),
        ("l1_present", C.c_uint8), ("l3_present", C.c_uint8),
        ("l1_min_pq", C.c_uint16), ("l1_max_pq", C.c_uint16), ("l1_avg_pq", C.c_uint16),
        ("l3_min_pq_offset", C.c_uint16), ("l3_max_pq_offset", C.c_uint16), ("l3_avg_pq_offset", C.c_uint16),
        ("n_l2", C.c_uint32), ("l2", DoviL2 * 32),
        ("ycc_to_rgb_matrix", C.c_double * 9), ("ycc_to_rgb_offset", C.c_double * 3), ("rgb_to_lms_matrix", C.c_double * 9),
        ("curves", DoviCurve * 3),
    ]

    @classmethod
    def from_dict(cls, d):
        """Build from the plain-dict form synth.dovi_metadata() produces:
        {bl_bit_depth, coef_log2_denom, source_max_pq, [l1_*, l3_*], l2: [{target_max_pq, trim_*}...],
         ycc_to_rgb_matrix[9], ycc_to_rgb_offset[3], rgb_to_lms_matrix[9],
         curves: 3 x {pivots: [...], pieces: [{order, poly: [c0,c1,c2]} | {order, constant, mmr: [[7]...]}]}}"""
        st = cls()
        for k in ("bl_bit_depth", "coef_log2_denom", "source_max_pq", "l1_present", "l3_present", "l1_min_pq",
                  "l1_max_pq", "l1_avg_pq", "l3_min_pq_offset", "l3_max_pq_offset", "l3_avg_pq_offset"):
            setattr(st, k, int(d.get(k, 0)))
        l2 = d.get("l2", [])
        st.n_l2 = len(l2)
        for i, e in enumerate(l2[:32]):
            for k, v in e.items():
                setattr(st.l2[i], k, int(v))
        for k in ("ycc_to_rgb_matrix", "ycc_to_rgb_offset", "rgb_to_lms_matrix"):
            getattr(st, k)[:] = [float(x) for x in d[k]]
        for c, cv in enumerate(d["curves"]):
            o = st.curves[c]
            o.num_pivots = cv.get("num_pivots", len(cv["pivots"]))
            o.pivots[:len(cv["pivots"])] = [int(x) for x in cv["pivots"]]
            for i, piece in enumerate(cv["pieces"]):
                if "poly" in piece:
                    o.mapping_idc[i] = piece.get("idc", 0)
                    o.poly_order[i] = piece["order"]
                    for j, x in enumerate(piece["poly"]):
                        o.poly_coef[i][j] = int(x)
                else:
                    o.mapping_idc[i] = piece.get("idc", 1)
                    o.mmr_order[i] = piece["order"]
                    o.mmr_constant[i] = int(piece["constant"])
                    for j, row in enumerate(piece["mmr"]):
                        for k, x in enumerate(row):
                            o.mmr_coef[i][j][k] = int(x)
        return st


HIST_BINS = 1024


class LightLevel(C.Structure):         # mpcvr_light_level
    _fields_ = [("pixels", C.c_uint64), ("min_code", C.c_int32), ("max_code", C.c_int32), ("max_nits", C.c_double), ("avg_nits", C.c_double)]


TENSOR_F32, TENSOR_F16, TENSOR_BF16 = 0, 1, 2
TENSOR_PLANAR, TENSOR_INTERLEAVED = 0, 1          # C,H,W / H,W,C
TENSOR_RGB, TENSOR_BGR = 0, 1


class TensorDesc(C.Structure):         # mpcvr_tensor_desc
    _fields_ = [("dtype", C.c_int32), ("layout", C.c_int32), ("channel_order", C.c_int32), ("reserved", C.c_int32),
                ("row_pitch", C.c_int64), ("plane_pitch", C.c_int64), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


def tensor_desc(dtype, layout, row_pitch, plane_pitch=0, scale=(1 / 255,) * 3, bias=(0,) * 3, channel_order=TENSOR_RGB):
    """(extension) An mpcvr_tensor_desc: dtype TENSOR_F32 / F16 / BF16, layout TENSOR_PLANAR / INTERLEAVED, pitches in bytes, scale and
    bias for R, G, B of the picture (rounded to fp32 here, as the C struct holds them)."""
    d = TensorDesc(int(dtype), int(layout), int(channel_order), 0, int(row_pitch), int(plane_pitch))
    for k in range(3):
        d.scale[k], d.bias[k] = float(scale[k]), float(bias[k])
    return d


# (extension) motion-adaptive deinterlacing: the modes of mpcvr_deint_pass, and a plane as mpcvr_plan_deint_planes describes it
DEINT_ADAPTIVE_EXT, DEINT_ADAPTIVE_NOCHECK_EXT = 0, 1
FIELD_ORDER_TFF, FIELD_ORDER_BFF = 1, 2


class DeintPlane(C.Structure):
    _fields_ = [("offset", C.c_size_t), ("pitch", C.c_int32), ("comps", C.c_int32), ("lines", C.c_int32), ("bytes", C.c_int32),
                ("cs", C.c_int32), ("mask", C.c_int32)]


class DebandParams(C.Structure):       # mpcvr_deband_params
    _fields_ = [("range", C.c_int32), ("iterations", C.c_int32), ("threshold", C.c_int32), ("dither", C.c_int32)]


class SharpenParams(C.Structure):      # mpcvr_sharpen_params
    _fields_ = [("radius", C.c_int32), ("amount", C.c_int32), ("threshold", C.c_int32), ("overshoot", C.c_int32), ("mode", C.c_int32), ("dither", C.c_int32)]


SHARPEN_RGB_EXT, SHARPEN_LUMA_EXT = 0, 1


class MpcvrError(RuntimeError):
    def __init__(self, hr, msg):
        super().__init__(f"HRESULT 0x{hr & 0xffffffff:08X}: {msg}")
        self.hr = hr


EXPORTS = [
    "mpcvr_settings_default", "mpcvr_create", "mpcvr_destroy", "mpcvr_set_stream", "mpcvr_synchronize",
    "mpcvr_set_input", "mpcvr_set_video_rect", "mpcvr_set_window_rect", "mpcvr_set_rotation", "mpcvr_set_error_diffusion_patience", "mpcvr_set_flip", "mpcvr_set_sample_format", "mpcvr_set_hdr_output", "mpcvr_set_hdr_metadata",
    "mpcvr_set_dovi_metadata", "mpcvr_plan_dovi", "mpcvr_correction_pass", "mpcvr_plan_correction_matrices",
    "mpcvr_configure", "mpcvr_set_procamp", "mpcvr_copy_sample", "mpcvr_process", "mpcvr_process_frames", "mpcvr_render",
    "mpcvr_get_backbuffer", "mpcvr_get_current_image", "mpcvr_get_displayed_image", "mpcvr_flush", "mpcvr_reset", "mpcvr_process_batch", "mpcvr_process_batch_dovi",
    "mpcvr_get_param_blob", "mpcvr_set_param_blob", "mpcvr_broadcast_param_blob_begin", "mpcvr_broadcast_param_blob_end",
    "mpcvr_broadcast_param_blob", "mpcvr_get_color_matrix", "mpcvr_get_extfmt",
    "mpcvr_get_frame_bytes", "mpcvr_get_fused_tables", "mpcvr_get_path_info", "mpcvr_get_last_batch_info", "mpcvr_plan_up2x_row_carry", "mpcvr_last_error", "mpcvr_version",
    "mpcvr_get_last_process_ms", "mpcvr_get_last_timings",
    "mpcvr_plan_frame_layout", "mpcvr_plan_color_matrix", "mpcvr_plan_gamut_2020_to_709", "mpcvr_plan_pq_lut",
    "mpcvr_plan_upscale_weights", "mpcvr_plan_axis_taps", "mpcvr_plan_describe", "mpcvr_plan_final_pass_multiplier",
    "mpcvr_plan_strip", "mpcvr_plan_pq_eotf_table", "mpcvr_plan_pq_eotf_lut", "mpcvr_bandwidth_probe", "mpcvr_plan_period", "mpcvr_plan_hdr10_params", "mpcvr_plan_draw_tables",
    "mpcvr_eval_transcendental", "mpcvr_eval_transcendental_host", "mpcvr_bandwidth_probe_up2x", "mpcvr_eval_dovi_tail",
    "mpcvr_plan_encode", "mpcvr_encode_pass", "mpcvr_render_yuv",
    "mpcvr_plan_batch_yuv", "mpcvr_set_batch_yuv_budget", "mpcvr_process_batch_yuv",
    "mpcvr_measure_pass", "mpcvr_measure_backbuffer", "mpcvr_process_batch_yuv_stats",
    "mpcvr_light_level_from_histogram", "mpcvr_histogram_percentile",
    "mpcvr_plan_tensor_value", "mpcvr_tensor_pass", "mpcvr_render_tensor", "mpcvr_plan_batch_tensor", "mpcvr_process_batch_tensor",
    "mpcvr_plan_sample_code", "mpcvr_sample_pass", "mpcvr_copy_sample_tensor", "mpcvr_plan_batch_from_tensors", "mpcvr_process_batch_from_tensors",
    "mpcvr_plan_deint_planes", "mpcvr_deint_plane_host", "mpcvr_deint_pass", "mpcvr_copy_sample_fields", "mpcvr_plan_batch_deint", "mpcvr_process_batch_deint",
    "mpcvr_plan_lut3d_entries", "mpcvr_plan_lut3d_value", "mpcvr_lut3d_pass", "mpcvr_render_lut3d", "mpcvr_plan_batch_lut3d", "mpcvr_process_batch_lut3d",
    "mpcvr_deband_params_default", "mpcvr_deband_host", "mpcvr_plan_deband", "mpcvr_deband_pass", "mpcvr_render_deband", "mpcvr_plan_batch_deband", "mpcvr_process_batch_deband",
    "mpcvr_sharpen_params_default", "mpcvr_sharpen_host", "mpcvr_plan_sharpen", "mpcvr_sharpen_pass", "mpcvr_render_sharpen", "mpcvr_plan_batch_sharpen", "mpcvr_process_batch_sharpen",
]

_lib = None


def load_library():
    """dlopen libmpcvr.so.  Raises (never falls back) when it has not been built.
    Side effect: imports torch first when it is installed (one HIP runtime for both, see below) unless MPCVR_NO_TORCH_IMPORT=1."""
    global _lib
    if _lib is not None:
        return _lib
    # MPCVR_LIB=<path>: load another build of the library instead (same-box A/B runs of tools/ against an older libmpcvr.so; entry
    # points that build lacks are skipped).  Never set in normal use.
    lib_path = os.environ.get("MPCVR_LIB") or LIB_PATH
    if not os.path.exists(lib_path):
        raise RuntimeError(f"{lib_path} is missing: run `python -m videorenderer_amd.build` "
                           "(or __graft_entry__.build()); there is no CPU fallback")
    # In a process that also uses torch, torch's bundled HIP runtime must be the one both share: libmpcvr.so resolves
    # libamdhip64 through the dynamic loader, and a second copy of the runtime (loaded first from /opt/rocm) sees no device once
    # torch has initialised its own.  Importing torch first — only if it is installed; the library itself does not need it —
    # makes the load order irrelevant.  A host that never touches torch can skip the (slow) import with MPCVR_NO_TORCH_IMPORT=1.
    if "torch" not in sys.modules and not os.environ.get("MPCVR_NO_TORCH_IMPORT"):
        try:
            import importlib.util
            if importlib.util.find_spec("torch") is not None:
                import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(lib_path)
    vp, i32, u32, f = C.c_void_p, C.c_int32, C.c_uint32, C.c_float
    P = C.POINTER
    sig = {
        "mpcvr_settings_default": [P(Settings)],
        "mpcvr_create": [P(Settings), i32, P(vp)],
        "mpcvr_destroy": [vp],
        "mpcvr_set_stream": [vp, vp],
        "mpcvr_synchronize": [vp],
        "mpcvr_set_input": [vp, i32, i32, i32, i32, P(Rect), u32],
        "mpcvr_set_video_rect": [vp, P(Rect)],
        "mpcvr_set_window_rect": [vp, P(Rect)],
        "mpcvr_set_rotation": [vp, i32],
        "mpcvr_set_error_diffusion_patience": [vp, i32],
        "mpcvr_set_flip": [vp, i32],
        "mpcvr_set_sample_format": [vp, i32],
        "mpcvr_set_hdr_output": [vp, i32, i32, f],
        "mpcvr_set_hdr_metadata": [vp, f, f, f, f],
        "mpcvr_set_dovi_metadata": [vp, P(DoviMetadata)],
        "mpcvr_plan_dovi": [P(DoviMetadata), i32, P(f), P(i32), P(f), P(f), P(i32), P(u32), P(i32)],
        "mpcvr_correction_pass": [i32, vp, i32, i32, vp, i32, i32, i32, i32, i32, vp],
        "mpcvr_plan_correction_matrices": [P(f), P(f), P(f)],
        "mpcvr_configure": [vp, P(Settings)],
        "mpcvr_set_procamp": [vp, u32, f, f, f, f],
        "mpcvr_copy_sample": [vp, vp, i32, i32],
        "mpcvr_process": [vp, vp, i32, P(Rect), P(Rect), i32],
        "mpcvr_render": [vp, i32],
        "mpcvr_process_frames": [vp, i32, P(C.c_void_p), i32, i32, P(C.c_void_p), i32],
        "mpcvr_get_backbuffer": [vp, P(vp), P(i32), P(i32), P(i32)],
        "mpcvr_get_displayed_image": [vp, C.c_void_p, P(C.c_size_t), i32, P(i32), P(i32), P(i32)],
        "mpcvr_get_current_image": [vp, vp, P(C.c_size_t)],
        "mpcvr_flush": [vp],
        "mpcvr_reset": [vp],
        "mpcvr_process_batch": [vp, i32, P(vp), P(vp), i32],
        "mpcvr_process_batch_dovi": [vp, i32, P(vp), P(vp), i32, P(DoviMetadata)],
        "mpcvr_get_param_blob": [vp, vp, P(C.c_size_t)],
        "mpcvr_set_param_blob": [vp, vp, C.c_size_t],
        "mpcvr_broadcast_param_blob_begin": [vp, vp, i32, i32],
        "mpcvr_broadcast_param_blob_end": [vp],
        "mpcvr_broadcast_param_blob": [vp, vp, i32, i32],
        "mpcvr_get_color_matrix": [vp, P(f)],
        "mpcvr_get_extfmt": [vp, P(u32)],
        "mpcvr_get_frame_bytes": [vp, P(C.c_size_t), P(i32)],
        "mpcvr_get_fused_tables": [vp, vp, P(C.c_size_t)],
        "mpcvr_get_path_info": [vp, C.c_char_p, C.c_size_t],
        "mpcvr_get_last_batch_info": [vp, C.c_char_p, C.c_size_t],
        "mpcvr_plan_up2x_row_carry": [i32, i32, i32, i32, i32, i32],
        "mpcvr_get_last_process_ms": [vp, P(f)],
        "mpcvr_get_last_timings": [vp, P(f), P(f), P(f), P(f)],
        "mpcvr_plan_frame_layout": [i32, i32, i32, P(i32), P(C.c_size_t)],
        "mpcvr_plan_color_matrix": [i32, i32, i32, u32, f, f, f, f, P(f), P(u32)],
        "mpcvr_plan_gamut_2020_to_709": [P(f)],
        "mpcvr_plan_pq_lut": [f, P(f)],
        "mpcvr_plan_final_pass_multiplier": [i32, i32, P(u32)],
        "mpcvr_plan_upscale_weights": [i32, f, P(f)],
        "mpcvr_plan_axis_taps": [i32, i32, i32, i32, i32, i32, u32, i32, P(i32), P(f), P(f), P(i32), P(i32)],
        "mpcvr_plan_strip": [i32, i32, i32, i32, i32, i32, i32, i32, u32, P(i32), P(i32), P(i32), P(i32), P(f), P(i32), P(f)],
        "mpcvr_plan_hdr10_params": [f, f, f, f, f, i32, P(u32)],
        "mpcvr_plan_period": [i32, i32, i32, i32, i32, u32, P(i32), P(i32), P(f), P(f), P(i32), P(i32)],
        "mpcvr_plan_pq_eotf_table": [P(f), i32, P(i32)],
        "mpcvr_plan_pq_eotf_lut": [P(f)],
        "mpcvr_bandwidth_probe": [C.c_void_p, C.c_void_p, C.c_size_t, i32, C.c_void_p],
        "mpcvr_bandwidth_probe_up2x": [i32, i32, P(C.c_void_p), P(C.c_void_p), i32, i32, i32, i32, C.c_void_p],
        "mpcvr_eval_transcendental": [i32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p],
        "mpcvr_eval_dovi_tail": [i32, C.c_void_p, C.c_void_p, C.c_size_t, P(f), P(f), i32, f, C.c_void_p],
        "mpcvr_eval_transcendental_host": [i32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
        "mpcvr_plan_describe": [P(Settings), i32, i32, i32, P(Rect), i32, i32, C.c_char_p, C.c_size_t],
        "mpcvr_plan_draw_tables": [P(Settings), i32, i32, i32, P(Rect), P(Rect), i32, i32, i32, i32, C.c_void_p, P(C.c_size_t)],
        "mpcvr_plan_encode": [i32, i32, u32, P(i32), P(i32), P(i32), P(i32), P(u32)],
        "mpcvr_encode_pass": [vp, i32, i32, i32, i32, i32, u32, vp, i32, vp, i32, vp],
        "mpcvr_render_yuv": [vp, i32, i32, u32, vp, i32, vp, i32],
        "mpcvr_plan_batch_yuv": [i32, i32, i32, C.c_size_t, P(i32), P(C.c_size_t), P(i32), P(i32)],
        "mpcvr_set_batch_yuv_budget": [vp, C.c_size_t],
        "mpcvr_process_batch_yuv": [vp, i32, P(vp), i32, u32, P(vp), i32, P(vp), i32],
        "mpcvr_measure_pass": [vp, i32, i32, i32, i32, P(Rect), vp, vp],
        "mpcvr_measure_backbuffer": [vp, vp],
        "mpcvr_process_batch_yuv_stats": [vp, i32, P(vp), i32, u32, P(vp), i32, P(vp), i32, vp],
        "mpcvr_light_level_from_histogram": [vp, i32, P(LightLevel)],
        "mpcvr_histogram_percentile": [vp, u32, P(i32)],
        "mpcvr_plan_tensor_value": [i32, i32, u32, f, f, P(u32)],
        "mpcvr_tensor_pass": [vp, i32, i32, i32, i32, P(TensorDesc), vp, vp],
        "mpcvr_render_tensor": [vp, i32, P(TensorDesc), vp],
        "mpcvr_plan_batch_tensor": [i32, i32, i32, C.c_size_t, P(i32), P(C.c_size_t), P(i32), P(i32)],
        "mpcvr_process_batch_tensor": [vp, i32, P(vp), P(TensorDesc), P(vp)],
        "mpcvr_plan_sample_code": [i32, i32, u32, f, f, P(u32)],
        "mpcvr_sample_pass": [vp, P(TensorDesc), i32, i32, i32, vp, i32, vp],
        "mpcvr_copy_sample_tensor": [vp, vp, P(TensorDesc)],
        "mpcvr_plan_batch_from_tensors": [i32, i32, i32, C.c_size_t, P(C.c_size_t), P(i32), P(i32)],
        "mpcvr_process_batch_from_tensors": [vp, i32, P(vp), P(TensorDesc), P(vp), i32],
        "mpcvr_plan_deint_planes": [i32, i32, i32, i32, P(i32), P(DeintPlane)],
        "mpcvr_deint_plane_host": [vp, vp, vp, C.c_int64, i32, i32, i32, i32, i32, i32, i32, i32, vp, C.c_int64],
        "mpcvr_deint_pass": [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, i32, vp],
        "mpcvr_copy_sample_fields": [vp, vp, vp, vp, i32, i32, i32],
        "mpcvr_plan_batch_deint": [i32, i32, i32, C.c_size_t, P(C.c_size_t), P(i32), P(i32)],
        "mpcvr_process_batch_deint": [vp, i32, P(vp), i32, i32, i32, P(vp), i32],
        "mpcvr_plan_lut3d_entries": [vp, i32, vp],
        "mpcvr_plan_lut3d_value": [i32, i32, vp, i32, u32, P(u32)],
        "mpcvr_lut3d_pass": [vp, i32, i32, i32, i32, vp, i32, vp, i32, i32, vp],
        "mpcvr_render_lut3d": [vp, i32, vp, i32, vp, i32, i32],
        "mpcvr_plan_batch_lut3d": [i32, i32, i32, C.c_size_t, P(i32), P(C.c_size_t), P(i32), P(i32)],
        "mpcvr_process_batch_lut3d": [vp, i32, P(vp), vp, i32, P(vp), i32, i32],
        "mpcvr_deband_params_default": [i32, P(DebandParams)],
        "mpcvr_deband_host": [vp, C.c_int64, i32, i32, i32, P(DebandParams), u32, vp, C.c_int64, i32],
        "mpcvr_plan_deband": [i32, P(DebandParams), i32, i32, P(i32), P(i32)],
        "mpcvr_deband_pass": [vp, i32, i32, i32, i32, P(DebandParams), u32, vp, i32, i32, vp],
        "mpcvr_render_deband": [vp, i32, P(DebandParams), u32, vp, i32, i32],
        "mpcvr_plan_batch_deband": [i32, i32, i32, C.c_size_t, P(i32), P(C.c_size_t), P(i32), P(i32)],
        "mpcvr_process_batch_deband": [vp, i32, P(vp), P(DebandParams), u32, P(vp), i32, i32],
        "mpcvr_sharpen_params_default": [i32, P(SharpenParams)],
        "mpcvr_sharpen_host": [vp, C.c_int64, i32, i32, i32, P(SharpenParams), u32, vp, C.c_int64, i32],
        "mpcvr_plan_sharpen": [i32, P(SharpenParams), i32, i32, P(i32), P(i32)],
        "mpcvr_sharpen_pass": [vp, i32, i32, i32, i32, P(SharpenParams), u32, vp, i32, i32, vp],
        "mpcvr_render_sharpen": [vp, i32, P(SharpenParams), u32, vp, i32, i32],
        "mpcvr_plan_batch_sharpen": [i32, i32, i32, C.c_size_t, P(i32), P(C.c_size_t), P(i32), P(i32)],
        "mpcvr_process_batch_sharpen": [vp, i32, P(vp), P(SharpenParams), u32, P(vp), i32, i32],
    }
    for name, args in sig.items():
        if lib_path != LIB_PATH and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = i32
    L.mpcvr_last_error.argtypes = [vp]
    L.mpcvr_last_error.restype = C.c_char_p
    L.mpcvr_version.argtypes = []
    L.mpcvr_version.restype = C.c_char_p
    _lib = L
    return L


def default_settings(**kw):
    s = Settings()
    load_library().mpcvr_settings_default(C.byref(s))
    for k, v in kw.items():
        setattr(s, k, v)
    return s


# ---- host-side parameter maths (no context, no GPU) ------------------------------------------------
def plan_frame_layout(cformat, width, height):
    pitch, nbytes = C.c_int32(), C.c_size_t()
    hr = load_library().mpcvr_plan_frame_layout(cformat, width, height, C.byref(pitch), C.byref(nbytes))
    if hr < 0:
        raise MpcvrError(hr, "mpcvr_plan_frame_layout")
    return nbytes.value, pitch.value


def plan_up2x_row_carry(vk1, vk2, vk3, rect_t, h, ch):
    """True when the exact-2x kernel's bi-planar twin may carry a chroma row from one iteration to the next over source rows
    rect_t .. rect_t + h - 1 of a sample with ch chroma rows (include/mpcvr.h: mpcvr_plan_up2x_row_carry)."""
    return bool(load_library().mpcvr_plan_up2x_row_carry(vk1, vk2, vk3, rect_t, h, ch))


def plan_color_matrix(cformat, rect_w, rect_h, extfmt=0, brightness=0.0, contrast=1.0, hue=0.0, saturation=1.0):
    out = (C.c_float * 12)()
    ex = C.c_uint32()
    hr = load_library().mpcvr_plan_color_matrix(cformat, rect_w, rect_h, extfmt, brightness, contrast, hue,
                                                saturation, out, C.byref(ex))
    if hr < 0:
        raise MpcvrError(hr, "mpcvr_plan_color_matrix")
    return list(out), ex.value


def plan_gamut_2020_to_709():
    out = (C.c_float * 9)()
    load_library().mpcvr_plan_gamut_2020_to_709(out)
    return list(out)


def plan_pq_lut(lum_scale):
    out = (C.c_float * 4096)()
    load_library().mpcvr_plan_pq_lut(lum_scale, out)
    return list(out)


def plan_final_pass_multiplier(quant, maxv):
    """M of the fused path's integer final pass, (k*M + (j << 14)) >> 24; 0 when not representable."""
    m = C.c_uint32(0)
    load_library().mpcvr_plan_final_pass_multiplier(quant, maxv, C.byref(m))
    return m.value


def plan_dovi(md, display_nits=1000):
    """Host maths of the Dolby Vision path (SetShaderDoviCurves, LMS matrix, level-2 selection, level-1 nits)."""
    st = md if isinstance(md, DoviMetadata) else DoviMetadata.from_dict(md)
    cb = (C.c_float * 705)(); lms = (C.c_float * 9)(); l2k = (C.c_float * 5)(); l1 = (C.c_uint32 * 3)()
    has_mmr, l2on, l1on = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    hr = load_library().mpcvr_plan_dovi(C.byref(st), int(display_nits), cb, C.byref(has_mmr), lms, l2k, C.byref(l2on),
                                        l1, C.byref(l1on))
    if hr:
        raise MpcvrError(hr, "mpcvr_plan_dovi")
    import numpy as np
    return dict(cb=np.array(cb, dtype=np.float32).reshape(3, 235), has_mmr=has_mmr.value,
                lms=np.array(lms, dtype=np.float32), l2k=np.array(l2k, dtype=np.float32), l2_enabled=l2on.value,
                l1_nits=np.array(l1, dtype=np.uint32), l1_present=l1on.value)


CORR_FIX_BT2020, CORR_FIX_YCGCO, CORR_FIXCONVERT_PQ_TO_SDR, CORR_FIXCONVERT_HLG_TO_SDR, CORR_CONVERT_PQ_TO_SDR, CORR_CONVERT_HLG_TO_PQ = range(1, 7)


def plan_correction_matrices():
    """fix_bt2020_matrix, fix_ycgco_matrix (4x4) and convert_matrix_2020_to_709 (3x3) of the correction shaders, in fp32."""
    a, b, g = (C.c_float * 16)(), (C.c_float * 16)(), (C.c_float * 9)()
    hr = load_library().mpcvr_plan_correction_matrices(a, b, g)
    if hr:
        raise MpcvrError(hr, "mpcvr_plan_correction_matrices")
    return list(a), list(b), list(g)


def correction_pass(kind, src, src_pitch, src_fmt, dst, dst_pitch, dst_fmt, w, h, sdr_nits=125, stream=None):
    """One m_pPSCorrection shader (CORR_*) over a device surface of 32-bit texels; fmt: 0 = BGRA8, 1 = RGB10A2."""
    hr = load_library().mpcvr_correction_pass(int(kind), C.c_void_p(_ptr(src)), int(src_pitch), int(src_fmt), C.c_void_p(_ptr(dst)),
                                              int(dst_pitch), int(dst_fmt), int(w), int(h), int(sdr_nits),
                                              C.c_void_p(stream) if stream else None)
    if hr:
        raise MpcvrError(hr, "mpcvr_correction_pass")


def plan_encode(out_cformat, src_fmt, extfmt=0):
    """(extension) The integers of the RGB -> NV12 / P010 pass (include/mpcvr.h: mpcvr_plan_encode): dict(coef = 3x3 int32 with rows
    Y, U, V and columns R, G, B, off = 3 int32, shift, siting (0 centre, 1 left, 2 top-left), extfmt = the description after its defaults).  No GPU needed."""
    import numpy as np
    coef, off = (C.c_int32 * 9)(), (C.c_int32 * 3)()
    shift, siting, ex = C.c_int32(), C.c_int32(), C.c_uint32()
    hr = load_library().mpcvr_plan_encode(int(out_cformat), int(src_fmt), int(extfmt), coef, off, C.byref(shift), C.byref(siting), C.byref(ex))
    if hr:
        raise MpcvrError(hr, "mpcvr_plan_encode")
    return dict(coef=np.array(coef, dtype=np.int32).reshape(3, 3), off=np.array(off, dtype=np.int32), shift=shift.value,
                siting=siting.value, extfmt=ex.value)


def encode_pass(src, src_pitch, src_fmt, w, h, out_cformat, extfmt, y_plane, y_pitch, uv_plane, uv_pitch, stream=None):
    """(extension) One device surface of 32-bit RGB texels (src_fmt: 0 = BGRA8, 1 = RGB10A2) written as NV12 / P010 planes."""
    hr = load_library().mpcvr_encode_pass(C.c_void_p(_ptr(src)), int(src_pitch), int(src_fmt), int(w), int(h), int(out_cformat), int(extfmt),
                                          C.c_void_p(_ptr(y_plane)), int(y_pitch), C.c_void_p(_ptr(uv_plane)), int(uv_pitch),
                                          C.c_void_p(stream) if stream else None)
    if hr:
        raise MpcvrError(hr, "mpcvr_encode_pass")


def measure_pass(src, src_pitch, src_fmt, w, h, hist, rect=None, stream=None):
    """(extension) The histogram of max(R, G, B) over `rect` = (left, top, right, bottom) (None: the whole surface) of one device surface of
    32-bit RGB texels (src_fmt: 0 = BGRA8, 1 = RGB10A2) into the 1024 uint32 words at `hist` (device tensor or address), which it overwrites
    (include/mpcvr.h: mpcvr_measure_pass).  Complete in stream order."""
    r = Rect(*[int(v) for v in rect]) if rect is not None else None
    hr = load_library().mpcvr_measure_pass(C.c_void_p(_ptr(src)), int(src_pitch), int(src_fmt), int(w), int(h), C.byref(r) if r is not None else None,
                                           C.c_void_p(_ptr(hist)), C.c_void_p(stream) if stream else None)
    if hr:
        raise MpcvrError(hr, "mpcvr_measure_pass")


def _host_hist(hist):
    import numpy as np
    h = np.ascontiguousarray(hist, dtype=np.uint32).reshape(-1)
    if h.size != HIST_BINS:
        raise ValueError("a histogram has %d bins" % HIST_BINS)
    return h


def light_level_from_histogram(hist, src_fmt):
    """(extension) dict(pixels, min_code, max_code, max_nits, avg_nits) of a host histogram (include/mpcvr.h: mpcvr_light_level_from_histogram).
    The nits mean something for a PQ surface only; MaxCLL / MaxFALL of a stream are the maxima of max_nits / avg_nits over its frames.  No GPU needed."""
    h = _host_hist(hist)
    out = LightLevel()
    hr = load_library().mpcvr_light_level_from_histogram(C.c_void_p(h.ctypes.data), int(src_fmt), C.byref(out))
    if hr:
        raise MpcvrError(hr, "mpcvr_light_level_from_histogram")
    return dict(pixels=out.pixels, min_code=out.min_code, max_code=out.max_code, max_nits=out.max_nits, avg_nits=out.avg_nits)


def histogram_percentile(hist, ppm):
    """(extension) The smallest code whose cumulative count reaches ceil(ppm * pixels / 10^6) (include/mpcvr.h: mpcvr_histogram_percentile).  No GPU needed."""
    h = _host_hist(hist)
    code = C.c_int32()
    hr = load_library().mpcvr_histogram_percentile(C.c_void_p(h.ctypes.data), int(ppm), C.byref(code))
    if hr:
        raise MpcvrError(hr, "mpcvr_histogram_percentile")
    return code.value


def plan_tensor_value(dtype, src_fmt, code, scale, bias):
    """(extension) The stored bits of one element of the tensor pass (include/mpcvr.h: mpcvr_plan_tensor_value): fp32 bits, or the 16 bits
    of fp16 / bf16, of code * scale + bias for a channel code of a BGRA8 (0) / RGB10A2 (1) surface.  No GPU needed."""
    bits = C.c_uint32()
    hr = load_library().mpcvr_plan_tensor_value(int(dtype), int(src_fmt), int(code), float(scale), float(bias), C.byref(bits))
    if hr:
        raise MpcvrError(hr, "mpcvr_plan_tensor_value")
    return bits.value


def tensor_pass(src, src_pitch, src_fmt, w, h, desc, dst, stream=None):
    """(extension) One device surface of 32-bit RGB texels (src_fmt: 0 = BGRA8, 1 = RGB10A2) written as the float tensor `desc`
    (tensor_desc) describes at `dst` (device tensor or address) (include/mpcvr.h: mpcvr_tensor_pass).  Complete in stream order."""
    hr = load_library().mpcvr_tensor_pass(C.c_void_p(_ptr(src)), int(src_pitch), int(src_fmt), int(w), int(h),
                                          C.byref(desc) if desc is not None else None, C.c_void_p(_ptr(dst)), C.c_void_p(stream) if stream else None)
    if hr:
        raise MpcvrError(hr, "mpcvr_tensor_pass")


def plan_batch_tensor(window_w, window_h, n, budget_bytes=0):
    """(extension) The layout integers of mpcvr_process_batch_tensor (include/mpcvr.h: mpcvr_plan_batch_tensor): plan_batch_yuv's formulas
    for a window of any parity.  No GPU needed."""
    pitch, fpc, chunks, stride = C.c_int32(), C.c_int32(), C.c_int32(), C.c_size_t()
    hr = load_library().mpcvr_plan_batch_tensor(int(window_w), int(window_h), int(n), int(budget_bytes), C.byref(pitch), C.byref(stride), C.byref(fpc), C.byref(chunks))
    if hr:
        raise MpcvrError(hr, "mpcvr_plan_batch_tensor")
    return dict(surface_pitch=pitch.value, frame_stride=stride.value, frames_per_chunk=fpc.value, chunks=chunks.value)


def plan_lut3d_entries(rgb, n):
    """(extension) The table of the 3D LUT pass from n^3 float triplets in .cube order, R fastest (include/mpcvr.h:
    mpcvr_plan_lut3d_entries): a numpy uint16 array of (n^3, 4) {R, G, B, pad = 0}, each component rint(clamp(x, 0, 1) * 65535) in double,
    NaN -> 0.  Host only, no GPU.  Upload it as it is (8 bytes per entry) for lut3d_pass."""
    import numpy as np
    n = int(n)
    rgb = np.ascontiguousarray(rgb, dtype=np.float32).reshape(-1, 3)
    if rgb.shape[0] != n ** 3:
        raise ValueError("a table of size %d takes %d triplets, not %d" % (n, n ** 3, rgb.shape[0]))
    out = np.empty((rgb.shape[0], 4), dtype=np.uint16)
    hr = load_library().mpcvr_plan_lut3d_entries(C.c_void_p(rgb.ctypes.data), n, C.c_void_p(out.ctypes.data))
    if hr != S_OK:
        raise MpcvrError(hr, "mpcvr_plan_lut3d_entries")
    return out


def plan_lut3d_value(src_fmt, dst_fmt, entries, n, texel):
    """(extension) One texel of the 3D LUT pass on the host (include/mpcvr.h: mpcvr_plan_lut3d_value): `entries` the (n^3, 4) uint16
    table in host memory, `texel` a 32-bit source texel or an array of them; the destination texel(s), bit for bit what the kernel writes."""
    import numpy as np
    entries = np.ascontiguousarray(entries, dtype=np.uint16)
    if entries.size != 4 * int(n) ** 3:
        raise ValueError("a table of size %d takes %d uint16 words, not %d" % (n, 4 * int(n) ** 3, entries.size))
    f = load_library().mpcvr_plan_lut3d_value
    ep, out = C.c_void_p(entries.ctypes.data), C.c_uint32()
    scalar = np.ndim(texel) == 0
    res = []
    for t in np.atleast_1d(np.asarray(texel, dtype=np.uint32)).ravel().tolist():
        hr = f(int(src_fmt), int(dst_fmt), ep, int(n), t, C.byref(out))
        if hr != S_OK:
            raise MpcvrError(hr, "mpcvr_plan_lut3d_value")
        res.append(out.value)
    return res[0] if scalar else np.array(res, dtype=np.uint32).reshape(np.shape(texel))


def lut3d_pass(src, src_pitch, src_fmt, w, h, lut, n, dst, dst_pitch, dst_fmt, stream=None):
    """(extension) One device surface of 32-bit RGB texels (0 = BGRA8, 1 = RGB10A2) through the 3D LUT at `lut` (device tensor or address:
    n^3 entries of 8 bytes, plan_lut3d_entries) into the surface at `dst`, of either format; dst may be src with the same pitch
    (include/mpcvr.h: mpcvr_lut3d_pass).  Complete in stream order."""
    hr = load_library().mpcvr_lut3d_pass(C.c_void_p(_ptr(src)), int(src_pitch), int(src_fmt), int(w), int(h), C.c_void_p(_ptr(lut)), int(n),
                                         C.c_void_p(_ptr(dst)), int(dst_pitch), int(dst_fmt), C.c_void_p(stream or 0))
    if hr != S_OK:
        raise MpcvrError(hr, "mpcvr_lut3d_pass")
    return hr


def plan_batch_lut3d(window_w, window_h, n, budget_bytes=0):
    """(extension) The layout integers of mpcvr_process_batch_lut3d (include/mpcvr.h: mpcvr_plan_batch_lut3d): plan_batch_tensor's formulas.
    dict(surface_pitch, frame_stride, frames_per_chunk, chunks).  Host only, no GPU."""
    pitch, stride, fpc, chunks = C.c_int32(), C.c_size_t(), C.c_int32(), C.c_int32()
    hr = load_library().mpcvr_plan_batch_lut3d(int(window_w), int(window_h), int(n), int(budget_bytes), C.byref(pitch), C.byref(stride), C.byref(fpc), C.byref(chunks))
    if hr != S_OK:
        raise MpcvrError(hr, "mpcvr_plan_batch_lut3d")
    return dict(surface_pitch=pitch.value, frame_stride=stride.value, frames_per_chunk=fpc.value, chunks=chunks.value)


def _deband_params(params):
    """a DebandParams from one, from a dict of its fields, or from a (range, iterations, threshold, dither) sequence"""
    if isinstance(params, DebandParams):
        return params
    if isinstance(params, dict):
        return DebandParams(**{k: int(v) for k, v in params.items()})
    return DebandParams(*[int(v) for v in params])


def deband_params_default(src_fmt):
    """(extension) The default parameters of the deband pass for a source of src_fmt (0 = BGRA8, 1 = RGB10A2) as a DebandParams
    (include/mpcvr.h: mpcvr_deband_params_default): range 16, iterations 2, threshold one 8-bit code, dither on.  Host only."""
    p = DebandParams()
    hr = load_library().mpcvr_deband_params_default(int(src_fmt), C.byref(p))
    if hr != S_OK:
        raise MpcvrError(hr, "mpcvr_deband_params_default")
    return p


def deband_host(src, src_fmt, params, seed, dst_fmt, src_pitch=None, dst=None, dst_pitch=None, w=None):
    """(extension) The deband pass over a surface in HOST memory, bit for bit what the kernel writes (include/mpcvr.h: mpcvr_deband_host).
    `src`: a (h, w) uint32 numpy array, or with src_pitch and w a uint8 array of h rows of src_pitch bytes.  Returns a (h, w) uint32 array,
    or fills `dst` (uint8, h rows of dst_pitch bytes) and returns it.  No GPU."""
    import numpy as np
    if src_pitch is None:
        src = np.ascontiguousarray(src, dtype=np.uint32)
        h, w = src.shape
        src_pitch = 4 * w
    else:
        h = (src.size + src_pitch - 4 * w) // src_pitch
    out = dst
    if out is None:
        out, dst_pitch = np.empty((h, w), dtype=np.uint32), 4 * w
    p = _deband_params(params)
    hr = load_library().mpcvr_deband_host(C.c_void_p(src.ctypes.data), int(src_pitch), int(src_fmt), int(w), int(h), C.byref(p), int(seed) & 0xffffffff,
                                          C.c_void_p(out.ctypes.data), int(dst_pitch), int(dst_fmt))
    if hr != S_OK:
        raise MpcvrError(hr, "mpcvr_deband_host")
    return out


def plan_deband(src_fmt, params, w, h):
    """(extension) (halo R = range * iterations, 'lds' | 'global': where a launch over a w x h surface reads its taps from)
    (include/mpcvr.h: mpcvr_plan_deband; MPCVR_DEBAND_TAPS overrides the rule where possible).  Host only, no GPU."""
    halo, place = C.c_int32(), C.c_int32()
    p = _deband_params(params)
    hr = load_library().mpcvr_plan_deband(int(src_fmt), C.byref(p), int(w), int(h), C.byref(halo), C.byref(place))
    if hr != S_OK:
        raise MpcvrError(hr, "mpcvr_plan_deband")
    return halo.value, "lds" if place.value == 1 else "global"


def deband_pass(src, src_pitch, src_fmt, w, h, params, seed, dst, dst_pitch, dst_fmt, stream=None):
    """(extension) One device surface of 32-bit RGB texels (0 = BGRA8, 1 = RGB10A2) through the deband pass into the surface at `dst`, of
    either format; dst must not overlap src (include/mpcvr.h: mpcvr_deband_pass).  Complete in stream order."""
    p = _deband_params(params)
    hr = load_library().mpcvr_deband_pass(C.c_void_p(_ptr(src)), int(src_pitch), int(src_fmt), int(w), int(h), C.byref(p), int(seed) & 0xffffffff,
                                          C.c_void_p(_ptr(dst)), int(dst_pitch), int(dst_fmt), C.c_void_p(stream or 0))
    if hr != S_OK:
        raise MpcvrError(hr, "mpcvr_deband_pass")
    return hr


def plan_batch_deband(window_w, window_h, n, budget_bytes=0):
    """(extension) The layout integers of mpcvr_process_batch_deband (include/mpcvr.h: mpcvr_plan_batch_deband): plan_batch_tensor's formulas.
    dict(surface_pitch, frame_stride, frames_per_chunk, chunks).  Host only, no GPU."""
    pitch, stride, fpc, chunks = C.c_int32(), C.c_size_t(), C.c_int32(), C.c_int32()
    hr = load_library().mpcvr_plan_batch_deband(int(window_w), int(window_h), int(n), int(budget_bytes), C.byref(pitch), C.byref(stride), C.byref(fpc), C.byref(chunks))
    if hr != S_OK:
        raise MpcvrError(hr, "mpcvr_plan_batch_deband")
    return dict(surface_pitch=pitch.value, frame_stride=stride.value, frames_per_chunk=fpc.value, chunks=chunks.value)


def _sharpen_params(params):
    """a SharpenParams from one, from a dict of its fields, or from a (radius, amount, threshold, overshoot, mode, dither) sequence"""
    if isinstance(params, SharpenParams):
        return params
    if isinstance(params, dict):
        return SharpenParams(**{k: int(v) for k, v in params.items()})
    return SharpenParams(*[int(v) for v in params])


def sharpen_params_default(src_fmt):
    """(extension) The default parameters of the sharpen pass for a source of src_fmt (0 = BGRA8, 1 = RGB10A2) as a SharpenParams
    (include/mpcvr.h: mpcvr_sharpen_params_default): radius 2, amount 32 / 64, threshold one 8-bit code, overshoot two, luma mode, dither
    on.  Host only."""
    p = SharpenParams()
    hr = load_library().mpcvr_sharpen_params_default(int(src_fmt), C.byref(p))
    if hr != S_OK:
        raise MpcvrError(hr, "mpcvr_sharpen_params_default")
    return p


def sharpen_host(src, src_fmt, params, seed, dst_fmt, src_pitch=None, dst=None, dst_pitch=None, w=None):
    """(extension) The sharpen pass over a surface in HOST memory, bit for bit what the kernel writes (include/mpcvr.h: mpcvr_sharpen_host).
    `src`: a (h, w) uint32 numpy array, or with src_pitch and w a uint8 array of h rows of src_pitch bytes.  Returns a (h, w) uint32 array,
    or fills `dst` (uint8, h rows of dst_pitch bytes) and returns it.  No GPU."""
    import numpy as np
    if src_pitch is None:
        src = np.ascontiguousarray(src, dtype=np.uint32)
        h, w = src.shape
        src_pitch = 4 * w
    else:
        h = (src.size + src_pitch - 4 * w) // src_pitch
    out = dst
    if out is None:
        out, dst_pitch = np.empty((h, w), dtype=np.uint32), 4 * w
    p = _sharpen_params(params)
    hr = load_library().mpcvr_sharpen_host(C.c_void_p(src.ctypes.data), int(src_pitch), int(src_fmt), int(w), int(h), C.byref(p), int(seed) & 0xffffffff,
                                           C.c_void_p(out.ctypes.data), int(dst_pitch), int(dst_fmt))
    if hr != S_OK:
        raise MpcvrError(hr, "mpcvr_sharpen_host")
    return out


def plan_sharpen(src_fmt, params, w, h):
    """(extension) (halo = radius, the LDS bytes of one workgroup) of a launch over a w x h surface (include/mpcvr.h: mpcvr_plan_sharpen).
    Host only, no GPU."""
    halo, lds = C.c_int32(), C.c_int32()
    p = _sharpen_params(params)
    hr = load_library().mpcvr_plan_sharpen(int(src_fmt), C.byref(p), int(w), int(h), C.byref(halo), C.byref(lds))
    if hr != S_OK:
        raise MpcvrError(hr, "mpcvr_plan_sharpen")
    return halo.value, lds.value


def sharpen_pass(src, src_pitch, src_fmt, w, h, params, seed, dst, dst_pitch, dst_fmt, stream=None):
    """(extension) One device surface of 32-bit RGB texels (0 = BGRA8, 1 = RGB10A2) through the sharpen pass into the surface at `dst`, of
    either format; dst must not overlap src (include/mpcvr.h: mpcvr_sharpen_pass).  Complete in stream order."""
    p = _sharpen_params(params)
    hr = load_library().mpcvr_sharpen_pass(C.c_void_p(_ptr(src)), int(src_pitch), int(src_fmt), int(w), int(h), C.byref(p), int(seed) & 0xffffffff,
                                           C.c_void_p(_ptr(dst)), int(dst_pitch), int(dst_fmt), C.c_void_p(stream or 0))
    if hr != S_OK:
        raise MpcvrError(hr, "mpcvr_sharpen_pass")
    return hr


def plan_batch_sharpen(window_w, window_h, n, budget_bytes=0):
    """(extension) The layout integers of mpcvr_process_batch_sharpen (include/mpcvr.h: mpcvr_plan_batch_sharpen): plan_batch_tensor's formulas.
    dict(surface_pitch, frame_stride, frames_per_chunk, chunks).  Host only, no GPU."""
    pitch, stride, fpc, chunks = C.c_int32(), C.c_size_t(), C.c_int32(), C.c_int32()
    hr = load_library().mpcvr_plan_batch_sharpen(int(window_w), int(window_h), int(n), int(budget_bytes), C.byref(pitch), C.byref(stride), C.byref(fpc), C.byref(chunks))
    if hr != S_OK:
        raise MpcvrError(hr, "mpcvr_plan_batch_sharpen")
    return dict(surface_pitch=pitch.value, frame_stride=stride.value, frames_per_chunk=fpc.value, chunks=chunks.value)


def read_cube(path):
    """(extension) A .cube file with a 3D table: (n, float32 array of (n^3, 3)) in the file's order, R fastest, which is the order
    plan_lut3d_entries takes.  LUT_3D_SIZE, TITLE and # comments are understood; DOMAIN_MIN / DOMAIN_MAX are folded in linearly (a value
    v of channel k becomes (v - min[k]) / (max[k] - min[k])).  A LUT_1D_SIZE file, another keyword, or an entry count that is not n^3 raises
    ValueError."""
    import numpy as np
    n, lo, hi, rows = None, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], []
    with open(path, "r", encoding="utf-8", errors="replace") as fh:
        for ln, raw in enumerate(fh, 1):
            line = raw.split("#", 1)[0].strip()
            if not line:
                continue
            tok = line.split()
            key = tok[0].upper()
            if key == "TITLE":
                continue
            if key == "LUT_1D_SIZE":
                raise ValueError("%s:%d: a 1D table (LUT_1D_SIZE); the pass takes a 3D table" % (path, ln))
            if key == "LUT_3D_SIZE":
                if len(tok) != 2 or n is not None:
                    raise ValueError("%s:%d: LUT_3D_SIZE takes one integer, once" % (path, ln))
                n = int(tok[1])
                if not 2 <= n <= 65:
                    raise ValueError("%s:%d: a table size of %d is outside 2 .. 65" % (path, ln, n))
                continue
            if key in ("DOMAIN_MIN", "DOMAIN_MAX"):
                if len(tok) != 4:
                    raise ValueError("%s:%d: %s takes three numbers" % (path, ln, key))
                (lo if key == "DOMAIN_MIN" else hi)[:] = [float(x) for x in tok[1:]]
                continue
            if key[0].isalpha() and key not in ("NAN", "INF", "INFINITY"):
                raise ValueError("%s:%d: unknown keyword %s" % (path, ln, tok[0]))
            if len(tok) != 3:
                raise ValueError("%s:%d: a table line takes three numbers" % (path, ln))
            rows.append([float(x) for x in tok])
    if n is None:
        raise ValueError("%s: no LUT_3D_SIZE" % path)
    if len(rows) != n ** 3:
        raise ValueError("%s: %d entries, LUT_3D_SIZE %d takes %d" % (path, len(rows), n, n ** 3))
    if any(not h > l for l, h in zip(lo, hi)):
        raise ValueError("%s: DOMAIN_MAX must lie above DOMAIN_MIN" % path)
    v = np.array(rows, dtype=np.float64)
    v = (v - np.array(lo)) / (np.array(hi) - np.array(lo))
    return n, v.astype(np.float32)


def _tensor_dtype(dt):
    """torch dtype -> TENSOR_*"""
    import torch
    try:
        return {torch.float32: TENSOR_F32, torch.float16: TENSOR_F16, torch.bfloat16: TENSOR_BF16}[dt]
    except KeyError:
        raise ValueError("a tensor of float32, float16 or bfloat16, not %s" % (dt,)) from None


def _tensor_order(channel_order):
    try:
        return {"rgb": TENSOR_RGB, "bgr": TENSOR_BGR}[channel_order]
    except KeyError:
        raise ValueError("channel_order 'rgb' or 'bgr'") from None


def plan_sample_code(dtype, cformat, element_bits, scale, bias):
    """(extension) The code of one tensor element in a GBRP8 / GBRP10 / GBRP16 sample (include/mpcvr.h: mpcvr_plan_sample_code):
    element_bits are the fp32 bits, or the 16 bits of fp16 / bf16.  No GPU needed."""
    code = C.c_uint32()
    hr = load_library().mpcvr_plan_sample_code(int(dtype), int(cformat), int(element_bits), float(scale), float(bias), C.byref(code))
    if hr:
        raise MpcvrError(hr, "mpcvr_plan_sample_code")
    return code.value


def sample_pass(tensor, desc, w, h, cformat, sample, pitch, stream=None):
    """(extension) The float tensor `desc` (tensor_desc) describes at `tensor` (device tensor or address) written as a planar RGB sample
    (cformat CF_GBRP8 / GBRP10 / GBRP16; planes G, B, R, pitch * h apart) at `sample` (include/mpcvr.h: mpcvr_sample_pass).  Complete in
    stream order."""
    hr = load_library().mpcvr_sample_pass(C.c_void_p(_ptr(tensor)), C.byref(desc) if desc is not None else None, int(w), int(h), int(cformat),
                                          C.c_void_p(_ptr(sample)), int(pitch), C.c_void_p(stream) if stream else None)
    if hr:
        raise MpcvrError(hr, "mpcvr_sample_pass")


def plan_batch_from_tensors(pitch, h, n, budget_bytes=0):
    """(extension) The integers of ProcessBatchFromTensors' sample surface (include/mpcvr.h: mpcvr_plan_batch_from_tensors): dict(frame_stride,
    frames_per_chunk, chunks) for n samples of three planes of pitch * h bytes under a budget of bytes (0: the default).  No GPU needed."""
    fpc, chunks, stride = C.c_int32(), C.c_int32(), C.c_size_t()
    hr = load_library().mpcvr_plan_batch_from_tensors(int(pitch), int(h), int(n), int(budget_bytes), C.byref(stride), C.byref(fpc), C.byref(chunks))
    if hr:
        raise MpcvrError(hr, "mpcvr_plan_batch_from_tensors")
    return dict(frame_stride=stride.value, frames_per_chunk=fpc.value, chunks=chunks.value)


def plan_deint_planes(cformat, w, h, pitch=0):
    """(extension) The planes of a sample as the deinterlacing pass walks them (include/mpcvr.h: mpcvr_plan_deint_planes): a list of
    dict(offset, pitch, comps, lines, bytes, cs, mask).  No GPU needed."""
    n, out = C.c_int32(), (DeintPlane * 3)()
    hr = load_library().mpcvr_plan_deint_planes(int(cformat), int(w), int(h), int(pitch), C.byref(n), out)
    if hr:
        raise MpcvrError(hr, "mpcvr_plan_deint_planes")
    return [dict(offset=p.offset, pitch=p.pitch, comps=p.comps, lines=p.lines, bytes=p.bytes, cs=p.cs, mask=p.mask) for p in out[:n.value]]


def deint_plane_host(prev, cur, nxt, src_pitch, comps, lines, nbytes, cs, mask, keep, first, mode, dst, dst_pitch):
    """(extension) One plane in HOST memory by the definition of mpcvr_deint_pass (include/mpcvr.h: mpcvr_deint_plane_host): prev, cur, nxt
    and dst are numpy arrays or addresses, rows src_pitch / dst_pitch bytes apart.  No GPU needed."""
    hr = load_library().mpcvr_deint_plane_host(C.c_void_p(_ptr(prev)), C.c_void_p(_ptr(cur)), C.c_void_p(_ptr(nxt)), int(src_pitch), int(comps), int(lines),
                                               int(nbytes), int(cs), int(mask), int(keep), int(first), int(mode), C.c_void_p(_ptr(dst)), int(dst_pitch))
    if hr:
        raise MpcvrError(hr, "mpcvr_deint_plane_host")


def deint_pass(prev, cur, nxt, cformat, w, h, pitch, keep, first, mode, dst, dst_pitch, stream=None):
    """(extension) Motion-adaptive deinterlacing of the device sample `cur` between `prev` and `nxt` into the sample at `dst`, showing the
    field of parity `keep` (include/mpcvr.h: mpcvr_deint_pass).  Complete in stream order."""
    hr = load_library().mpcvr_deint_pass(C.c_void_p(_ptr(prev)), C.c_void_p(_ptr(cur)), C.c_void_p(_ptr(nxt)), int(cformat), int(w), int(h), int(pitch),
                                         int(keep), int(first), int(mode), C.c_void_p(_ptr(dst)), int(dst_pitch), C.c_void_p(stream) if stream else None)
    if hr:
        raise MpcvrError(hr, "mpcvr_deint_pass")


def plan_batch_deint(pitch, lines, n_out, budget_bytes=0):
    """(extension) The integers of ProcessBatchDeint's sample surface (include/mpcvr.h: mpcvr_plan_batch_deint): dict(frame_stride,
    frames_per_chunk, chunks) for n_out samples of pitch * lines bytes under a budget of bytes (0: the default).  No GPU needed."""
    fpc, chunks, stride = C.c_int32(), C.c_int32(), C.c_size_t()
    hr = load_library().mpcvr_plan_batch_deint(int(pitch), int(lines), int(n_out), int(budget_bytes), C.byref(stride), C.byref(fpc), C.byref(chunks))
    if hr:
        raise MpcvrError(hr, "mpcvr_plan_batch_deint")
    return dict(frame_stride=stride.value, frames_per_chunk=fpc.value, chunks=chunks.value)


def _frame_tensor_desc(t, scale, bias, channel_order):
    """The mpcvr_tensor_desc of one frame held by a torch tensor: (3, H, W) with a dense last dim, or (H, W, 3) with the last two dims
    dense; dtype and pitches are read off it (a slice works).  Returns (desc, w, h)."""
    es = t.element_size()
    if t.dim() == 3 and t.shape[0] == 3 and t.stride(2) == 1:          # (a (3, H, 3) tensor is taken as 3 planes of H x 3)
        return tensor_desc(_tensor_dtype(t.dtype), TENSOR_PLANAR, t.stride(1) * es, t.stride(0) * es, scale, bias, _tensor_order(channel_order)), t.shape[2], t.shape[1]
    if t.dim() == 3 and t.shape[2] == 3 and t.stride(2) == 1 and t.stride(1) == 3:
        return tensor_desc(_tensor_dtype(t.dtype), TENSOR_INTERLEAVED, t.stride(0) * es, 0, scale, bias, _tensor_order(channel_order)), t.shape[1], t.shape[0]
    raise ValueError("a tensor of shape %s / strides %s is neither (3, H, W) with a dense last dim nor (H, W, 3) with the last two dims dense"
                     % (tuple(t.shape), t.stride()))


def plan_batch_yuv(window_w, window_h, n, budget_bytes=0):
    """(extension) The layout integers of mpcvr_process_batch_yuv (include/mpcvr.h: mpcvr_plan_batch_yuv): dict(surface_pitch, frame_stride,
    frames_per_chunk, chunks) for n frames of a window under a budget of bytes (0: the default).  No GPU needed."""
    pitch, fpc, chunks, stride = C.c_int32(), C.c_int32(), C.c_int32(), C.c_size_t()
    hr = load_library().mpcvr_plan_batch_yuv(int(window_w), int(window_h), int(n), int(budget_bytes), C.byref(pitch), C.byref(stride), C.byref(fpc), C.byref(chunks))
    if hr:
        raise MpcvrError(hr, "mpcvr_plan_batch_yuv")
    return dict(surface_pitch=pitch.value, frame_stride=stride.value, frames_per_chunk=fpc.value, chunks=chunks.value)


def plan_upscale_weights(method, t):
    w = (C.c_float * 6)()
    n = load_library().mpcvr_plan_upscale_weights(method, t, w)
    return list(w)[:n]


def plan_strip(kind_x, method_x, kind_y, method_y, src_w, src_h, out_w, out_h, flags=0):
    """PlanFusedStrip through the C-ABI (no device): dict with the kernel's geometry and its tables as numpy arrays, or None when
    the resize does not fit the arbitrary-ratio fused kernel."""
    import numpy as np
    L = load_library()
    out8 = (C.c_int32 * 8)()
    hr = L.mpcvr_plan_strip(kind_x, method_x, kind_y, method_y, src_w, src_h, out_w, out_h, flags, out8, None, None, None, None, None, None)
    if hr == E_NOTIMPL:
        return None
    if hr != 0:
        raise MpcvrError(hr, "mpcvr_plan_strip")
    nt, pxl, strip_w, ring, acols, strips, lds_wave, _ = list(out8)
    yr = np.zeros((out_h, 2), np.int32); xs = np.zeros((strips, 2), np.int32)
    xi = np.zeros((nt, out_w), np.int32); xw = np.zeros((nt, out_w), np.float32)
    yi = np.zeros((out_h, nt), np.int32); yw = np.zeros((out_h, nt), np.float32)
    as_p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    hr = L.mpcvr_plan_strip(kind_x, method_x, kind_y, method_y, src_w, src_h, out_w, out_h, flags, out8, as_p(yr, C.c_int32), as_p(xs, C.c_int32),
                            as_p(xi, C.c_int32), as_p(xw, C.c_float), as_p(yi, C.c_int32), as_p(yw, C.c_float))
    if hr != 0:
        raise MpcvrError(hr, "mpcvr_plan_strip")
    return dict(taps=nt, px_per_lane=pxl, strip_w=strip_w, ring=ring, acols=acols, strips=strips, lds_per_wave=lds_wave,
                yrange=yr, xstrip=xs, xi_t=xi, xw_t=xw, yi=yi, yw=yw)


def plan_period(method, src_w, src_h, out_w, out_h, flags=0):
    """PlanFusedPeriod through the C-ABI (no device): the periodic-phase kernel's geometry and tables, or None when the vertical
    ratio is not one of 4:3 / 3:2 / 2:3 / 1:2 / 3:1 (or the tap rows are not the pattern the kernel hard-codes)."""
    import numpy as np
    L = load_library()
    out6 = (C.c_int32 * 6)()
    sw = C.c_int32(0)
    hr = L.mpcvr_plan_period(method, src_w, src_h, out_w, out_h, flags, out6, None, None, None, None, C.byref(sw))
    if hr == E_NOTIMPL:
        return None
    if hr != 0:
        raise MpcvrError(hr, "mpcvr_plan_period")
    Pn, Qn, nt, strips, acols, pb = list(out6)
    xi = np.zeros((nt, out_w), np.int32); xw = np.zeros((nt, out_w), np.float32)
    yw = np.zeros((out_h, 8), np.float32); xs = np.zeros((strips, 2), np.int32)
    as_p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    hr = L.mpcvr_plan_period(method, src_w, src_h, out_w, out_h, flags, out6, as_p(xi, C.c_int32), as_p(xw, C.c_float), as_p(yw, C.c_float), as_p(xs, C.c_int32), C.byref(sw))
    if hr != 0:
        raise MpcvrError(hr, "mpcvr_plan_period")
    return dict(strip_w=sw.value, P=Pn, Q=Qn, taps=nt, strips=strips, acols=acols, rows_per_body=pb, xi_t=xi, xw_t=xw, yw=yw, xstrip=xs)


def plan_draw_tables(settings, cformat, src_w, src_h, src_rect, video_rect, window_w, window_h, rotation=0, flip=False):
    """Every table the resize draws of one plan read, as the processor builds and uploads them (include/mpcvr.h:
    mpcvr_plan_draw_tables; no device).  dict: the header's scalars, `x` / `y` = the first / second draw's axis pack (None: the draw
    has no tables) and `strip` (None: not planned).  An axis pack: its scalars, `words` (the pack as int32), `off` (word offsets of
    idx / w / wsum / other / blk inside it, None where absent) and `n_other`; the strip pack: `words`, `off` (six), `period_off`
    (four, None without a periodic plan) and both plans' scalars."""
    import numpy as np
    L = load_library()
    size = C.c_size_t(0)
    src = C.byref(Rect(*src_rect)) if src_rect is not None else None
    args = (C.byref(settings), cformat, src_w, src_h, src, C.byref(Rect(*video_rect)), window_w, window_h, rotation, 1 if flip else 0)
    hr = L.mpcvr_plan_draw_tables(*args, None, C.byref(size))
    if hr != 0:
        raise MpcvrError(hr, "mpcvr_plan_draw_tables")
    buf = np.zeros(size.value // 4, np.int32)
    hr = L.mpcvr_plan_draw_tables(*args, buf.ctypes.data, C.byref(size))
    if hr != 0:
        raise MpcvrError(hr, "mpcvr_plan_draw_tables")
    h = [int(v) for v in buf[:int(buf[0])]]
    out = dict(first_axis=h[1], first_swap=h[2], first_jinc=h[3], second_jinc=h[4], strip_planned=h[5], P=h[6], Q=h[7])
    for a, name in enumerate("xy"):
        o = h[8 + 16 * a:24 + 16 * a]
        out[name] = None if o[1] == 0 else dict(
            words=buf[o[0]:o[0] + o[1]], ntaps=o[2], normalise=o[3], n_out=o[4], blk_span=o[5], blk8_span=o[6], blk32_span=o[7],
            other_identity=o[8], off=dict(zip(("idx", "w", "wsum", "other", "blk"), (None if v < 0 else v for v in o[9:14]))), n_other=o[14])
    o = h[40:61]
    out["strip"] = None if not h[5] else dict(
        words=buf[o[0]:o[0] + o[1]], off=o[2:8], period_off=o[8:12] if h[6] else None, taps=o[12], px_per_lane=o[13], strip_w=o[14],
        ring=o[15], acols=o[16], period_taps=o[17], period_acols=o[18], period_strip_w=o[19], period_own=o[20])
    return out


def plan_pq_eotf_lut():
    import numpy as np
    L = load_library()
    n = C.c_int32(0)
    hr = L.mpcvr_plan_pq_eotf_table(None, 0, C.byref(n))
    if hr:
        raise MpcvrError(hr, "mpcvr_plan_pq_eotf_table")
    out = np.zeros(n.value, np.float32)
    hr = L.mpcvr_plan_pq_eotf_table(out.ctypes.data_as(C.POINTER(C.c_float)), n.value, None)
    if hr:
        raise MpcvrError(hr, "mpcvr_plan_pq_eotf_table")
    return out


def plan_axis_taps(kind, method, src_l, src_len, n_out, tex_len, flags=0, cap_taps=160):
    """Returns (idx[n_out][ntaps], w[n_out][ntaps], wsum[n_out] or None) as nested lists."""
    idx = (C.c_int32 * (n_out * cap_taps))()
    w = (C.c_float * (n_out * cap_taps))()
    ws = (C.c_float * n_out)()
    nt, norm = C.c_int32(), C.c_int32()
    hr = load_library().mpcvr_plan_axis_taps(kind, method, src_l, src_len, n_out, tex_len, flags, cap_taps,
                                             idx, w, ws, C.byref(nt), C.byref(norm))
    if hr != 0:
        raise MpcvrError(hr, "mpcvr_plan_axis_taps")
    n = nt.value
    I = [list(idx[i * n:(i + 1) * n]) for i in range(n_out)]
    W = [list(w[i * n:(i + 1) * n]) for i in range(n_out)]
    return I, W, (list(ws) if norm.value else None)


def plan_describe(settings, cformat, rect_w, rect_h, video_rect, window_w, window_h):
    buf = C.create_string_buffer(256)
    hr = load_library().mpcvr_plan_describe(C.byref(settings), cformat, rect_w, rect_h, C.byref(Rect(*video_rect)),
                                            window_w, window_h, buf, 256)
    if hr < 0:
        raise MpcvrError(hr, buf.value.decode())
    return buf.value.decode()


def _ptr(x):
    """Device/host address of a torch tensor, numpy array or int."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if hasattr(x, "ctypes"):
        return x.ctypes.data
    return int(x)


class PreparedBatch:
    __slots__ = ("n", "sa", "da", "keep")

    def __init__(self, n, sa, da, keep):
        self.n, self.sa, self.da, self.keep = n, sa, da, keep


class VideoProcessor:
    """One processor context on one GPU (not re-entrant, like the reference under m_RendererLock)."""

    def __init__(self, settings=None, device=0, use_torch_stream=True):
        self._L = load_library()
        self._ctx = C.c_void_p()
        self.settings = settings.copy() if settings is not None else default_settings()
        hr = self._L.mpcvr_create(C.byref(self.settings), device, C.byref(self._ctx))
        if hr < 0:
            self._ctx = C.c_void_p()
            raise MpcvrError(hr, "mpcvr_create failed (is a HIP device visible?)")
        self.device = device
        self._keep = []
        if use_torch_stream:
            import torch
            with torch.cuda.device(device):
                self.SetStream(torch.cuda.current_stream().cuda_stream)

    # -- plumbing --------------------------------------------------------------------------------
    def _check(self, hr, allow_false=True):
        if hr < 0:
            raise MpcvrError(hr, self._L.mpcvr_last_error(self._ctx).decode())
        return hr

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._L.mpcvr_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def SetStream(self, hip_stream):
        return self._check(self._L.mpcvr_set_stream(self._ctx, C.c_void_p(hip_stream or 0)))

    def Synchronize(self):
        return self._check(self._L.mpcvr_synchronize(self._ctx))

    # -- CVideoProcessor surface -------------------------------------------------------------------
    def InitMediaType(self, cformat, width, height, pitch=0, src_rect=None, extfmt=0):
        """VerifyMediaType + InitMediaType (DX11VideoProcessor.cpp:1569,1742)."""
        r = Rect(*src_rect) if src_rect is not None else None
        return self._check(self._L.mpcvr_set_input(self._ctx, cformat, width, height, pitch,
                                                   C.byref(r) if r is not None else None, extfmt))

    def SetVideoRect(self, rect):
        return self._check(self._L.mpcvr_set_video_rect(self._ctx, C.byref(Rect(*rect))))

    def SetWindowRect(self, rect):
        self._window = tuple(int(v) for v in rect)
        return self._check(self._L.mpcvr_set_window_rect(self._ctx, C.byref(Rect(*rect))))

    def SetRotation(self, value):
        return self._check(self._L.mpcvr_set_rotation(self._ctx, value))

    def SetErrorDiffusionPatience(self, polls):
        """(extension) polls a band of the error-diffusion pass waits for the band above before the pass fails; <= 0: the default."""
        return self._check(self._L.mpcvr_set_error_diffusion_patience(self._ctx, int(polls)))

    def SetFlip(self, value):
        return self._check(self._L.mpcvr_set_flip(self._ctx, int(bool(value))))

    def SetHdrOutput(self, enable, tone_map_type=0, display_max_nits=1000.0):
        """HDR10 display mode (m_bHdrPassthrough / m_bHdrLocalToneMapping, m_iHdrLocalToneMappingType, m_iHdrDisplayMaxNits)."""
        return self._check(self._L.mpcvr_set_hdr_output(self._ctx, int(bool(enable)), int(tone_map_type), float(display_max_nits)))

    def SetHdrMetadata(self, min_mastering, max_mastering, max_cll, max_fall):
        """The values Render() hands to SetHDR10ShaderParams (DX11VideoProcessor.cpp:907-917)."""
        return self._check(self._L.mpcvr_set_hdr_metadata(self._ctx, float(min_mastering), float(max_mastering), float(max_cll), float(max_fall)))

    def SetDoviMetadata(self, md):
        """The Dolby Vision RPU of the next sample(s) (CopySample, DX11VideoProcessor.cpp:2270-2520); None ends DoVi mode."""
        if md is None:
            return self._check(self._L.mpcvr_set_dovi_metadata(self._ctx, None))
        st = md if isinstance(md, DoviMetadata) else DoviMetadata.from_dict(md)
        return self._check(self._L.mpcvr_set_dovi_metadata(self._ctx, C.byref(st)))

    def SetSampleFormat(self, frame_format):
        """m_SampleFormat (DX11VideoProcessor.cpp:2209-2219): 0 progressive, 1 interlaced TFF, 2 interlaced BFF."""
        return self._check(self._L.mpcvr_set_sample_format(self._ctx, int(frame_format)))

    def Configure(self, settings):
        hr = self._check(self._L.mpcvr_configure(self._ctx, C.byref(settings)))
        self.settings = settings.copy()
        return hr

    def SetProcAmpValues(self, brightness=None, contrast=None, hue=None, saturation=None):
        flags = 0
        vals = []
        for bit, v, d in ((1, brightness, 0.0), (2, contrast, 1.0), (4, hue, 0.0), (8, saturation, 1.0)):
            if v is not None:
                flags |= bit
            vals.append(d if v is None else float(v))
        return self._check(self._L.mpcvr_set_procamp(self._ctx, flags, *vals))

    def CopySample(self, data, pitch=None, mem_kind=None):
        """CopySample (DX11VideoProcessor.cpp:2202): host array => upload; CUDA/HIP tensor => zero-copy."""
        if pitch is None:
            pitch = self.GetFrameBytes()[1]
        if mem_kind is None:
            mem_kind = MEM_DEVICE if (hasattr(data, "is_cuda") and data.is_cuda) else MEM_HOST
        self._keep = [data]
        return self._check(self._L.mpcvr_copy_sample(self._ctx, C.c_void_p(_ptr(data)), pitch, mem_kind))

    def Process(self, render_target, rt_pitch, src_rect=None, dst_rect=None, second=False):
        """Process (DX11VideoProcessor.cpp:3285). render_target: device tensor/pointer."""
        s = Rect(*src_rect) if src_rect is not None else None
        d = Rect(*dst_rect) if dst_rect is not None else None
        return self._check(self._L.mpcvr_process(self._ctx, C.c_void_p(_ptr(render_target)), rt_pitch,
                                                 C.byref(s) if s is not None else None,
                                                 C.byref(d) if d is not None else None, int(second)))

    def Render(self, field=1):
        return self._check(self._L.mpcvr_render(self._ctx, field))

    def RenderYuv(self, out_cformat, extfmt=0, field=1):
        """(extension) Render, then the back buffer as NV12 (uint8) or P010 (int16: the code in the top ten bits) planes: returns the
        (y, uv) device tensors of (h, w) and (h / 2, w) components (views of pitch-padded rows where w is no multiple of 4), complete after Synchronize."""
        import torch
        if getattr(self, "_window", None) is not None:
            ww, wh = self._window[2] - self._window[0], self._window[3] - self._window[1]
        else:                                      # (the window was not set through this object: the last Render knows it)
            ww, wh = self.GetBackBuffer()[2:]
        ten = out_cformat == CF_P010
        dt = torch.int16 if ten else torch.uint8
        cols = ww if ten else (ww + 3) & ~3        # a plane's pitch is a multiple of 4 bytes: NV12 rows of w = 2 (mod 4) are padded
        with torch.cuda.device(self.device):
            y = torch.empty((wh, cols), dtype=dt, device="cuda")
            uv = torch.empty((wh // 2, cols), dtype=dt, device="cuda")
        row = cols * (2 if ten else 1)
        self._check(self._L.mpcvr_render_yuv(self._ctx, field, int(out_cformat), int(extfmt), C.c_void_p(y.data_ptr()), row,
                                             C.c_void_p(uv.data_ptr()), row))
        if cols != ww:
            y, uv = y[:, :ww], uv[:, :ww]
        return y, uv

    def _window_size(self):
        if getattr(self, "_window", None) is not None:
            return self._window[2] - self._window[0], self._window[3] - self._window[1]
        return self.GetBackBuffer()[2:]            # (the window was not set through this object: the last Render knows it)

    def RenderTensor(self, dtype=None, layout="chw", channel_order="rgb", scale=(1 / 255,) * 3, bias=(0,) * 3, out=None, field=1):
        """(extension) Render, then the back buffer as a float tensor (mpcvr_render_tensor): value = code * scale + bias per channel of the
        picture (R, G, B), as (3, H, W) for layout "chw" or (H, W, 3) for "hwc", torch.float16 unless `dtype` says float32 / bfloat16.
        `out`: a device tensor of that shape to write into (its dtype and strides are used; the last dim(s) dense); else one is allocated.
        Complete after Synchronize; None when there is no sample."""
        import torch
        if layout not in ("chw", "hwc"):
            raise ValueError("layout 'chw' or 'hwc'")
        ww, wh = self._window_size()
        shape = (3, wh, ww) if layout == "chw" else (wh, ww, 3)
        if out is None:
            out = torch.empty(shape, dtype=dtype or torch.float16, device=f"cuda:{self.device}")
        elif tuple(out.shape) != shape or (dtype is not None and out.dtype != dtype):
            raise ValueError("out must be a %s tensor of shape %s" % (dtype or "float", shape))
        es = out.element_size()
        if layout == "chw":
            if out.stride(2) != 1:
                raise ValueError("the last dim of a (3, H, W) tensor must be dense")
            d = tensor_desc(_tensor_dtype(out.dtype), TENSOR_PLANAR, out.stride(1) * es, out.stride(0) * es, scale, bias, _tensor_order(channel_order))
        else:
            if out.stride(2) != 1 or out.stride(1) != 3:
                raise ValueError("the last two dims of an (H, W, 3) tensor must be dense")
            d = tensor_desc(_tensor_dtype(out.dtype), TENSOR_INTERLEAVED, out.stride(0) * es, 0, scale, bias, _tensor_order(channel_order))
        hr = self._check(self._L.mpcvr_render_tensor(self._ctx, field, C.byref(d), C.c_void_p(out.data_ptr())))
        return None if hr == S_FALSE else out

    def ProcessBatchTensor(self, srcs, out, scale=(1 / 255,) * 3, bias=(0,) * 3, channel_order="rgb"):
        """(extension) ProcessBatch with the frames written as float tensors (mpcvr_process_batch_tensor): `out` is a device tensor of
        (N, 3, H, W) — stride(-1) == 1 — or (N, H, W, 3) — the last two dims dense — with N = len(srcs) and H x W the window; dtype, layout,
        pitches and the per-frame pointers are read from it (any batch stride: a slice of a larger tensor works).  Anything else raises
        before any call.  Complete after Synchronize; GetLastBatchInfo adds tensor_chunks / tensor_lanes."""
        n = len(srcs)
        if n < 1 or out.dim() != 4 or out.shape[0] != n or not out.is_cuda:
            raise ValueError("out must be a device tensor of (len(srcs), 3, H, W) or (len(srcs), H, W, 3)")
        ww, wh = self._window_size()
        es = out.element_size()
        if tuple(out.shape[1:]) == (3, wh, ww) and out.stride(3) == 1:
            d = tensor_desc(_tensor_dtype(out.dtype), TENSOR_PLANAR, out.stride(2) * es, out.stride(1) * es, scale, bias, _tensor_order(channel_order))
        elif tuple(out.shape[1:]) == (wh, ww, 3) and out.stride(3) == 1 and out.stride(2) == 3:
            d = tensor_desc(_tensor_dtype(out.dtype), TENSOR_INTERLEAVED, out.stride(1) * es, 0, scale, bias, _tensor_order(channel_order))
        else:
            raise ValueError("out of shape %s / strides %s is neither (N, 3, %d, %d) with a dense last dim nor (N, %d, %d, 3) with the last two dims dense"
                             % (tuple(out.shape), out.stride(), wh, ww, wh, ww))
        arr = C.c_void_p * n
        keep = (arr(*[_ptr(s) for s in srcs]), arr(*[out.data_ptr() + i * out.stride(0) * es for i in range(n)]), d, (srcs, out))
        self._keep = keep
        return self._check(self._L.mpcvr_process_batch_tensor(self._ctx, n, keep[0], C.byref(d), keep[1]))

    def RenderLut3d(self, lut, n, dst_fmt=None, out=None, out_pitch=None, field=1):
        """(extension) Render, then the back buffer through the 3D LUT at `lut` (device tensor or address: n^3 entries of 8 bytes,
        plan_lut3d_entries) into a target of dst_fmt (OUT_BGRA8 / OUT_RGB10A2; None: the context's output_format) (mpcvr_render_lut3d).
        `out`: a device tensor or address of window_h rows of out_pitch bytes (None: 4 * window_w); else a (H, W, 4) uint8 tensor is
        allocated.  Returns the target, complete after Synchronize; None when there is no sample (S_FALSE).  The back buffer stays the
        plain frame."""
        import torch
        ww, wh = self._window_size()
        if dst_fmt is None:
            dst_fmt = self.settings.output_format
        if out is None:
            out = torch.empty((wh, ww, 4), dtype=torch.uint8, device="cuda")
            out_pitch = ww * 4
        elif out_pitch is None:
            out_pitch = ww * 4
        self._keep = (lut, out)
        hr = self._check(self._L.mpcvr_render_lut3d(self._ctx, field, C.c_void_p(_ptr(lut)), int(n), C.c_void_p(_ptr(out)), int(out_pitch), int(dst_fmt)))
        return out if hr == S_OK else None

    def ProcessBatchLut3d(self, srcs, lut, n, dsts, dst_pitch, dst_fmt=None):
        """(extension) ProcessBatch with every frame taken through the 3D LUT at `lut` on its way to its render target
        (mpcvr_process_batch_lut3d): dsts[i] are device tensors or addresses of window_h rows of dst_pitch bytes, of dst_fmt (None: the
        context's output_format).  One k_lut3d launch per chunk; complete after Synchronize.  GetLastBatchInfo adds lut3d_chunks /
        lut3d_lanes / lut3d_table."""
        m = len(srcs)
        assert m == len(dsts) and m > 0
        if dst_fmt is None:
            dst_fmt = self.settings.output_format
        arr = C.c_void_p * m
        keep = (arr(*[_ptr(s) for s in srcs]), arr(*[_ptr(d) for d in dsts]), (srcs, dsts, lut))
        self._keep = keep
        return self._check(self._L.mpcvr_process_batch_lut3d(self._ctx, m, keep[0], C.c_void_p(_ptr(lut)), int(n), keep[1], int(dst_pitch), int(dst_fmt)))

    def RenderDeband(self, params=None, seed=0, dst_fmt=None, out=None, out_pitch=None, field=1):
        """(extension) Render, then the back buffer through the deband pass (params: a DebandParams, a dict of its fields or None for
        deband_params_default of the context's output_format) into a target of dst_fmt (OUT_BGRA8 / OUT_RGB10A2; None: the context's
        output_format) (mpcvr_render_deband).  `out`: a device tensor or address of window_h rows of out_pitch bytes (None: 4 * window_w);
        else a (H, W, 4) uint8 tensor is allocated.  Returns the target, complete after Synchronize; None when there is no sample
        (S_FALSE).  The back buffer stays the plain frame."""
        import torch
        ww, wh = self._window_size()
        if dst_fmt is None:
            dst_fmt = self.settings.output_format
        p = deband_params_default(self.settings.output_format) if params is None else _deband_params(params)
        if out is None:
            out = torch.empty((wh, ww, 4), dtype=torch.uint8, device="cuda")
            out_pitch = ww * 4
        elif out_pitch is None:
            out_pitch = ww * 4
        self._keep = (out,)
        hr = self._check(self._L.mpcvr_render_deband(self._ctx, field, C.byref(p), int(seed) & 0xffffffff, C.c_void_p(_ptr(out)), int(out_pitch), int(dst_fmt)))
        return out if hr == S_OK else None

    def ProcessBatchDeband(self, srcs, params, seed, dsts, dst_pitch, dst_fmt=None):
        """(extension) ProcessBatch with every frame taken through the deband pass on its way to its render target, frame i with seed + i
        (mpcvr_process_batch_deband): dsts[i] are device tensors or addresses of window_h rows of dst_pitch bytes, of dst_fmt (None: the
        context's output_format).  One k_deband launch per chunk; complete after Synchronize.  GetLastBatchInfo adds deband_chunks /
        deband_lanes / deband_taps."""
        m = len(srcs)
        assert m == len(dsts) and m > 0
        if dst_fmt is None:
            dst_fmt = self.settings.output_format
        p = deband_params_default(self.settings.output_format) if params is None else _deband_params(params)
        arr = C.c_void_p * m
        keep = (arr(*[_ptr(s) for s in srcs]), arr(*[_ptr(d) for d in dsts]), (srcs, dsts))
        self._keep = keep
        return self._check(self._L.mpcvr_process_batch_deband(self._ctx, m, keep[0], C.byref(p), int(seed) & 0xffffffff, keep[1], int(dst_pitch), int(dst_fmt)))

    def RenderSharpen(self, params=None, seed=0, dst_fmt=None, out=None, out_pitch=None, field=1):
        """(extension) Render, then the back buffer through the sharpen pass (params: a SharpenParams, a dict of its fields or None for
        sharpen_params_default of the context's output_format) into a target of dst_fmt (OUT_BGRA8 / OUT_RGB10A2; None: the context's
        output_format) (mpcvr_render_sharpen).  `out`: a device tensor or address of window_h rows of out_pitch bytes (None: 4 * window_w);
        else a (H, W, 4) uint8 tensor is allocated.  Returns the target, complete after Synchronize; None when there is no sample
        (S_FALSE).  The back buffer stays the plain frame."""
        import torch
        ww, wh = self._window_size()
        if dst_fmt is None:
            dst_fmt = self.settings.output_format
        p = sharpen_params_default(self.settings.output_format) if params is None else _sharpen_params(params)
        if out is None:
            out = torch.empty((wh, ww, 4), dtype=torch.uint8, device="cuda")
            out_pitch = ww * 4
        elif out_pitch is None:
            out_pitch = ww * 4
        self._keep = (out,)
        hr = self._check(self._L.mpcvr_render_sharpen(self._ctx, field, C.byref(p), int(seed) & 0xffffffff, C.c_void_p(_ptr(out)), int(out_pitch), int(dst_fmt)))
        return out if hr == S_OK else None

    def ProcessBatchSharpen(self, srcs, params, seed, dsts, dst_pitch, dst_fmt=None):
        """(extension) ProcessBatch with every frame taken through the sharpen pass on its way to its render target, frame i with seed + i
        (mpcvr_process_batch_sharpen): dsts[i] are device tensors or addresses of window_h rows of dst_pitch bytes, of dst_fmt (None: the
        context's output_format).  One k_sharpen launch per chunk; complete after Synchronize.  GetLastBatchInfo adds sharpen_chunks /
        sharpen_lanes."""
        m = len(srcs)
        assert m == len(dsts) and m > 0
        if dst_fmt is None:
            dst_fmt = self.settings.output_format
        p = sharpen_params_default(self.settings.output_format) if params is None else _sharpen_params(params)
        arr = C.c_void_p * m
        keep = (arr(*[_ptr(s) for s in srcs]), arr(*[_ptr(d) for d in dsts]), (srcs, dsts))
        self._keep = keep
        return self._check(self._L.mpcvr_process_batch_sharpen(self._ctx, m, keep[0], C.byref(p), int(seed) & 0xffffffff, keep[1], int(dst_pitch), int(dst_fmt)))

    def MeasureBackBuffer(self, hist=None):
        """(extension) The histogram of max(R, G, B) of the frame the last Render / RenderYuv left, over video rect ∩ window
        (mpcvr_measure_backbuffer): a device tensor of 1024 int32 words holding the uint32 counts (allocated when `hist` is None), complete
        after Synchronize; None when nothing has been rendered yet."""
        import torch
        if hist is None:
            hist = torch.empty(HIST_BINS, dtype=torch.int32, device=f"cuda:{self.device}")
        hr = self._check(self._L.mpcvr_measure_backbuffer(self._ctx, C.c_void_p(_ptr(hist))))
        return None if hr == S_FALSE else hist

    def GetBackBuffer(self):
        p, pitch, w, h = C.c_void_p(), C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._L.mpcvr_get_backbuffer(self._ctx, C.byref(p), C.byref(pitch), C.byref(w), C.byref(h)))
        return p.value, pitch.value, w.value, h.value

    def GetCurentImage(self):
        """GetCurentImage (DX11VideoProcessor.cpp:3493): BGRX snapshot at source-rect size -> numpy."""
        import numpy as np
        size = C.c_size_t(0)
        self._check(self._L.mpcvr_get_current_image(self._ctx, None, C.byref(size)))
        buf = np.empty(size.value, dtype=np.uint8)
        self._check(self._L.mpcvr_get_current_image(self._ctx, C.c_void_p(buf.ctypes.data), C.byref(size)))
        return buf

    def GetDisplayedImage(self, deep_color=False):
        """GetDisplayedImage (DX11VideoProcessor.cpp:3610): the back buffer of the last Render as DIB pixels -> (numpy bytes, width, height, bits)."""
        import numpy as np
        size, w, h, bits = C.c_size_t(0), C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._L.mpcvr_get_displayed_image(self._ctx, None, C.byref(size), int(deep_color), C.byref(w), C.byref(h), C.byref(bits)))
        buf = np.empty(size.value, dtype=np.uint8)
        self._check(self._L.mpcvr_get_displayed_image(self._ctx, C.c_void_p(buf.ctypes.data), C.byref(size), int(deep_color), C.byref(w), C.byref(h), C.byref(bits)))
        return buf, w.value, h.value, bits.value

    def CopySampleTensor(self, t, scale=(255.0,) * 3, bias=(0,) * 3, channel_order="rgb"):
        """(extension) A model's float tensor as the current sample of a GBRP8 / GBRP10 / GBRP16 input (mpcvr_copy_sample_tensor): code =
        round(value * scale + bias) per channel of the picture (R, G, B), clamped to the format.  `t` is a device tensor of (3, H, W) with a
        dense last dim or (H, W, 3) with the last two dims dense, float32 / float16 / bfloat16; dtype, layout and pitches are read off it,
        so a slice works.  The pass runs on the context stream; `t` is free in that stream's order behind the call."""
        d, w, h = _frame_tensor_desc(t, scale, bias, channel_order)
        if not t.is_cuda:
            raise ValueError("a device tensor")
        self._keep = (t, d)
        return self._check(self._L.mpcvr_copy_sample_tensor(self._ctx, C.c_void_p(t.data_ptr()), C.byref(d)))

    def ProcessBatchFromTensors(self, ts, dsts, rt_pitch, scale=(255.0,) * 3, bias=(0,) * 3, channel_order="rgb"):
        """(extension) ProcessBatch with float tensors as the samples (mpcvr_process_batch_from_tensors): `ts` is a device tensor of
        (N, 3, H, W) or (N, H, W, 3), or a sequence of frames of one shape, dtype and strides (_frame_tensor_desc); dsts[i] the render
        targets.  One k_sample_from_tensor launch per chunk in front of the chunk's batch; GetLastBatchInfo adds sample_chunks."""
        frames = [ts[i] for i in range(len(ts))]
        n = len(frames)
        if n < 1 or n != len(dsts):
            raise ValueError("as many tensors as render targets, at least one")
        d, w, h = _frame_tensor_desc(frames[0], scale, bias, channel_order)
        for t in frames:
            if not t.is_cuda or t.dtype != frames[0].dtype or tuple(t.shape) != tuple(frames[0].shape) or t.stride() != frames[0].stride():
                raise ValueError("every frame a device tensor of one dtype, shape and strides")
        arr = C.c_void_p * n
        keep = (arr(*[t.data_ptr() for t in frames]), arr(*[_ptr(x) for x in dsts]), d, (ts, dsts))
        self._keep = keep
        return self._check(self._L.mpcvr_process_batch_from_tensors(self._ctx, n, keep[0], C.byref(d), keep[1], int(rt_pitch)))

    def CopySampleFields(self, prev, cur, nxt, field_order, field, mode=DEINT_ADAPTIVE_EXT):
        """(extension) Field `field` (0 the first, 1 the second) of the interlaced device sample `cur`, deinterlaced between `prev` and
        `nxt` (pass `cur` again at a stream's ends), as the current sample (mpcvr_copy_sample_fields); field_order FIELD_ORDER_TFF / BFF.
        The pass runs on the context stream; the samples are free in that stream's order behind the call."""
        self._keep = (prev, cur, nxt)
        return self._check(self._L.mpcvr_copy_sample_fields(self._ctx, C.c_void_p(_ptr(prev)), C.c_void_p(_ptr(cur)), C.c_void_p(_ptr(nxt)),
                                                            int(field_order), int(field), int(mode)))

    def ProcessBatchDeint(self, frames, dsts, rt_pitch, field_order, fields_per_frame=2, mode=DEINT_ADAPTIVE_EXT):
        """(extension) ProcessBatch at field rate (mpcvr_process_batch_deint): `frames` are n + 2 interlaced device samples, the n interior
        ones deinterlaced with their neighbours; dsts the n * fields_per_frame render targets, target (i - 1) * fields_per_frame + f showing
        field f of frame i.  One pass per chunk in front of the chunk's batch; GetLastBatchInfo adds deint_chunks."""
        n = len(frames) - 2
        if n < 1 or len(dsts) != n * fields_per_frame:
            raise ValueError("n + 2 samples for n * fields_per_frame render targets, n at least one")
        keep = ((C.c_void_p * (n + 2))(*[_ptr(x) for x in frames]), (C.c_void_p * len(dsts))(*[_ptr(x) for x in dsts]), (frames, dsts))
        self._keep = keep
        return self._check(self._L.mpcvr_process_batch_deint(self._ctx, n, keep[0], int(field_order), int(fields_per_frame), int(mode), keep[1], int(rt_pitch)))

    def ProcessBatch(self, srcs, dsts, rt_pitch):
        if isinstance(srcs, PreparedBatch):          # pointer arrays built once (PrepareBatch): nothing per call but the C call
            return self._check(self._L.mpcvr_process_batch(self._ctx, srcs.n, srcs.sa, srcs.da, rt_pitch))
        b = self.PrepareBatch(srcs, dsts)
        self._keep = b
        return self._check(self._L.mpcvr_process_batch(self._ctx, b.n, b.sa, b.da, rt_pitch))

    def SetBatchYuvBudget(self, nbytes):
        """(extension) The bytes one context-owned RGB surface of ProcessBatchYuv may take (0: the default)."""
        return self._check(self._L.mpcvr_set_batch_yuv_budget(self._ctx, int(nbytes)))

    def ProcessBatchYuv(self, srcs, out_cformat, extfmt, y_planes, y_pitch, uv_planes, uv_pitch):
        """(extension) ProcessBatch with the frames written as NV12 / P010 planes (mpcvr_process_batch_yuv): y_planes[i] / uv_planes[i] are
        device tensors or addresses, one pitch each for all frames; complete after Synchronize.  GetLastBatchInfo adds yuv_chunks / yuv_lanes."""
        n = len(srcs)
        assert n == len(y_planes) == len(uv_planes) and n > 0
        arr = C.c_void_p * n
        keep = (arr(*[_ptr(s) for s in srcs]), arr(*[_ptr(p) for p in y_planes]), arr(*[_ptr(p) for p in uv_planes]), (srcs, y_planes, uv_planes))
        self._keep = keep
        return self._check(self._L.mpcvr_process_batch_yuv(self._ctx, n, keep[0], int(out_cformat), int(extfmt), keep[1], int(y_pitch), keep[2], int(uv_pitch)))

    def ProcessBatchYuvStats(self, srcs, out_cformat, extfmt, y_planes, y_pitch, uv_planes, uv_pitch, hist):
        """(extension) ProcessBatchYuv plus one histogram of max(R, G, B) per frame over video rect ∩ window (mpcvr_process_batch_yuv_stats):
        `hist` is a device tensor or address of len(srcs) rows of 1024 uint32 words; complete after Synchronize."""
        n = len(srcs)
        assert n == len(y_planes) == len(uv_planes) and n > 0
        arr = C.c_void_p * n
        keep = (arr(*[_ptr(s) for s in srcs]), arr(*[_ptr(p) for p in y_planes]), arr(*[_ptr(p) for p in uv_planes]), (srcs, y_planes, uv_planes, hist))
        self._keep = keep
        return self._check(self._L.mpcvr_process_batch_yuv_stats(self._ctx, n, keep[0], int(out_cformat), int(extfmt), keep[1], int(y_pitch), keep[2],
                                                                 int(uv_pitch), C.c_void_p(_ptr(hist))))

    def ProcessBatchDovi(self, srcs, dsts, rt_pitch, rpus):
        """ProcessBatch with one Dolby Vision RPU per frame (mpcvr_process_batch_dovi): rpus[i] is a DoviMetadata or the dict
        DoviMetadata.from_dict takes."""
        b = srcs if isinstance(srcs, PreparedBatch) else self.PrepareBatch(srcs, dsts)
        self._keep = b
        assert len(rpus) == b.n
        arr = (DoviMetadata * b.n)(*[m if isinstance(m, DoviMetadata) else DoviMetadata.from_dict(m) for m in rpus])
        return self._check(self._L.mpcvr_process_batch_dovi(self._ctx, b.n, b.sa, b.da, rt_pitch, arr))

    @staticmethod
    def PrepareBatch(srcs, dsts):
        """The pointer arrays of a batch, for callers that submit the same buffers again and again (a ring): building them
        costs ~2 us of interpreter time per frame, more than a 1080p frame costs the GPU."""
        n = len(srcs)
        assert n == len(dsts) and n > 0
        return PreparedBatch(n, (C.c_void_p * n)(*[_ptr(s) for s in srcs]), (C.c_void_p * n)(*[_ptr(d) for d in dsts]), (srcs, dsts))

    def Flush(self):
        return self._check(self._L.mpcvr_flush(self._ctx))

    def Reset(self):
        return self._check(self._L.mpcvr_reset(self._ctx))

    # -- introspection ---------------------------------------------------------------------------
    def GetParamBlob(self):
        size = C.c_size_t(0)
        self._check(self._L.mpcvr_get_param_blob(self._ctx, None, C.byref(size)))
        buf = (C.c_uint8 * size.value)()
        self._check(self._L.mpcvr_get_param_blob(self._ctx, buf, C.byref(size)))
        return bytes(buf)

    def GetFusedTables(self):
        """The exact-2x kernel's baked table image of the current plan (include/mpcvr.h: mpcvr_get_fused_tables)."""
        size = C.c_size_t(0)
        self._check(self._L.mpcvr_get_fused_tables(self._ctx, None, C.byref(size)))
        buf = (C.c_uint8 * size.value)()
        self._check(self._L.mpcvr_get_fused_tables(self._ctx, buf, C.byref(size)))
        return bytes(buf)

    def SetParamBlob(self, blob):
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        return self._check(self._L.mpcvr_set_param_blob(self._ctx, buf, len(blob)))

    def GetColorMatrix(self):
        out = (C.c_float * 12)()
        self._check(self._L.mpcvr_get_color_matrix(self._ctx, out))
        return list(out)

    def GetExtFmt(self):
        v = C.c_uint32()
        self._check(self._L.mpcvr_get_extfmt(self._ctx, C.byref(v)))
        return v.value

    def GetFrameBytes(self):
        n, p = C.c_size_t(), C.c_int32()
        self._check(self._L.mpcvr_get_frame_bytes(self._ctx, C.byref(n), C.byref(p)))
        return n.value, p.value

    def GetVPInfo(self):
        buf = C.create_string_buffer(256)
        self._check(self._L.mpcvr_get_path_info(self._ctx, buf, 256))
        return buf.value.decode()

    def GetLastBatchInfo(self):
        """'frames=<n>;launches=<kernel launches>;lane=<0 | 1: the batch ran on that lane beside its predecessor, -1: on the context stream>;waits=<frames / batches still in flight on other lanes, into memory this batch's targets overlap, that it was ordered behind>[;dovi_runs=...]' of the last ProcessBatch / ProcessBatchDovi / ProcessBatchYuv call, as a dict; behind a ProcessBatchYuv also yuv_chunks and yuv_lanes (the lane of each chunk), behind a ProcessBatchTensor tensor_chunks and tensor_lanes, behind a ProcessBatchFromTensors sample_chunks, behind a ProcessBatchLut3d lut3d_chunks, lut3d_lanes and lut3d_table, behind a ProcessBatchDeband deband_chunks, deband_lanes and deband_taps, behind a ProcessBatchSharpen sharpen_chunks and sharpen_lanes."""
        buf = C.create_string_buffer(512)
        self._check(self._L.mpcvr_get_last_batch_info(self._ctx, buf, 512))
        d = dict(kv.split("=", 1) for kv in buf.value.decode().split(";"))
        out = dict(frames=int(d["frames"]), launches=int(d["launches"]), dovi_runs=d.get("dovi_runs", ""), lane=int(d.get("lane", -1)), waits=int(d.get("waits", 0)), uploads=int(d.get("uploads", -1)))
        if "yuv_chunks" in d:        # (only behind a ProcessBatchYuv: the lane of each chunk, -1 = the context stream)
            out.update(yuv_chunks=int(d["yuv_chunks"]), yuv_lanes=[int(x) for x in d["yuv_lanes"].split(",") if x])
        if "tensor_chunks" in d:     # (only behind a ProcessBatchTensor, likewise)
            out.update(tensor_chunks=int(d["tensor_chunks"]), tensor_lanes=[int(x) for x in d["tensor_lanes"].split(",") if x])
        if "sample_chunks" in d:     # (only behind a ProcessBatchFromTensors)
            out.update(sample_chunks=int(d["sample_chunks"]))
        if "deint_chunks" in d:      # (only behind a ProcessBatchDeint)
            out.update(deint_chunks=int(d["deint_chunks"]))
        if "lut3d_chunks" in d:      # (only behind a ProcessBatchLut3d: the lane of each chunk, and where the pass read the table from)
            out.update(lut3d_chunks=int(d["lut3d_chunks"]), lut3d_lanes=[int(x) for x in d["lut3d_lanes"].split(",") if x], lut3d_table=d.get("lut3d_table", ""))
        if "deband_chunks" in d:     # (only behind a ProcessBatchDeband: the lane of each chunk, and where the pass read its taps from)
            out.update(deband_chunks=int(d["deband_chunks"]), deband_lanes=[int(x) for x in d["deband_lanes"].split(",") if x], deband_taps=d.get("deband_taps", ""))
        if "sharpen_chunks" in d:    # (only behind a ProcessBatchSharpen: the lane of each chunk)
            out.update(sharpen_chunks=int(d["sharpen_chunks"]), sharpen_lanes=[int(x) for x in d["sharpen_lanes"].split(",") if x])
        return out

    def GetUp2xForm(self):
        """'bp' / 'generic': the form of the context's last exact-2x fused launch since its last batch call began (";up2x=" of
        mpcvr_get_last_batch_info: the bi-planar twin k_fused_up2x_bp, or k_fused_up2x); None when it has launched none."""
        buf = C.create_string_buffer(512)
        self._check(self._L.mpcvr_get_last_batch_info(self._ctx, buf, 512))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(";")).get("up2x")

    def GetLastProcessMs(self):
        ms = C.c_float()
        self._check(self._L.mpcvr_get_last_process_ms(self._ctx, C.byref(ms)))
        return ms.value

    def GetLastTimings(self):
        """{copy_host_ms, upload_ms, process_ms, readback_ms} (FrameStats.h:145-173); -1 = not timed yet."""
        v = [C.c_float(-1.0) for _ in range(4)]
        self._check(self._L.mpcvr_get_last_timings(self._ctx, *(C.byref(x) for x in v)))
        return dict(zip(("copy_host_ms", "upload_ms", "process_ms", "readback_ms"), (x.value for x in v)))
