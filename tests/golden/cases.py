"""Named parity cases shared by the CPU golden-hash test and the GPU parity tests.

Each case = BASELINE.json config (at a size the oracle finishes in well under a second) or an edge
case of the path (ragged sizes, crops, clipping, every scaler / chroma mode / format family).
"""
import numpy as np

from videorenderer_amd import synth

# DXVA2_ExtendedFormat field values (Helper.cpp:1215-1223)
MPEG1, MPEG2, COSITED = 1, 5, 7
FULL, TV = 1, 2
M709, M601, M240, M2020, MYCGCO = 1, 2, 3, 4, 7
P709, P2020 = 2, 9
T22, T709, TSRGB, T26, TPQ, THLG = 4, 5, 7, 14, 15, 16


def ext(chroma=0, rng=0, matrix=0, prim=0, trc=0):
    return ((chroma & 0xf) << 8) | ((rng & 7) << 12) | ((matrix & 7) << 15) | ((prim & 0x1f) << 22) | ((trc & 0x1f) << 27)


HDR10 = ext(MPEG2, TV, M2020, P2020, TPQ)
HLG = ext(MPEG2, TV, M2020, P2020, THLG)

# name -> dict(cformat, w, h, kind, seed, dst=(w2,h2), + optional: exfmt, settings overrides, src_rect,
#              window=(w,h), offset=(x,y), procamp=(b,c,h,s), pitch)
GOLDEN_CASES = {
    # ---- BASELINE.json configs, reduced size ----
    "c1_nv12_bt709_passthrough": dict(cformat=1, w=128, h=72, kind="structure", seed=1, dst=(128, 72), exfmt=ext(matrix=M709)),
    "c2_yuv420p10_catmull_2x": dict(cformat=20, w=96, h=54, kind="structure", seed=2, dst=(192, 108), exfmt=ext(matrix=M709), iUpscaling=2),
    "c3_p010_lanczos3_2x": dict(cformat=2, w=128, h=72, kind="structure", seed=3, dst=(256, 144), exfmt=ext(matrix=M709), iUpscaling=4),
    "c3hdr_p010_pq_lanczos3_2x": dict(cformat=2, w=128, h=72, kind="hdr", seed=4, dst=(256, 144), exfmt=HDR10, iUpscaling=4),
    "c4_p010_pq_mitchell_2x": dict(cformat=2, w=128, h=72, kind="hdr", seed=5, dst=(256, 144), exfmt=HDR10, iUpscaling=1),
    "c5_p010_hlg_lanczos3_2x": dict(cformat=2, w=128, h=72, kind="hdr", seed=6, dst=(256, 144), exfmt=HLG, iUpscaling=4),
    # exact 2x with the combinations no BASELINE configuration hits (both tap engines run every exact-2x case): a window offset that is
    # not a multiple of 4 (the generic epilogue behind a PQ table tail), HLG behind a 4-tap filter, the literal PQ chain (MPCVR_FLAG_NO_LUT)
    "x2_p010_pq_mitchell_offset": dict(cformat=2, w=64, h=40, kind="hdr", seed=501, dst=(128, 80), exfmt=HDR10, iUpscaling=1, window=(140, 88), offset=(3, 4)),
    "x2_p010_hlg_mitchell": dict(cformat=2, w=64, h=40, kind="hdr", seed=502, dst=(128, 80), exfmt=HLG, iUpscaling=1),
    "x2_p010_pq_lanczos3_literal_tail": dict(cformat=2, w=64, h=40, kind="hdr", seed=503, dst=(128, 80), exfmt=HDR10, iUpscaling=4, flags=4),
    # ---- noise through the headline pipeline (worst case for rounding) ----
    "noise_p010_pq_lanczos3_2x": dict(cformat=2, w=248, h=40, kind="noise", seed=7, dst=(496, 80), exfmt=HDR10, iUpscaling=4),
    "noise_p010_sdr_lanczos2_2x": dict(cformat=2, w=136, h=24, kind="noise", seed=8, dst=(272, 48), exfmt=ext(matrix=M709), iUpscaling=3),
    "noise_nv12_catmull_2x": dict(cformat=1, w=64, h=40, kind="noise", seed=9, dst=(128, 80), exfmt=ext(matrix=M709), iUpscaling=2),
    # ---- scalers ----
    "up_1p5x_lanczos3": dict(cformat=2, w=64, h=48, kind="structure", seed=10, dst=(96, 72), iUpscaling=4),
    "up_3x_mitchell_fixedflag": dict(cformat=2, w=40, h=24, kind="noise", seed=11, dst=(120, 72), iUpscaling=4, flags=1),
    "mild_down_uses_upscaler": dict(cformat=1, w=96, h=64, kind="structure", seed=12, dst=(60, 40), iUpscaling=2),
    "down_hamming_3x": dict(cformat=2, w=192, h=96, kind="structure", seed=13, dst=(64, 32), iDownscaling=2),
    "down_lanczos_2p5x": dict(cformat=2, w=160, h=100, kind="noise", seed=14, dst=(64, 40), iDownscaling=5),
    "down_box_bilinear_mix": dict(cformat=1, w=128, h=96, kind="noise", seed=15, dst=(32, 40), iDownscaling=0, bInterpolateAt50pct=0),
    "down_bicubic_sharp": dict(cformat=1, w=128, h=96, kind="structure", seed=16, dst=(48, 36), iDownscaling=4),
    "down_bilinear_x_up_y": dict(cformat=2, w=128, h=32, kind="structure", seed=17, dst=(40, 64), iDownscaling=1, iUpscaling=1),
    "nearest_2x": dict(cformat=1, w=32, h=24, kind="noise", seed=18, dst=(64, 48), iUpscaling=0),
    "x_only_resize": dict(cformat=2, w=48, h=32, kind="structure", seed=19, dst=(96, 32), iUpscaling=2),
    "y_only_resize": dict(cformat=2, w=48, h=32, kind="structure", seed=20, dst=(48, 80), iUpscaling=3),
    # ---- Jinc2m: one 2-D draw for both axes (ps_resize_onepass_jinc2.hlsl, :2921) ----
    "jinc2_p010_2x_dither": dict(cformat=2, w=64, h=32, kind="structure", seed=130, dst=(128, 64), iUpscaling=5),
    "jinc2_nv12_noise_1p5x": dict(cformat=1, w=64, h=40, kind="noise", seed=131, dst=(96, 60), iUpscaling=5),
    "jinc2_x_with_hamming_down_y": dict(cformat=1, w=48, h=96, kind="structure", seed=132, dst=(96, 30), iUpscaling=5, iDownscaling=2),
    "jinc2_y_only": dict(cformat=2, w=64, h=32, kind="noise", seed=133, dst=(64, 80), iUpscaling=5),
    "jinc2_rot90_pq": dict(cformat=2, w=48, h=32, kind="hdr", seed=134, dst=(64, 96), iUpscaling=5, rotation=90, exfmt=HDR10),
    # ---- HDR output: PQ passthrough, HLG -> PQ, ps_hdr10_tonemap post-scale step (N2) ----
    "hdrout_pq_passthrough_2x": dict(cformat=2, w=64, h=32, kind="hdr", seed=140, dst=(128, 64), exfmt=HDR10, iUpscaling=4, output_format=1, hdr_output=1),
    "hdrout_hlg_to_pq": dict(cformat=2, w=64, h=32, kind="hdr", seed=141, dst=(64, 32), exfmt=HLG, output_format=1, hdr_output=1),
    "hdrout_tm1_aces_2x": dict(cformat=2, w=64, h=32, kind="hdr", seed=142, dst=(128, 64), exfmt=HDR10, iUpscaling=4, output_format=1,
                               hdr_output=1, hdr_tonemap=1, hdr_display=600.0, hdr_meta=(0.005, 1000.0, 1000.0, 400.0)),
    "hdrout_tm2_reinhard": dict(cformat=2, w=64, h=32, kind="noise", seed=143, dst=(96, 48), exfmt=HDR10, iUpscaling=2, output_format=1,
                                hdr_output=1, hdr_tonemap=2, hdr_display=800.0, hdr_meta=(0.0, 4000.0, 2000.0, 300.0)),
    "hdrout_tm3_habel_same_size": dict(cformat=2, w=64, h=32, kind="hdr", seed=144, dst=(64, 32), exfmt=HDR10, output_format=1,
                                       hdr_output=1, hdr_tonemap=3, hdr_display=1000.0, hdr_meta=(0.01, 1000.0, 0.0, 0.0)),
    "hdrout_tm4_moebius_bgra8_dither": dict(cformat=2, w=64, h=32, kind="hdr", seed=145, dst=(128, 64), exfmt=HDR10, iUpscaling=1,
                                            hdr_output=1, hdr_tonemap=4, hdr_display=500.0, hdr_meta=(0.005, 1000.0, 1200.0, 200.0)),
    "hdrout_tm5_bt2390": dict(cformat=2, w=64, h=32, kind="hdr", seed=146, dst=(128, 64), exfmt=HDR10, iUpscaling=4, output_format=1,
                              hdr_output=1, hdr_tonemap=5, hdr_display=400.0, hdr_meta=(0.005, 1000.0, 1000.0, 400.0)),
    "hdrout_tm6_st2094_hlg_fp16": dict(cformat=2, w=64, h=32, kind="hdr", seed=147, dst=(96, 48), exfmt=HLG, iUpscaling=2, output_format=1, iTexFormat=16,
                                       hdr_output=1, hdr_tonemap=6, hdr_display=600.0, hdr_meta=(0.005, 1000.0, 1000.0, 180.0)),
    "hdrout_tm5_display_brighter_than_content": dict(cformat=2, w=64, h=32, kind="noise", seed=148, dst=(64, 32), exfmt=HDR10, output_format=1,
                                                     hdr_output=1, hdr_tonemap=5, hdr_display=2000.0, hdr_meta=(0.005, 1000.0, 1000.0, 400.0)),
    # ---- Dolby Vision (N2): reshaping curves, ycc_to_rgb matrix, PQ -> LMS -> PQ, level-1/2/3 metadata ----
    "dovi_poly_sdr": dict(cformat=20, w=96, h=54, kind="hdr", seed=150, dst=(96, 54), exfmt=ext(MPEG2, TV), dovi=dict(kind="poly")),
    "dovi_poly_sdr_l2_between_2x": dict(cformat=2, w=64, h=32, kind="hdr", seed=151, dst=(128, 64), iUpscaling=4, exfmt=ext(MPEG2, TV),
                                        dovi=dict(kind="poly", l2=(100, 600, 1000)), hdr_display=400.0),
    "dovi_mmr_sdr_l2_brighter": dict(cformat=20, w=64, h=40, kind="structure", seed=152, dst=(96, 60), iUpscaling=2,
                                     dovi=dict(kind="mmr", l2=(100,)), hdr_display=1000.0),
    "dovi_mixed_noise_catmull_chroma": dict(cformat=2, w=64, h=32, kind="noise", seed=153, dst=(64, 32), iChromaScaling=2,
                                            dovi=dict(kind="mixed", l2=(600, 2000)), hdr_display=300.0),
    "dovi_identity_hlg_tagged": dict(cformat=2, w=64, h=32, kind="hdr", seed=154, dst=(64, 32), exfmt=HLG, dovi=dict(kind="identity")),
    "dovi_procamp_down": dict(cformat=20, w=128, h=64, kind="structure", seed=155, dst=(48, 24), iDownscaling=2,
                              procamp=(12.0, 1.1, 30.0, 1.4), dovi=dict(kind="poly")),
    "dovi_hdrout_passthrough": dict(cformat=2, w=64, h=32, kind="hdr", seed=156, dst=(128, 64), iUpscaling=4, output_format=1, hdr_output=1,
                                    dovi=dict(kind="mmr")),
    "dovi_hdrout_bt2020_gamma_tag": dict(cformat=20, w=64, h=32, kind="hdr", seed=157, dst=(64, 32), output_format=1, hdr_output=1,
                                         exfmt=ext(MPEG2, TV, M2020, P2020, T709), dovi=dict(kind="poly")),
    "dovi_hdrout_tm5_l1_l3_l2": dict(cformat=2, w=64, h=32, kind="hdr", seed=158, dst=(96, 48), iUpscaling=2, output_format=1,
                                     hdr_output=1, hdr_tonemap=5, hdr_display=1000.0, dovi=dict(kind="mmr", l1=True, l3=True, l2=(600, 2000))),
    "dovi_hdrout_tm3_hdr10_meta": dict(cformat=20, w=64, h=32, kind="noise", seed=159, dst=(64, 32), output_format=1,
                                       hdr_output=1, hdr_tonemap=3, hdr_display=600.0, hdr_meta=(0.005, 1000.0, 1000.0, 400.0),
                                       dovi=dict(kind="poly", l2=(100, 1000))),
    # ---- geometry ----
    "crop_offset_letterbox": dict(cformat=2, w=96, h=64, kind="structure", seed=21, src_rect=(16, 8, 80, 56), dst=(128, 96),
                                  window=(200, 150), offset=(36, 27), iUpscaling=4),
    "clipped_by_window": dict(cformat=1, w=64, h=48, kind="structure", seed=22, dst=(128, 96), window=(90, 70), offset=(-20, -13), iUpscaling=2),
    "same_size_with_offset_dither": dict(cformat=2, w=64, h=32, kind="noise", seed=23, dst=(64, 32), window=(100, 60), offset=(5, 9)),
    "exact_2x_at_unaligned_offset": dict(cformat=2, w=64, h=32, kind="noise", seed=150, dst=(128, 64), window=(140, 80), offset=(5, 3),
                                         iUpscaling=4, exfmt=HDR10),
    "exact_2x_at_aligned_offset": dict(cformat=2, w=64, h=32, kind="noise", seed=151, dst=(128, 64), window=(140, 80), offset=(8, 3),
                                       iUpscaling=4, exfmt=HDR10),
    "tiny_8x8": dict(cformat=2, w=8, h=8, kind="noise", seed=24, dst=(16, 16), iUpscaling=4),
    "ragged_2x": dict(cformat=2, w=250, h=22, kind="noise", seed=25, dst=(500, 44), iUpscaling=4, exfmt=HDR10),
    # ---- formats / chroma ----
    "p016_fullrange": dict(cformat=3, w=64, h=32, kind="noise", seed=26, dst=(128, 64), exfmt=ext(MPEG2, FULL, M709), iUpscaling=2, full_range=True),
    "yv12_bt601_sd": dict(cformat=14, w=64, h=48, kind="structure", seed=27, dst=(64, 48)),
    "yuv420p8_cosited": dict(cformat=17, w=64, h=32, kind="noise", seed=28, dst=(128, 64), exfmt=ext(COSITED, TV, M709), iUpscaling=2),
    "yuv420p16_mpeg1": dict(cformat=21, w=64, h=32, kind="noise", seed=29, dst=(128, 64), exfmt=ext(MPEG1, TV, M709), iUpscaling=4),
    "p010_cosited_pq": dict(cformat=2, w=64, h=32, kind="noise", seed=30, dst=(128, 64), exfmt=ext(COSITED, TV, M2020, P2020, TPQ), iUpscaling=4),
    "p210_422": dict(cformat=6, w=64, h=32, kind="structure", seed=31, dst=(96, 48), iUpscaling=2),
    "yv16_422_catmull_chroma": dict(cformat=15, w=64, h=32, kind="noise", seed=32, dst=(64, 32), iChromaScaling=2),
    "yuv422p10_bilinear": dict(cformat=22, w=64, h=32, kind="noise", seed=33, dst=(128, 64), iUpscaling=1),
    "yv24_444": dict(cformat=16, w=48, h=32, kind="noise", seed=34, dst=(72, 48), iUpscaling=2),
    "yuv444p10": dict(cformat=24, w=48, h=32, kind="structure", seed=35, dst=(96, 64), iUpscaling=4),
    "yuv444p16_down": dict(cformat=25, w=96, h=64, kind="noise", seed=36, dst=(30, 20)),
    "nv12_chroma_nearest": dict(cformat=1, w=64, h=32, kind="noise", seed=37, dst=(128, 64), iChromaScaling=0, iUpscaling=2),
    "p010_chroma_catmull": dict(cformat=2, w=64, h=32, kind="noise", seed=38, dst=(128, 64), iChromaScaling=2, iUpscaling=4),
    "yuv420p10_chroma_catmull_cosited": dict(cformat=20, w=64, h=32, kind="noise", seed=39, dst=(64, 32), iChromaScaling=2, exfmt=ext(COSITED, TV, M709)),
    # ---- one-plane formats, planar RGB, gray ----
    "yuy2_bilinear_2x": dict(cformat=4, w=64, h=32, kind="structure", seed=60, dst=(128, 64), iUpscaling=2),
    "yuy2_noise_same_size": dict(cformat=4, w=62, h=20, kind="noise", seed=61, dst=(62, 20)),
    "uyvy_catmull_chroma": dict(cformat=5, w=64, h=32, kind="noise", seed=62, dst=(96, 48), iChromaScaling=2, iUpscaling=1),
    "y210_lanczos3_2x": dict(cformat=8, w=64, h=32, kind="noise", seed=63, dst=(128, 64), iUpscaling=4),
    "y216_catmull_chroma_down": dict(cformat=9, w=96, h=48, kind="structure", seed=64, dst=(40, 20), iChromaScaling=2),
    "v210_2x": dict(cformat=10, w=66, h=24, kind="noise", seed=65, dst=(132, 48), iUpscaling=2),
    "v210_ragged_width": dict(cformat=10, w=50, h=16, kind="structure", seed=66, dst=(50, 16)),
    "ayuv_same_size": dict(cformat=11, w=48, h=32, kind="noise", seed=67, dst=(48, 32)),
    "y410_pq_2x": dict(cformat=12, w=64, h=32, kind="hdr", seed=68, dst=(128, 64), exfmt=ext(0, TV, M2020, P2020, TPQ), iUpscaling=4),
    "y416_fullrange": dict(cformat=13, w=48, h=32, kind="noise", seed=69, dst=(72, 48), exfmt=ext(0, FULL, M709), iUpscaling=2, full_range=True),
    "gbrp8_2x": dict(cformat=26, w=48, h=32, kind="noise", seed=70, dst=(96, 64), iUpscaling=2),
    "gbrp10_procamp": dict(cformat=27, w=48, h=32, kind="structure", seed=71, dst=(48, 32), procamp=(8.0, 1.1, 0.0, 1.0)),
    "gbrp16_down": dict(cformat=28, w=96, h=64, kind="noise", seed=72, dst=(40, 24)),
    "y8_gray_2x": dict(cformat=37, w=62, h=32, kind="structure", seed=73, dst=(124, 64), iUpscaling=4),
    "y10_gray_tv_matrix": dict(cformat=38, w=48, h=32, kind="noise", seed=74, dst=(48, 32), exfmt=ext(0, TV, M709)),
    "y16_gray_crop": dict(cformat=39, w=64, h=48, kind="structure", seed=75, src_rect=(8, 4, 56, 44), dst=(96, 80), iUpscaling=1),
    # ---- interleaved RGB: no convert draw unless brightness/contrast are set; bottom-up DIBs ----
    "rgb24_same_size": dict(cformat=29, w=46, h=20, kind="noise", seed=110, dst=(46, 20)),
    "rgb32_catmull_2x": dict(cformat=30, w=48, h=32, kind="structure", seed=111, dst=(96, 64), iUpscaling=2),
    "argb32_bottom_up_down": dict(cformat=31, w=96, h=64, kind="structure", seed=112, dst=(40, 28), iDownscaling=2, bottom_up=1),
    "rgb24_bottom_up_procamp": dict(cformat=29, w=48, h=32, kind="noise", seed=113, dst=(48, 32), procamp=(15.0, 1.2, 40.0, 0.5), bottom_up=1),
    "rgb32_crop_offset_lanczos3": dict(cformat=30, w=96, h=64, kind="structure", seed=114, src_rect=(16, 8, 80, 56), dst=(128, 96),
                                       window=(200, 150), offset=(36, 27), iUpscaling=4),
    "r210_2x_dither": dict(cformat=32, w=48, h=32, kind="noise", seed=115, dst=(96, 64), iUpscaling=4),
    "r210_same_size_final_pass_on_source": dict(cformat=32, w=48, h=32, kind="structure", seed=116, src_rect=(8, 4, 40, 28), dst=(32, 24)),
    "rgb48_2x": dict(cformat=33, w=48, h=32, kind="noise", seed=117, dst=(96, 64), iUpscaling=1),
    "rgb48_width_not_multiple_of_4": dict(cformat=33, w=46, h=16, kind="structure", seed=118, dst=(46, 16)),
    "bgr48_ragged_same_size": dict(cformat=34, w=46, h=16, kind="noise", seed=119, dst=(46, 16)),
    "bgra64_rot90": dict(cformat=35, w=48, h=32, kind="structure", seed=120, dst=(32, 48), rotation=90),
    "b64a_procamp_contrast": dict(cformat=36, w=48, h=32, kind="noise", seed=121, dst=(72, 48), iUpscaling=2, procamp=(0.0, 0.8, 0.0, 1.0)),
    "rgb32_hue_only_stays_unconverted": dict(cformat=30, w=48, h=32, kind="noise", seed=122, dst=(48, 32), procamp=(0.0, 1.0, 90.0, 0.3)),
    # ---- blend deinterlace (bDeintBlend on interlaced 4:2:0 samples) ----
    "nv12_blend_deint": dict(cformat=1, w=64, h=32, kind="structure", seed=80, dst=(64, 32), bDeintBlend=1, sample_format=1),
    "p010_blend_deint_2x": dict(cformat=2, w=64, h=32, kind="noise", seed=81, dst=(128, 64), iUpscaling=4, bDeintBlend=1, sample_format=2),
    "yv12_blend_deint_progressive_sample": dict(cformat=14, w=64, h=32, kind="noise", seed=82, dst=(64, 32), bDeintBlend=1, sample_format=0),
    "yuv422p8_blend_deint_not_420": dict(cformat=18, w=64, h=32, kind="noise", seed=83, dst=(64, 32), bDeintBlend=1, sample_format=1),
    # ---- rotation / flip of the first resize draw (FillVertices :130-179, ResizeShaderPass :3112-3137) ----
    "rot90_copy_nv12": dict(cformat=1, w=64, h=40, kind="structure", seed=90, dst=(40, 64), rotation=90),
    "rot180_lanczos3_2x_dither": dict(cformat=2, w=64, h=32, kind="noise", seed=91, dst=(128, 64), iUpscaling=4, rotation=180),
    "rot270_down_hamming": dict(cformat=2, w=96, h=64, kind="structure", seed=92, dst=(20, 30), iDownscaling=2, rotation=270),
    "rot90_same_shader_single_draw": dict(cformat=2, w=48, h=32, kind="noise", seed=93, dst=(64, 96), iUpscaling=2, rotation=90),
    "rot90_two_pass_down_up": dict(cformat=1, w=96, h=32, kind="structure", seed=94, dst=(48, 40), iUpscaling=1, iDownscaling=5, rotation=90),
    "rot270_one_axis_only": dict(cformat=1, w=64, h=32, kind="noise", seed=95, dst=(32, 96), iUpscaling=3, rotation=270),
    "flip_ignored_same_rect_final_pass": dict(cformat=2, w=64, h=32, kind="structure", seed=96, dst=(64, 32), flip=1),
    "flip_copy_no_final_pass": dict(cformat=1, w=64, h=32, kind="structure", seed=97, dst=(64, 32), flip=1),
    "flip_offset_rect_final_pass": dict(cformat=2, w=64, h=32, kind="structure", seed=98, dst=(64, 32), window=(80, 48), offset=(8, 8), flip=1),
    "flip_catmull_1p5x": dict(cformat=2, w=64, h=32, kind="noise", seed=99, dst=(96, 48), iUpscaling=2, flip=1),
    "rot90_flip_mitchell": dict(cformat=1, w=64, h=48, kind="structure", seed=100, dst=(96, 80), iUpscaling=1, rotation=90, flip=1),
    "rot180_crop_letterbox": dict(cformat=2, w=96, h=64, kind="structure", seed=101, src_rect=(16, 8, 80, 56), dst=(128, 96),
                                  window=(200, 150), offset=(36, 27), iUpscaling=4, rotation=180),
    # ---- colour / settings ----
    "bt2020_sdr_gamma_gamut": dict(cformat=2, w=64, h=32, kind="structure", seed=40, dst=(128, 64), exfmt=ext(MPEG2, TV, M2020, P2020, T709), iUpscaling=2),
    "bt2020_gamma26": dict(cformat=2, w=64, h=32, kind="noise", seed=41, dst=(64, 32), exfmt=ext(MPEG2, TV, M2020, P2020, T26)),
    "pq_no_convert_to_sdr": dict(cformat=2, w=64, h=32, kind="hdr", seed=42, dst=(128, 64), exfmt=HDR10, bConvertToSdr=0, iUpscaling=4),
    "hlg_no_convert_bt2020": dict(cformat=2, w=64, h=32, kind="hdr", seed=43, dst=(64, 32), exfmt=HLG, bConvertToSdr=0),
    "pq_200nits": dict(cformat=2, w=64, h=32, kind="hdr", seed=44, dst=(128, 64), exfmt=HDR10, iSDRDisplayNits=200, iUpscaling=1),
    "ycgco": dict(cformat=19, w=48, h=32, kind="noise", seed=45, dst=(48, 32), exfmt=ext(0, FULL, MYCGCO)),
    "smpte240m": dict(cformat=1, w=64, h=32, kind="noise", seed=46, dst=(64, 32), exfmt=ext(MPEG2, TV, M240)),
    "procamp": dict(cformat=1, w=64, h=32, kind="structure", seed=47, dst=(128, 64), procamp=(12.0, 1.15, 25.0, 0.8), iUpscaling=2),
    "texfmt_16f_dither": dict(cformat=2, w=64, h=32, kind="noise", seed=48, dst=(128, 64), iTexFormat=16, iUpscaling=4, exfmt=HDR10),
    "texfmt_16f_out10": dict(cformat=2, w=64, h=32, kind="noise", seed=49, dst=(96, 48), iTexFormat=16, output_format=1, iUpscaling=2),
    "texfmt_10_out10_no_final": dict(cformat=2, w=64, h=32, kind="noise", seed=50, dst=(128, 64), output_format=1, iUpscaling=4),
    "texfmt_8_forced_on_10bit": dict(cformat=2, w=64, h=32, kind="structure", seed=51, dst=(128, 64), iTexFormat=8, iUpscaling=2),
    "texfmt_10_on_8bit_dither": dict(cformat=1, w=64, h=32, kind="structure", seed=52, dst=(128, 64), iTexFormat=10, iUpscaling=2),
    "dither_off_10bit": dict(cformat=2, w=64, h=32, kind="structure", seed=53, dst=(128, 64), bUseDither=0, iUpscaling=4),
    "nv12_pitch_padded": dict(cformat=1, w=62, h=32, kind="noise", seed=54, dst=(124, 64), iUpscaling=2),
    "p010_pitch_padded": dict(cformat=2, w=64, h=32, kind="noise", seed=55, dst=(128, 64), iUpscaling=4, pitch=160),
}

# ---- pinning cases: used by tests/test_ref_hlsl.py only (oracle vs the reference's own shader text, oracle/ref_hlsl/).
# Power-of-two sizes and ratios: every texture coordinate is exactly representable, so the reference arithmetic has ONE fp32
# evaluation and the oracle must reproduce it bit for bit (other ratios carry an ulp of slack in Tex * wh, see the test).
PINNING_CASES = {}
for _m, _n in ((1, "mitchell"), (2, "catmull"), (3, "lanczos2"), (4, "lanczos3"), (5, "jinc2"), (0, "nearest")):
    PINNING_CASES["pin_up2x_" + _n] = dict(cformat=2, w=64, h=32, kind="noise", seed=300 + _m, dst=(128, 64), iUpscaling=_m)
    PINNING_CASES["pin_up4x_" + _n] = dict(cformat=1, w=32, h=16, kind="noise", seed=310 + _m, dst=(128, 64), iUpscaling=_m)
    PINNING_CASES["pin_half_via_up_" + _n] = dict(cformat=2, w=128, h=64, kind="noise", seed=320 + _m, dst=(64, 32), iUpscaling=_m)
for _m, _n in ((0, "box"), (1, "bilinear"), (2, "hamming"), (3, "bicubic"), (4, "bicubic_sharp"), (5, "lanczos")):
    PINNING_CASES["pin_down4x_" + _n] = dict(cformat=2, w=256, h=128, kind="noise", seed=330 + _m, dst=(64, 32), iDownscaling=_m)
    PINNING_CASES["pin_down2x_" + _n] = dict(cformat=1, w=128, h=64, kind="noise", seed=340 + _m, dst=(64, 32), iDownscaling=_m,
                                             bInterpolateAt50pct=0)
    PINNING_CASES["pin_down8x_x_only_" + _n] = dict(cformat=2, w=512, h=32, kind="noise", seed=350 + _m, dst=(64, 32), iDownscaling=_m)
for _i, (_cf, _ex) in enumerate(((2, HDR10), (2, HLG), (20, ext(COSITED, TV, M709)), (21, ext(MPEG1, FULL, M2020, P2020, T22)), (1, ext(MPEG2, TV, M601)),
                                 (6, ext(matrix=M709)), (16, ext(0, FULL, MYCGCO)), (24, HDR10))):
    for _cs in (0, 1, 2):
        PINNING_CASES["pin_convert_%d_chroma%d" % (_i, _cs)] = dict(cformat=_cf, w=64, h=32, kind="noise", seed=360 + 3 * _i + _cs, dst=(64, 32),
                                                                      exfmt=_ex, iChromaScaling=_cs, full_range=(_i in (3, 6)))

# ---- full-size cases: the BASELINE.json configurations (and the two everyday non-2x bench workloads) at their REAL sizes.
# tests/golden/make_full_size_pins.py runs the reference's own shader text over them (oracle/ref_hlsl) and records the sha256 of
# its render target; tests/test_ref_hlsl.py holds the oracle to those hashes, tests/test_parity_gpu.py holds every GPU tier to
# the reference-text output directly (live on the GPU box, where libref_hlsl.so travels).
FULL_SIZE_CASES = {
    "c3hdr": dict(cformat=2, w=3840, h=2160, kind="noise", seed=77, dst=(7680, 4320), exfmt=HDR10, iUpscaling=4),
    "c3_sdr": dict(cformat=2, w=3840, h=2160, kind="noise", seed=77, dst=(7680, 4320), exfmt=ext(matrix=M709), iUpscaling=4),
    "c5_hlg": dict(cformat=2, w=3840, h=2160, kind="noise", seed=77, dst=(7680, 4320), exfmt=HLG, iUpscaling=4),
    "c4_mitchell": dict(cformat=2, w=3840, h=2160, kind="noise", seed=77, dst=(7680, 4320), exfmt=HDR10, iUpscaling=1),
    "C1": dict(cformat=1, w=1920, h=1080, kind="structure", seed=201, dst=(1920, 1080), exfmt=ext(matrix=M709)),
    "C2": dict(cformat=20, w=1920, h=1080, kind="noise", seed=202, dst=(3840, 2160), exfmt=ext(matrix=M709), iUpscaling=2),
    "up1440": dict(cformat=2, w=1920, h=1080, kind="noise", seed=311, dst=(2560, 1440), exfmt=HDR10, iUpscaling=4),
    "down1440": dict(cformat=2, w=3840, h=2160, kind="noise", seed=312, dst=(2560, 1440), exfmt=HDR10, iDownscaling=2),
    "up1080_from_720_nv12": dict(cformat=1, w=1280, h=720, kind="noise", seed=318, dst=(1920, 1080), exfmt=ext(matrix=M709), iUpscaling=2),
    "down1080_from_4k_hlg": dict(cformat=2, w=3840, h=2160, kind="noise", seed=315, dst=(1920, 1080), exfmt=HLG, iUpscaling=1),
    # round 3's new geometries: 3:1 (every third row and column exactly on a texel centre: the fp32 texcoord decides the tap rows),
    # a flipped and an upside-down frame, a 13-tap ps_convolution downscale
    "up2160_from_720": dict(cformat=2, w=1280, h=720, kind="noise", seed=417, dst=(3840, 2160), exfmt=HDR10, iUpscaling=4),
    "up720_from_240_nv12_catmull": dict(cformat=1, w=426, h=240, kind="noise", seed=415, dst=(1278, 720), exfmt=ext(matrix=M709), iUpscaling=2),
    "flipped_540_to_720_nv12": dict(cformat=1, w=960, h=540, kind="noise", seed=418, dst=(1280, 720), exfmt=ext(matrix=M709), iUpscaling=4, flip=1),
    "rot180_540_to_720_pq": dict(cformat=2, w=960, h=540, kind="noise", seed=439, dst=(1280, 720), exfmt=HDR10, iUpscaling=4, rotation=180),
    "down1080_from_4k_lanczos_convolution": dict(cformat=2, w=3840, h=2160, kind="noise", seed=320, dst=(1920, 1080), exfmt=HDR10, iDownscaling=5,
                                                 bInterpolateAt50pct=0),
    # round 5: the one-draw 2-D scaler at exactly 2x (the fused Jinc2m kernel; the 8-bit source runs the exact form of its convert stage)
    "jinc_4k_from_1080_pq": dict(cformat=2, w=1920, h=1080, kind="noise", seed=521, dst=(3840, 2160), exfmt=HDR10, iUpscaling=5),
    "jinc_1440_from_720_nv12": dict(cformat=1, w=1280, h=720, kind="noise", seed=522, dst=(2560, 1440), exfmt=ext(matrix=M709), iUpscaling=5),
}

# the two ColorFormat_t values no other case carries (P216, YUV422P16): with them the reference-text comparison covers all 39 formats
PINNING_CASES["pin_format_p216_2x"] = dict(cformat=7, w=64, h=32, kind="noise", seed=390, dst=(128, 64), iUpscaling=2, exfmt=ext(matrix=M709))
PINNING_CASES["pin_format_yuv422p16_down"] = dict(cformat=23, w=128, h=64, kind="noise", seed=391, dst=(48, 24), iDownscaling=2, exfmt=HDR10)

# ps_convolution near its largest tap count (128: BuildAxisTaps, ORC_MAX_TAPS) on a 16-output strip: a Lanczos downscale at 20x (121 taps)
# along X and a Box downscale at 120x (121 taps) along Y, so that the oracle's answer at the top of the ladder of tests/large_geometry.py
# rests on the reference's own ps_convolution.hlsl text
PINNING_CASES["pin_down20x_x_only_lanczos_121taps"] = dict(cformat=2, w=320, h=32, kind="noise", seed=395, dst=(16, 32), iDownscaling=5)
PINNING_CASES["pin_down120x_y_only_box_121taps"] = dict(cformat=1, w=64, h=1920, kind="noise", seed=396, dst=(64, 16), iDownscaling=0, exfmt=ext(matrix=M709))

SETTING_KEYS = ("iTexFormat", "iChromaScaling", "iUpscaling", "iDownscaling", "bInterpolateAt50pct",
                "bUseDither", "bConvertToSdr", "iSDRDisplayNits", "output_format", "flags")


def case_geometry(c):
    w2, h2 = c["dst"]
    ww, wh = c.get("window", (w2, h2))
    ox, oy = c.get("offset", (0, 0))
    return (ww, wh), (ox, oy, ox + w2, oy + h2)


def case_frame(c):
    frame, pitch = synth.make_frame(c["cformat"], c["w"], c["h"], c["kind"], seed=c["seed"], pitch=c.get("pitch"),
                                    full_range=c.get("full_range", False))
    if c.get("bottom_up"):       # BI_RGB with biHeight > 0: rows stored last-first, negative pitch (:1801-1803)
        frame = np.ascontiguousarray(frame.reshape(c["h"], pitch)[::-1]).reshape(-1)
        pitch = -pitch
    return frame, pitch


def oracle_params(oracle, c):
    (ww, wh), vr = case_geometry(c)
    kw = {k: c[k] for k in SETTING_KEYS if k in c}
    p = oracle.default_params(cformat=c["cformat"], width=c["w"], height=c["h"], exfmt=c.get("exfmt", 0),
                              window_w=ww, window_h=wh, video_rect=vr, **kw)
    if "src_rect" in c:
        oracle.set_params(p, src_rect=c["src_rect"])
    if "procamp" in c:
        b, ct, h, s = c["procamp"]
        oracle.set_params(p, brightness=b, contrast=ct, hue=h, saturation=s)
    # m_bDeintBlend && m_SampleFormat != PROGRESSIVE (DX11VideoProcessor.cpp:3075); the 4:2:0 check is the oracle's
    oracle.set_params(p, blend_deint=int(bool(c.get("bDeintBlend", 0)) and c.get("sample_format", 0) != 0))
    oracle.set_params(p, rotation=c.get("rotation", 0), flip=c.get("flip", 0))
    oracle.set_params(p, hdr_display_max_nits=c.get("hdr_display", 1000.0))     # m_iHdrDisplayMaxNits (level-2 selection)
    if "dovi" in c:
        oracle.set_params(p, dovi=synth.dovi_metadata(**c["dovi"]))
    if c.get("hdr_output"):
        m = c.get("hdr_meta", (0.0, 0.0, 0.0, 0.0))
        oracle.set_params(p, hdr_output=1, hdr_tonemap_type=c.get("hdr_tonemap", 0), hdr_display_max_nits=c.get("hdr_display", 1000.0),
                          hdr_min_mastering=m[0], hdr_max_mastering=m[1], hdr_max_cll=m[2], hdr_max_fall=m[3])
    return p


def run_case(oracle, name, background=0):
    """Oracle output for a named case: (window_h, window_w, 4) uint8; untouched pixels = background."""
    c = GOLDEN_CASES[name] if name in GOLDEN_CASES else PINNING_CASES[name] if name in PINNING_CASES else FULL_SIZE_CASES[name]
    frame, pitch = case_frame(c)
    p = oracle_params(oracle, c)
    dst = np.full((p.window_h, p.window_w, 4), background, dtype=np.uint8)
    return oracle.process(p, frame, pitch, dst=dst)
