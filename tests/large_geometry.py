"""The largest ratios and frame extents the resize routes accept: the case table and helpers of tests/test_large_geometry.py (CPU) and
tests/test_large_geometry_gpu.py (GPU).  Importable without a GPU.

tests/tiny_frames.py pins the small end of every route and tests/huge_layouts.py the address end; this table draws the large end of the
GEOMETRY: ps_convolution downscales from 16 to 128 taps per axis (BuildAxisTaps accepts 128 and refuses 129, like the oracle's ORC_MAX_TAPS),
the 16-tap / 32-row-ring variant of k_fused_strip at and around its limits, the LDS gates that choose between the tiled, column, row-window and
plain kernels of the pass-per-kernel tiers, upscales of 16x to 127x, and thin frames whose long side is the input limit (16384) or the
non-power-of-two extents at which TexCenter's fp32 texture coordinate drifts furthest from the nominal filter phase (16380, 15360).

A case is a dict in the style of tests/golden/cases.py plus:
    name         unique, family first
    taps         {"x": n, "y": n}: ntaps of the resize draw along that screen axis (absent axis: no draw)
    strip        True: the processor's plan holds a strip plan (api.plan_draw_tables; an exact-2x plan keeps one behind k_fused_up2x); False /
                 absent: it does not
    fused        the fragment GetVPInfo must show on the default tier; None: no name of FUSED_NAMES may appear
    aside        an exact-2x case whose predictor (below) is above the planner's threshold: the nominal-phase kernels must have stepped aside
    refused      every tier and the oracle refuse the geometry (family F; nothing else in the table is refused)
    ring, acols, passes, strip_nt, spans ...   what the family's CPU test asserts of the plan
Content is "noise" throughout; every frame stays small by being thin.

The exact-2x predictor (family E).  k_fused_up2x uses the two nominal weight sets of t = 0.75 / 0.25 and the Jinc2m kernels of a dyadic ratio a
table of the nominal phases; the real weights drift from them with the fp32 rounding of the texture coordinate.  predictor = max over the
outputs of an axis of sum_k |w_real - w_nominal|, times the quantisation of the target (255 / 1023): twice the furthest ONE axis can move the
filtered value, in codes.  tests/test_large_geometry.py computes it (api.plan_axis_taps; Jinc2m: the shader's weights restated in numpy):
                             Lanczos3 (6 weights)   8 bits   10 bits      Jinc2m (16 weights)   8 bits   10 bits
    texture 3840 -> 7680     3.05e-4                0.078    0.31         7.7e-4                0.20     0.79       (the headline)
    texture 7680 -> 15360    6.09e-4                0.155    0.62
    16380, 15360 (whole)     1.22e-3                0.311    1.25         3.08e-3               0.79     3.15
    16384, 8, 16 (whole)     0                      0        0            0                     0        0
A source rect of a planar sample does not enter: the resize draws read the convert draw's output, which is rect-sized with the rect at its
origin.  Only an interleaved RGB sample (no convert draw) is read in place — and then by k_fused_strip:surface with the real table.

Measured on an MI355X, default tier against the oracle, frames of 0.5 M pixels (max |delta| in codes of the target, share of channels off by one):
  * 8-bit targets: exact 2x at 16384 1 / 0.00001 .. 0.00043, at 16380 1 / 0.00002 .. 0.00042, at 15360 (predictor 0.31) 1 / 0.00066 .. 0.00118: the
    drift is there (two to three times the channels) and far inside the bar;
  * R10G10B10A2 with HDR passthrough, exact 2x Lanczos3 at 15360 (predictor 1.25) through k_fused_up2x: 2 / 0.00324 (h: 1 / 0.00297) against
    1 / 0.00009 at 16384: 30 times the channels.  The planner now holds the nominal-phase kernels to 0.5 codes per axis (vp_plan.h:
    kNominalPhaseMaxCodes); above it k_fused_strip draws the frame with the real table: 2 / 0.00012 (h: 1 / 0.00011) — the share is the
    power-of-two frame's.  The one channel two codes off is NOT the drift's: it is there with the real table too, and the Jinc2m frames
    show 1 to 8 such channels of 1.5 M on every route, at 16384 as well (a code of the 10-bit convert output under a filter whose weights'
    magnitudes sum to more than one); compare_rgb10 grants a PQ-tagged source two codes;
  * Jinc2m on the folded tier (k_jinc2_phases against the per-pixel k_jinc2, the bar 0.999 identical): 8 bits at 15360 1137 of 5.9 M bytes,
    10 bits at 15360 4655 of 2.1 M bytes = 0.997 — below the bar until the phase table was held to the same threshold (BuildJincPhases).
"""
from tests.golden.cases import HDR10, HLG, M709, ext

SDR = ext(matrix=M709)
NV12, P010, RGB32, R210 = 1, 2, 30, 32
MITCHELL, CATMULL, LANCZOS2, LANCZOS3, JINC2 = 1, 2, 3, 4, 5
BOX, BILINEAR, HAMMING, BICUBIC, BICUBIC_SHARP, LANCZOS = 0, 1, 2, 3, 4, 5
DOWN_NAMES = ("box", "bilinear", "hamming", "bicubic", "bicubic_sharp", "lanczos")
FLAG_LANCZOS3_FIXED = 1           # (= api.FLAG_LANCZOS3_FIXED: six taps; no library is loaded to import this table)

FUSED_NAMES = ("fused_up2x", "fused_jinc2x", "kernel=fused_strip", "kernel=fused_period")

# the LDS gates of the pass-per-kernel tier (vp_kernels.hip): the widest source span of a block of 64 / 32 / 8 outputs the tiled (k_resize_2d),
# column (k_resize_cols) and row-window (k_resize_rows) kernels stage
K_RESIZE_SPAN_MAX, K_RESIZE_TILE_ROWS_MAX, K_RESIZE_ROW_SPAN_MAX = 192, 72, 14
MAX_TAPS = 128                    # BuildAxisTaps / ORC_MAX_TAPS
MAX_EXTENT = 16384                # mpcvr_set_input

_seed = [9000]


def _case(family, tag, cformat, src, dst, exfmt=SDR, **kw):
    _seed[0] += 1
    c = dict(name=f"{family}_{tag}", family=family, cformat=cformat, w=src[0], h=src[1], kind="noise", seed=_seed[0], dst=tuple(dst),
             exfmt=0 if cformat in (RGB32, R210) else exfmt)
    c.update(kw)
    return c


FORMATS = (("p010_pq", P010, HDR10), ("nv12", NV12, SDR), ("rgb32", RGB32, 0))

# ---- family A: the tap-count ladder of ps_convolution.  LADDER[filter] = source lengths onto 16 outputs whose ntaps is the rung's
# (16, 17, a mid value, the largest: 128), then the refused length (>= 129 taps; family F).  Bilinear = Hamming, Bicubic sharp = Bicubic (support)
RUNGS = (16, 17, 64, 128)
# The lengths are no multiples of 16: the windows of the output rows then differ in length, and the shorter ones are padded with zero weights
LADDER = {BOX: (236, 252, 1002, 2028, 2048), BILINEAR: (116, 124, 500, 1012, 1024), HAMMING: (116, 124, 500, 1012, 1024),
          BICUBIC: (58, 62, 250, 506, 512), BICUBIC_SHARP: (58, 62, 250, 506, 512), LANCZOS: (38, 42, 166, 338, 342)}
N_FILTERED, N_OTHER = 16, 70      # outputs along the filtered axis (both edge clamps and interior pixels) / the other axis (a second block of 64)


def _ladder():
    out = []
    n = 0
    for m in range(6):
        for r, rung in enumerate(RUNGS):
            s = LADDER[m][r]
            down = dict(iDownscaling=m, bInterpolateAt50pct=n % 2)
            for k, axes in enumerate(("x", "y", "xy")):
                tag, cf, ex = FORMATS[(m + r + k) % 3]
                n += 1
                over = dict(down)
                if axes == "x" and m == r:
                    over["iTexFormat"] = 16                      # one case per rung on fp16 surfaces
                if axes == "y" and m == (r + 1) % 6:
                    over["output_format"] = 1                    # ... and one into an R10G10B10A2 target
                if axes == "x":
                    src, dst, taps = (s, N_OTHER), (N_FILTERED, N_OTHER), dict(x=rung)
                elif axes == "y":
                    src, dst, taps = (N_OTHER, s), (N_OTHER, N_FILTERED), dict(y=rung)
                elif rung <= 17:
                    # both axes, five times the outputs along X at the same ratio: more than one 64-wide strip for k_fused_strip (16 taps)
                    src, dst, taps = (5 * s, s), (5 * N_FILTERED, N_FILTERED), dict(x=rung, y=rung)
                else:
                    src, dst, taps = (s, s), (N_FILTERED, N_FILTERED), dict(x=rung, y=rung)
                # 16 taps on both axes is k_fused_strip's (nt = 16); above that and on one axis the pass-per-kernel draws run.  fp16 surfaces
                # and RGB samples go through the surface variant
                strip = axes == "xy" and rung == 16
                fused = None if not strip else "kernel=fused_strip:surface(" if cf == RGB32 else "kernel=fused_strip("
                out.append(_case("ladder", f"{DOWN_NAMES[m]}_{rung}taps_{axes}_{tag}", cf, src, dst, ex, taps=taps, strip=strip, fused=fused,
                                 strip_nt=16 if strip else None, **over))
        # one mixed case per filter: the top rung on one axis against a 4-tap upscale on the other
        s = LADDER[m][3]
        tag, cf, ex = FORMATS[m % 3]
        if m % 2 == 0:
            src, dst, taps = (s, 40), (N_FILTERED, N_OTHER), dict(x=128, y=4)
        else:
            src, dst, taps = (40, s), (N_OTHER, N_FILTERED), dict(x=4, y=128)
        out.append(_case("ladder", f"{DOWN_NAMES[m]}_128taps_against_mitchell_up_{'x' if m % 2 == 0 else 'y'}_{tag}", cf, src, dst, ex, taps=taps,
                         strip=False, fused=None, iDownscaling=m, iUpscaling=MITCHELL))
    return out


# ---- family F: refusal at 129 taps and above, one geometry per filter, the axes taking turns
def _refused():
    out = []
    for m in range(6):
        s = LADDER[m][4]
        tag, cf, ex = FORMATS[m % 3]
        src, dst = (((s, N_OTHER), (N_FILTERED, N_OTHER)), ((N_OTHER, s), (N_OTHER, N_FILTERED)), ((s, s), (N_FILTERED, N_FILTERED)))[m % 3]
        # back_to: the video rect the context goes back to — twice the outputs along the refused axes, half the taps
        out.append(_case("refused", f"{DOWN_NAMES[m]}_{'x y xy'.split()[m % 3]}_{tag}", cf, src, dst, ex, refused=True, iDownscaling=m,
                         back_to=tuple(2 * d if d == N_FILTERED else d for d in dst)))
    return out


# ---- family B: the strip kernel's edges.  Each geometry from the raw sample (P010 / NV12: kernel=fused_strip() and from a surface (RGB32, or
# Catmull-Rom chroma: kernel=fused_strip:surface(), the tails none / PQ / HLG taking turns.
# The ring holds the source rows of one output row's window plus one: a window spans at most ntaps <= 16 rows, so 32 rows are reached by
# the 16-row window alone (span + 1 = 17 > 16) and a window of 17 .. 31 rows does not exist: one row beyond the largest ring-32 window is the
# 17th tap, which PlanFusedStrip refuses.
STRIP_GEOMETRIES = (
    # tag, src, dst, settings, what the plan must show
    ("ring32_span16", (200, 120), (80, 16), dict(iDownscaling=HAMMING, bInterpolateAt50pct=0), dict(ring=32, strip_nt=16, yspan=16)),
    ("nt16_x_up_y", (600, 40), (80, 70), dict(iDownscaling=HAMMING, iUpscaling=MITCHELL), dict(strip_nt=16, tapsxy=(16, 4), ring=8)),
    ("up_x_nt16_y", (40, 120), (70, 16), dict(iDownscaling=HAMMING, iUpscaling=LANCZOS3), dict(strip_nt=16, tapsxy=(6, 16), ring=32)),
    ("four_convert_passes", (560, 40), (80, 16), dict(iDownscaling=HAMMING), dict(strip_nt=16, passes=4, acols=452)),
    ("widest_acols_box_15p5x", (1240, 40), (80, 16), dict(iDownscaling=BOX), dict(strip_nt=16, passes=8, acols=994, widest=True)),
)
STRIP_REFUSED = ("ring32_one_row_beyond", (200, 128), (80, 16), dict(iDownscaling=HAMMING, bInterpolateAt50pct=0))
STRIP_SOURCES = (("p010_pq", P010, HDR10, {}), ("p010_hlg", P010, HLG, {}), ("nv12", NV12, SDR, {}),
                 ("rgb32_surface", RGB32, 0, {}), ("p010_pq_catmull_chroma_surface", P010, HDR10, dict(iChromaScaling=2)),
                 ("p010_hlg_catmull_chroma_surface", P010, HLG, dict(iChromaScaling=2)))


def _strip_edges():
    out = []
    for gtag, src, dst, over, want in STRIP_GEOMETRIES:
        for stag, cf, ex, sover in STRIP_SOURCES:
            fused = "kernel=fused_strip:surface(" if "surface" in stag else "kernel=fused_strip("
            out.append(_case("strip", f"{gtag}_{stag}", cf, src, dst, ex, strip=True, fused=fused, **want, **over, **sover))
    gtag, src, dst, over = STRIP_REFUSED
    for stag, cf, ex, sover in STRIP_SOURCES[:1] + STRIP_SOURCES[2:4]:
        out.append(_case("strip", f"{gtag}_{stag}", cf, src, dst, ex, strip=False, fused=None, tapsxy=(7, 17), **over, **sover))
    return out


# ---- family C: the LDS gates of the folded kernels.  GATE_GEOMETRIES: (tag, src, dst, settings, {pack: {field: value}}): the spans
# api.plan_draw_tables must report ("x" = the first draw's pack, "y" = the second's).  `at` = the span equals the gate, `above` = it exceeds it
# by the value given.  The row window of k_resize_rows (compile-time 4 / 6 taps) has two gates: K_RESIZE_ROW_SPAN_MAX and RowWindowPays
# (blk8_span * 3 <= ntaps * 8): 14 | 15 rows with 6 taps, 10 | 11 rows with 4
_HAM = dict(iDownscaling=HAMMING, bInterpolateAt50pct=0, iUpscaling=MITCHELL)
GATE_GEOMETRIES = (
    # blk_span: source columns under a block of 64 outputs of the X draw
    ("blk_span_192", (284, 40), (96, 70), _HAM, dict(x=dict(blk_span=192))),
    ("blk_span_193", (208, 40), (70, 70), _HAM, dict(x=dict(blk_span=193))),
    # blk32_span: source rows under a block of 32 output rows of the Y draw
    ("blk32_span_72", (70, 88), (70, 40), _HAM, dict(x=dict(blk32_span=72))),
    ("blk32_span_73", (70, 106), (70, 48), _HAM, dict(x=dict(blk32_span=73))),
    # blk8_span: source rows under 8 output rows of the interpolation shaders below 1.4x
    ("blk8_span_14_lanczos3", (70, 42), (70, 40), dict(iUpscaling=LANCZOS3, flags=FLAG_LANCZOS3_FIXED), dict(x=dict(blk8_span=14, ntaps=6, row_window=True))),
    ("blk8_span_15_lanczos3", (70, 48), (70, 40), dict(iUpscaling=LANCZOS3, flags=FLAG_LANCZOS3_FIXED), dict(x=dict(blk8_span=15, ntaps=6, row_window=False))),
    ("blk8_span_10_mitchell", (70, 60), (70, 80), dict(iUpscaling=MITCHELL), dict(x=dict(blk8_span=10, ntaps=4, row_window=True))),
    ("blk8_span_11_mitchell", (70, 50), (70, 48), dict(iUpscaling=MITCHELL), dict(x=dict(blk8_span=11, ntaps=4, row_window=False))),
    # both axes: X passes the tiled kernel's gate and Y does not, and the reverse: the two separate kernels
    ("x_inside_y_outside", (284, 106), (96, 48), _HAM, dict(x=dict(blk_span=192), y=dict(blk32_span=73))),
    ("x_outside_y_inside", (208, 88), (70, 40), _HAM, dict(x=dict(blk_span=193), y=dict(blk32_span=72))),
    ("x_inside_y_inside", (284, 88), (96, 40), _HAM, dict(x=dict(blk_span=192), y=dict(blk32_span=72))),
)


def _gates():
    out = []
    for i, (gtag, src, dst, over, spans) in enumerate(GATE_GEOMETRIES):
        for tag, cf, ex in (FORMATS[i % 3], FORMATS[(i + 1) % 3]):
            # (a two-draw resize is k_fused_strip's on the default tier; the gates act on the plain and folded tiers)
            two = src[0] != dst[0] and src[1] != dst[1]
            fused = None if not two else "kernel=fused_strip:surface(" if cf == RGB32 else "kernel=fused_strip("
            out.append(_case("gates", f"{gtag}_{tag}", cf, src, dst, ex, spans=spans, strip=two, fused=fused, **over))
    return out


# ---- family D: large upscale ratios.  8 x 8 and 10 x 6 sources to 16x, 64x and 127x, one axis only and both axes: many output rows share
# one source row (k_fused_strip's row march with a ring of 8; every lane of a strip reads the same few columns)
UP_METHODS = ((MITCHELL, "mitchell"), (LANCZOS3, "lanczos3"), (JINC2, "jinc2"))


def _big_up():
    out = []
    for si, src in enumerate(((8, 8), (10, 6))):
        for ri, ratio in enumerate((16, 64, 127)):
            for ai, axes in enumerate(("x", "y", "xy")):
                up, uname = UP_METHODS[(si + ri + ai) % 3]
                tag, cf, ex = FORMATS[(si + ri + 2 * ai) % 3]
                dst = (src[0] * (ratio if "x" in axes else 1), src[1] * (ratio if "y" in axes else 1))
                strip = axes == "xy" and up != JINC2             # (a two-draw resize; Jinc2m is one 2-D draw)
                fused = None if not strip else "kernel=fused_strip:surface(" if cf == RGB32 else "kernel=fused_strip("
                out.append(_case("bigup", f"{uname}_{ratio}x_{axes}_{src[0]}x{src[1]}_{tag}", cf, src, dst, ex, iUpscaling=up, strip=strip, fused=fused, ratio=ratio,
                                 strip_nt=(4 if up == MITCHELL else 6) if strip else None, ring=8 if strip else None))
    return out


# ---- family E: the largest extents.  Thin frames, the long side 16384 (the input limit, a power of two: no phase drift), 16380 and 15360
# (the extents at which the drift is largest), as width and as height
LONG_SIDES = (16384, 16380, 15360)
UP2X = {"taps4": dict(iUpscaling=MITCHELL), "taps5": dict(iUpscaling=LANCZOS3), "taps6": dict(iUpscaling=LANCZOS3, flags=FLAG_LANCZOS3_FIXED)}


def _along(orient, long_, short):
    return (long_, short) if orient == "w" else (short, long_)


def _extents():
    out = []
    n = 0
    for L in LONG_SIDES:
        for orient in ("w", "h"):
            two = lambda s: (2 * s[0], 2 * s[1])
            src = _along(orient, L, 8)
            for ttag, over in UP2X.items():
                tag, cf, ex = FORMATS[n % 2]
                n += 1
                out.append(_case("extent", f"up2x_{ttag}_{orient}{L}_{tag}", cf, src, two(src), ex, plan="fused_up2x", fused="fused_up2x", strip=True, predict=True, **over))
            tag, cf, ex = FORMATS[n % 2]
            n += 1
            # (Jinc2m's 16 weights move 2.5 times as far as Lanczos3's six: at 16380 and 15360 its predictor is 0.79 codes of 8 bits — `aside`)
            drifts = L != 16384
            out.append(_case("extent", f"jinc2x_{orient}{L}_{tag}", cf, src, two(src), ex, plan="fused_jinc2x", fused=None if drifts else "fused_jinc2x", predict=True,
                             aside=drifts, iUpscaling=JINC2))
            # 1.5x along the long side, 13 / 8 along the short one (not a periodic ratio): k_fused_strip
            tag, cf, ex = FORMATS[n % 2]
            n += 1
            dst = (3 * L // 2, 13) if orient == "w" else (13, 3 * L // 2 + 2)
            out.append(_case("extent", f"strip_1p5x_{orient}{L}_{tag}", cf, src, dst, ex, plan="passes:", fused="kernel=fused_strip(", strip=True, iUpscaling=LANCZOS3))
            # 4:3 down the rows: k_fused_period (an even output width: its 8-byte stores)
            if orient == "w" or L % 3 == 0:
                tag, cf, ex = FORMATS[n % 2]
                n += 1
                src43 = _along(orient, L, 12)
                dst = ((4 * L // 3 + 1) & ~1, 16) if orient == "w" else (16, 4 * L // 3)
                out.append(_case("extent", f"period_4to3_{orient}{L}_{tag}", cf, src43, dst, ex, plan="passes:", fused="kernel=fused_period(rows=4:3,taps=5,", strip=True,
                                 period=(4, 3, 5), iUpscaling=LANCZOS3))
            # same size: the streaming convert (width % 4 == 0) and, two columns narrower, k_convert_blocks
            for w_off in (0, 2):
                tag, cf, ex = FORMATS[n % 2]
                n += 1
                s = (src[0] - w_off, src[1]) if orient == "w" else (src[0] + w_off, src[1])
                out.append(_case("extent", f"same_size_{orient}{L}_{s[0]}x{s[1]}_{tag}", cf, s, s, ex, plan="direct:", fused=None))
            # a 2.5x Hamming downscale on both axes
            tag, cf, ex = FORMATS[n % 2]
            n += 1
            srcd = _along(orient, L, 40)
            dst = _along(orient, (2 * L // 5 + 1) & ~1, 16)
            out.append(_case("extent", f"down_2p5x_hamming_{orient}{L}_{tag}", cf, srcd, dst, ex, plan="passes:", fused="kernel=fused_strip(", strip=True, iDownscaling=HAMMING))
    # output formats on the worst extents: R10G10B10A2 with HDR passthrough (the 10-bit code is the one the drift moves first) and without.
    # There the predictor is 1.0 .. 1.25 ten-bit codes, above the planner's threshold of 0.5 (vp_plan.h: kNominalPhaseMaxCodes): `aside` —
    # the exact-2x kernel hands the frame to k_fused_strip (the real table), the Jinc2m draw runs the per-pixel k_jinc2 behind a convert kernel
    for L in (16380, 15360):
        for orient in ("w", "h"):
            src = _along(orient, L, 8)
            dst = (2 * src[0], 2 * src[1])
            out.append(_case("extent", f"up2x_taps5_{orient}{L}_p010_pq_hdr_out10", P010, src, dst, HDR10, plan="passes:", fused="kernel=fused_strip(", strip=True, predict=True,
                             aside=True, iUpscaling=LANCZOS3, output_format=1, hdr_output=1))
            out.append(_case("extent", f"jinc2x_{orient}{L}_p010_pq_hdr_out10", P010, src, dst, HDR10, plan="fused_jinc2x", fused=None, predict=True, aside=True,
                             iUpscaling=JINC2, output_format=1, hdr_output=1))
    out.append(_case("extent", "up2x_taps4_w16380_p010_sdr_out10", P010, (16380, 8), (32760, 16), SDR, plan="passes:", fused="kernel=fused_strip(", strip=True, predict=True,
                     aside=True, iUpscaling=MITCHELL, output_format=1))
    out.append(_case("extent", "up2x_taps6_w16384_p010_pq_hdr_out10", P010, (16384, 8), (32768, 16), HDR10, plan="fused_up2x", fused="fused_up2x", strip=True, predict=True,
                     iUpscaling=LANCZOS3, flags=FLAG_LANCZOS3_FIXED, output_format=1, hdr_output=1))
    out.append(_case("extent", "jinc2x_w16384_p010_pq_hdr_out10", P010, (16384, 8), (32768, 16), HDR10, plan="fused_jinc2x", fused="fused_jinc2x", predict=True,
                     iUpscaling=JINC2, output_format=1, hdr_output=1))
    # source rects of 64 .. 256 columns (rows) starting at or beyond 13900 of a 16380-wide (-tall) texture, left / top multiples of 4 / 2
    rects = (("w", (13900, 0, 14156, 8)), ("w", (16000, 0, 16064, 8)), ("h", (0, 13900, 8, 14156)), ("h", (0, 16316, 8, 16380)))
    for i, (orient, r) in enumerate(rects):
        tex = _along(orient, 16380, 8)
        rw, rh = r[2] - r[0], r[3] - r[1]
        for tag, cf, ex in FORMATS[:2]:
            out.append(_case("extent", f"rect_{orient}_at_{max(r[0], r[1])}_up2x_{tag}", cf, tex, (2 * rw, 2 * rh), ex, src_rect=r, plan="fused_up2x", fused="fused_up2x", strip=True,
                             predict=True, iUpscaling=LANCZOS3))
            dst = (3 * rw // 2, 13) if orient == "w" else (13, 3 * rh // 2 + 2)
            out.append(_case("extent", f"rect_{orient}_at_{max(r[0], r[1])}_1p5x_{tag}", cf, tex, dst, ex, src_rect=r, plan="passes:", fused="kernel=fused_strip(", strip=True,
                             iUpscaling=LANCZOS3))
        # an interleaved RGB sample is read in place: the tap tables see the texture's own coordinates (k_fused_strip:surface, the real weights)
        out.append(_case("extent", f"rect_{orient}_at_{max(r[0], r[1])}_up2x_rgb32", RGB32, tex, (2 * rw, 2 * rh), 0, src_rect=r, plan="passes:",
                         fused="kernel=fused_strip:surface(", strip=True, iUpscaling=LANCZOS3, in_place=True))
    return out


# one case per route for the batch test (three frames through mpcvr_process_batch == the single frames, byte for byte)
BATCH_CASES = ("extent_up2x_taps5_w16380_p010_pq", "extent_up2x_taps4_h16380_p010_pq", "extent_jinc2x_w16384_nv12", "extent_jinc2x_w15360_p010_pq", "extent_strip_1p5x_h16384_nv12",
               "extent_period_4to3_w16380_p010_pq", "extent_same_size_w16384_16384x8_p010_pq", "extent_same_size_w16380_16378x8_p010_pq",
               "extent_down_2p5x_hamming_w16384_p010_pq")

FAMILIES = {"ladder": _ladder(), "refused": _refused(), "strip": _strip_edges(), "gates": _gates(), "bigup": _big_up(), "extent": _extents()}
CASES = {c["name"]: c for cases in FAMILIES.values() for c in cases}
assert len(CASES) == sum(len(v) for v in FAMILIES.values()), "case names are unique"


def source_size(c):
    """(w1, h1) of the rect the draws read"""
    r = c.get("src_rect", (0, 0, c["w"], c["h"]))
    return r[2] - r[0], r[3] - r[1]


def resizers(c):
    """((kind, method) of the X draw, of the Y draw): kind 1 = the upscaler, 2 = the downscaler, 0 = none (DecidePlan, vp_plan.cpp: the
    downscaler where the source is more than k times the target, k = 2 with bInterpolateAt50pct)."""
    k = 2 if c.get("bInterpolateAt50pct", 1) else 1
    up, down = c.get("iUpscaling", 2), c.get("iDownscaling", 2)
    (w1, h1), (w2, h2) = source_size(c), c["dst"]
    pick = lambda a, b: (0, 0) if a == b else (2, down) if a > k * b else (1, up)
    return pick(w1, w2), pick(h1, h2)


def axis_geometry(c, axis):
    """(src_l, src_len, n_out, tex_len) of the resize draw along screen axis "x" / "y" as BuildPlanTables hands them to BuildAxisTaps: the convert
    draw's output is rect-sized with the rect at its origin; an interleaved RGB sample without a convert draw is read in place (X draw), and
    the second draw of a two-draw resize reads m_TexResize"""
    a = 0 if axis == "x" else 1
    r = c.get("src_rect", (0, 0, c["w"], c["h"]))
    length = r[2 + a] - r[a]
    in_place = c["cformat"] in (RGB32, R210) and (axis == "x" or resizers(c)[0][0] == 0)
    return (r[a], length, c["dst"][a], (c["w"], c["h"])[a]) if in_place else (0, length, c["dst"][a], length)


def groups(family, size):
    """the family's cases in groups of at most `size` -> [(id, [case, ...])] for pytest.mark.parametrize"""
    cases = FAMILIES[family]
    return [(f"{family}_{i // size}", cases[i:i + size]) for i in range(0, len(cases), size)]
