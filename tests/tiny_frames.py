"""The smallest frames every fused route accepts: the case table and helpers of tests/test_tiny_frames.py (CPU) and
tests/test_tiny_frames_gpu.py (GPU).  Importable without a GPU.

Every fused kernel has a size gate (FusedUp2xSupported: source >= 8 x 8; ConvertBlocksSupported / FusedStripSupported: >= 8 x 2; surface
mode: >= 1 x 1; PlanFusedPeriod: two output columns, one output row).  The cases sit AT the gate, one step above it and one step below it
(`below_gate`: the fused kernel must step aside and the frame must still be right).  At these sizes the halo of a filter is wider than what
is left of the frame, both edge clamps act inside one tap window, a 128-column strip holds 8 live columns and the row prefetches and
register windows run past the frame.

A case is a dict in the style of tests/golden/cases.py plus:
    name         unique, family first
    plan         what api.plan_describe must start with (the planner-level name: fused_up2x, fused_jinc2x, direct:, passes:)
    route        fragments GetVPInfo of the `tight` render-target layout must ALL show on the default tier
    no_route     fragments it must NOT show (below the gate: no fused name)
    below_gate   the case sits one step below its family's gate
    period       (P, Q, taps) of the periodic plan the case is meant for
    strip        True: api.plan_strip must accept the geometry; False: it must refuse it (absent: not a strip family case)
Content is "noise" (every pixel matters) plus one "hdr" frame per HDR family.
"""
from tests.golden.cases import HDR10, HLG, M709, MPEG2, TV, ext

SDR = ext(matrix=M709)
TVONLY = ext(MPEG2, TV)
NV12, P010, YUY2, AYUV, YV12, YV24, YUV420P10, RGB32, R210, Y8 = 1, 2, 4, 11, 14, 16, 20, 30, 32, 37
MITCHELL, CATMULL, LANCZOS2, LANCZOS3, JINC2, SPLINE36 = 1, 2, 3, 4, 5, 6
FLAG_LANCZOS3_FIXED = 1           # (= api.FLAG_LANCZOS3_FIXED: six taps; no library is loaded to import this table)

FUSED_NAMES = ("fused_up2x", "fused_jinc2x", "kernel=fused_strip", "kernel=fused_period")

# the formats and tails of the exact-2x and any-ratio families: (tag, cformat, exfmt)
FORMATS_AND_TAILS = (("p010_pq", P010, HDR10), ("p010_hlg", P010, HLG), ("p010_sdr", P010, SDR), ("nv12", NV12, SDR), ("yuv420p10", YUV420P10, SDR),
                     ("yv12", YV12, SDR), ("yuy2", YUY2, SDR), ("y8", Y8, SDR), ("yv24", YV24, SDR))
# tap counts of the separable fused kernels: 4 (Mitchell), 5 (Lanczos3 as Direct3D 11 draws it), 6 (the fixed Lanczos3; the Spline36 extension)
TAPS = {4: dict(iUpscaling=MITCHELL), 5: dict(iUpscaling=LANCZOS3), 6: dict(iUpscaling=LANCZOS3, flags=FLAG_LANCZOS3_FIXED)}

_seed = [7000]


def _case(family, tag, cformat, src, dst, exfmt=SDR, kind="noise", **kw):
    _seed[0] += 1
    c = dict(name=f"{family}_{tag}", family=family, cformat=cformat, w=src[0], h=src[1], kind=kind, seed=_seed[0], dst=tuple(dst), exfmt=exfmt)
    c.update(kw)
    return c


def _x(wh):
    return "%dx%d" % tuple(wh)


def rows_dword_aligned(cformat, w):
    """The fused convert stages load dwords: a sample at its default pitch reaches them only where the luma rows and the chroma rows of a
    three-plane format start on multiples of 4 bytes (fast_convert, CHipVideoProcessor::FillFusedParams).  NV12 and Y8 rows are padded to 4 bytes
    by the reference's default pitch; YV24 at 10 columns or YUV420P10 at 14 are not, and the planner hands those frames to a convert kernel
    of its own and the surface variants — correctly, so the table gives such formats the widths their loads can take."""
    if cformat in (NV12, Y8, AYUV, RGB32, R210):
        return True
    if cformat in (P010, YUY2):
        return (2 * w) % 4 == 0
    luma, chroma = {YV12: (w, w // 2), YV24: (w, w), YUV420P10: (2 * w, w)}[cformat]
    return luma % 4 == 0 and chroma % 4 == 0


def _up2x():
    out = []
    route = dict(plan="fused_up2x", route=("fused_up2x",))
    # every source size x every tap count behind the headline tail
    for src in ((8, 8), (10, 8), (8, 10), (14, 12)):
        for nt, over in TAPS.items():
            out.append(_case("up2x", f"p010_pq_{_x(src)}_taps{nt}", P010, src, (2 * src[0], 2 * src[1]), HDR10, **over, **route))
    out.append(_case("up2x", "p010_pq_8x8_spline36", P010, (8, 8), (16, 16), HDR10, iUpscaling=SPLINE36, **route))
    # every format and tail, the sizes and tap counts taking turns
    sizes = ((8, 8), (10, 8), (8, 10), (14, 12))
    for i, (tag, cf, ex) in enumerate(FORMATS_AND_TAILS):
        src, nt = next(sizes[(i + 1 + k) % 4] for k in range(4) if rows_dword_aligned(cf, sizes[(i + 1 + k) % 4][0])), (5, 4, 6)[i % 3]
        out.append(_case("up2x", f"{tag}_{_x(src)}_taps{nt}_formats", cf, src, (2 * src[0], 2 * src[1]), ex, **TAPS[nt], **route))
    for tag, ex in (("pq", HDR10), ("hlg", HLG)):
        out.append(_case("up2x", f"p010_{tag}_8x8_hdr_content", P010, (8, 8), (16, 16), ex, kind="hdr", iUpscaling=LANCZOS3, **route))
    # a window offset that is not a multiple of 4 (the generic epilogue) and one that is
    out.append(_case("up2x", "p010_pq_8x8_offset_3_1", P010, (8, 8), (16, 16), HDR10, iUpscaling=LANCZOS3, window=(24, 20), offset=(3, 1), **route))
    out.append(_case("up2x", "p010_pq_10x8_offset_4_3", P010, (10, 8), (20, 16), HDR10, iUpscaling=MITCHELL, window=(28, 20), offset=(4, 3), **route))
    out.append(_case("up2x", "p010_pq_8x8_out10", P010, (8, 8), (16, 16), HDR10, iUpscaling=LANCZOS3, output_format=1, **route))
    out.append(_case("up2x", "nv12_8x10_out10", NV12, (8, 10), (16, 20), SDR, iUpscaling=MITCHELL, output_format=1, **route))
    # below the gate: the planner reports `passes:`.  A source 8 wide and 2 .. 6 high is still k_fused_strip's (its own gate is 8 x 2):
    # the exact-2x kernel steps aside, the any-ratio kernel draws the frame; 6 x 8 is below both gates on raw samples: a convert kernel of its
    # own, then the any-ratio kernel's surface variant (whose gate is 1 x 1) — no two-draw resize leaves the fused kernels for its size alone
    for src, frag, no in (((8, 6), ("passes:", "kernel=fused_strip("), ("fused_up2x",)), ((8, 2), ("passes:", "kernel=fused_strip("), ("fused_up2x",)),
                          ((6, 8), ("passes:", "kernel=fused_strip:surface("), ("fused_up2x", "kernel=fused_strip("))):
        for tag, cf in (("p010_sdr", P010), ("nv12", NV12)):
            out.append(_case("up2x", f"{tag}_{_x(src)}_below_gate", cf, src, (2 * src[0], 2 * src[1]), SDR, iUpscaling=LANCZOS3, plan="passes:", route=frag,
                             no_route=no, below_gate=True))
    return out


def _jinc2x():
    out = []
    for src in ((8, 8), (10, 8), (8, 10)):
        for tag, cf, ex in (("p010_pq", P010, HDR10), ("nv12", NV12, SDR), ("p010_sdr", P010, SDR)):
            out.append(_case("jinc2x", f"{tag}_{_x(src)}", cf, src, (2 * src[0], 2 * src[1]), ex, iUpscaling=JINC2, plan="fused_jinc2x", route=("fused_jinc2x",)))
    out.append(_case("jinc2x", "p010_pq_8x8_hdr_content", P010, (8, 8), (16, 16), HDR10, kind="hdr", iUpscaling=JINC2, plan="fused_jinc2x", route=("fused_jinc2x",)))
    for tag, cf in (("p010_sdr", P010), ("nv12", NV12)):
        out.append(_case("jinc2x", f"{tag}_6x6_below_gate", cf, (6, 6), (12, 12), SDR, iUpscaling=JINC2, plan="passes:", route=("passes:",), no_route=FUSED_NAMES,
                         below_gate=True))
    return out


def _same_size():
    out = []
    route = dict(plan="direct:", route=("direct:",), no_route=("kernel=",))
    # width % 4 == 0: the streaming kernel's condition (P01x / NV12); 10 and 14 wide: k_convert_blocks
    for src in ((8, 2), (8, 4), (12, 2), (10, 2), (14, 6)):
        out.append(_case("same", f"p010_pq_{_x(src)}", P010, src, src, HDR10, **route))
        out.append(_case("same", f"nv12_{_x(src)}", NV12, src, src, SDR, **route))
    for tag, cf, ex in (("p010_hlg", P010, HLG), ("p010_sdr", P010, SDR), ("yuv420p10", YUV420P10, SDR), ("yuy2", YUY2, SDR), ("y8", Y8, SDR), ("ayuv", AYUV, SDR)):
        for src in ((8, 2), (10, 2)):
            src = src if rows_dword_aligned(cf, src[0]) else (12, 2)        # (YUV420P10: the chroma rows of 10 columns are 10 bytes)
            out.append(_case("same", f"{tag}_{_x(src)}", cf, src, src, ex, **route))
    for tag, ex in (("pq", HDR10), ("hlg", HLG)):
        out.append(_case("same", f"p010_{tag}_8x2_hdr_content", P010, (8, 2), (8, 2), ex, kind="hdr", **route))
    # Catmull-Rom chroma on 4:2:0 (four chroma rows and columns under every pixel: all clamped in a frame with one chroma row)
    out.append(_case("same", "p010_pq_8x2_catmull_chroma", P010, (8, 2), (8, 2), HDR10, iChromaScaling=2, **route))
    out.append(_case("same", "nv12_10x4_catmull_chroma", NV12, (10, 4), (10, 4), SDR, iChromaScaling=2, **route))
    # Dolby Vision: polynomial reshaping; MMR + a level-2 trim
    out.append(_case("same", "p010_dovi_poly_8x2", P010, (8, 2), (8, 2), TVONLY, kind="hdr", dovi=dict(kind="poly"), **route))
    out.append(_case("same", "p010_dovi_mmr_l2_10x4", P010, (10, 4), (10, 4), TVONLY, kind="hdr", dovi=dict(kind="mmr", l2=(100,)), hdr_display=1000.0, **route))
    # below the gate: the planner-level name stays `direct:` (the per-pixel k_convert_direct draws the frame; GetVPInfo has one name for the
    # three kernels of a same-size frame), SDR content: bit-exact with the oracle
    for src in ((6, 2), (4, 4)):
        for tag, cf in (("p010_sdr", P010), ("nv12", NV12)):
            out.append(_case("same", f"{tag}_{_x(src)}_below_gate", cf, src, src, SDR, plan="direct:", route=("direct:",), no_route=("kernel=",), below_gate=True))
    return out


# every (P, Q) the periodic-phase kernel is built for, at the smallest frames the planner accepts.  An odd output width sits in a window one
# pixel wider: k_fused_period stores 8 bytes per lane and wants a row pitch that is a multiple of 8, which a tight target of 11 pixels is not.
# (8 x 2 -> 3 x 1 is NOT one of them: mpcvr_plan_period takes it as 1:2, but 8 columns onto 3 is more than 2:1, so the X draw is the
# downscaler's and the processor plans no periodic kernel — the geometry is k_fused_strip's and sits in that family)
PERIOD_GEOMETRIES = (
    ((4, 3), (8, 6), (11, 8)), ((4, 3), (12, 6), (16, 8)),
    ((3, 2), (8, 2), (12, 3)), ((3, 2), (8, 2), (11, 3)), ((3, 2), (8, 4), (12, 6)),
    ((2, 3), (12, 6), (8, 4)),
    ((1, 2), (8, 2), (4, 1)), ((1, 2), (8, 4), (5, 2)),
    ((3, 1), (8, 2), (24, 6)), ((3, 1), (8, 4), (24, 12)),
)
PERIOD_TAILS_AND_TAPS = (("p010_pq_lanczos3", P010, HDR10, LANCZOS3, 5), ("p010_hlg_lanczos3", P010, HLG, LANCZOS3, 5),
                         ("p010_pq_mitchell", P010, HDR10, MITCHELL, 4), ("nv12_lanczos3", NV12, SDR, LANCZOS3, 5))


def _period():
    out = []
    for (P, Q), src, dst in PERIOD_GEOMETRIES:
        for tag, cf, ex, up, nt in PERIOD_TAILS_AND_TAPS:
            over = dict(window=(dst[0] + 1, dst[1])) if dst[0] & 1 else {}
            out.append(_case("period", f"{tag}_{P}to{Q}_{_x(src)}_to_{_x(dst)}", cf, src, dst, ex, iUpscaling=up, plan="passes:", period=(P, Q, nt), strip=True,
                             route=("passes:", f"kernel=fused_period(rows={P}:{Q},taps={nt},"), **over))
    out.append(_case("period", "p010_pq_lanczos3_3to2_8x2_to_12x3_hdr_content", P010, (8, 2), (12, 3), HDR10, kind="hdr", iUpscaling=LANCZOS3, plan="passes:",
                     period=(3, 2, 5), strip=True, route=("passes:", "kernel=fused_period(rows=3:2,taps=5,")))
    return out


def _strip():
    out = []
    route = dict(plan="passes:", route=("passes:", "kernel=fused_strip("), strip=True)
    geos = (("8x2_to_9x5", (8, 2), (9, 5), dict(iUpscaling=LANCZOS3)), ("10x4_to_13x5", (10, 4), (13, 5), dict(iUpscaling=MITCHELL)),
            ("8x2_to_12x2_one_axis", (8, 2), (12, 2), dict(iUpscaling=LANCZOS3)),
            ("14x6_to_9x5_hamming", (14, 6), (9, 5), dict(iDownscaling=2, bInterpolateAt50pct=0)),
            ("14x6_to_9x5_bicubic", (14, 6), (9, 5), dict(iDownscaling=3, bInterpolateAt50pct=0)),
            ("16x2_to_7x1", (16, 2), (7, 1), dict(iDownscaling=2, iUpscaling=CATMULL)),
            ("8x2_to_3x1", (8, 2), (3, 1), dict(iDownscaling=2, iUpscaling=LANCZOS3)))        # (X: Hamming, 8 > 2 * 3; Y: Lanczos3 at 1:2, one output row)
    # one axis only (8 x 2 -> 12 x 2): the processor plans the any-ratio kernel for two-draw resizes only, so this geometry is drawn by the
    # block convert and the folded row kernel — no fused resize name, held to the same bar
    one_axis = dict(plan="passes:", route=("passes:convert,resizeX",), no_route=FUSED_NAMES, one_axis=True)
    # every geometry behind the headline tail and from NV12, every format and tail with the geometries taking turns
    for gtag, src, dst, over in geos:
        r = one_axis if "one_axis" in gtag else route
        out.append(_case("strip", f"p010_pq_{gtag}", P010, src, dst, HDR10, **over, **r))
        out.append(_case("strip", f"nv12_{gtag}", NV12, src, dst, SDR, **over, **r))
    for i, (tag, cf, ex) in enumerate(FORMATS_AND_TAILS):
        if tag in ("p010_pq", "nv12"):
            continue
        ok = [g for g in geos if rows_dword_aligned(cf, g[1][0])]
        for gtag, src, dst, over in (ok[i % len(ok)], ok[(i + 3) % len(ok)]):
            out.append(_case("strip", f"{tag}_{gtag}", cf, src, dst, ex, **over, **(one_axis if "one_axis" in gtag else route)))
    for tag, ex in (("pq", HDR10), ("hlg", HLG)):
        out.append(_case("strip", f"p010_{tag}_8x2_to_9x5_hdr_content", P010, (8, 2), (9, 5), ex, kind="hdr", iUpscaling=LANCZOS3, **route))
    # below the gate (a source 6 wide): the convert stage declines (FusedStripSupported; the tables fit) — a convert kernel of its own, then the
    # surface variant
    for tag, cf in (("p010_sdr", P010), ("nv12", NV12)):
        out.append(_case("strip", f"{tag}_6x2_to_9x5_below_gate", cf, (6, 2), (9, 5), SDR, iUpscaling=LANCZOS3, plan="passes:",
                         route=("passes:", "kernel=fused_strip:surface("), no_route=("kernel=fused_strip(",), below_gate=True, strip=True))
    return out


def _surface():
    out = []
    for tag, cf in (("rgb32", RGB32), ("r210", R210)):
        # (interleaved RGB has no convert draw: the source texture itself is the surface.  2 x 1 -> 3 x 1 is one axis only — see _strip — and
        # runs the plain row kernel)
        out.append(_case("surface", f"{tag}_1x1_to_3x5", cf, (1, 1), (3, 5), 0, iUpscaling=LANCZOS3, plan="passes:", strip=True, route=("passes:", "kernel=fused_strip:surface(")))
        out.append(_case("surface", f"{tag}_2x1_to_3x1", cf, (2, 1), (3, 1), 0, iUpscaling=MITCHELL, plan="passes:", route=("passes:",), no_route=FUSED_NAMES, one_axis=True))
        # 3 x 3 -> 4 x 4 and 5 x 3 -> 8 x 4 are 4:3 down the rows: the periodic-phase kernel's surface variant
        for src, dst in (((3, 3), (4, 4)), ((5, 3), (8, 4))):
            out.append(_case("surface", f"{tag}_{_x(src)}_to_{_x(dst)}", cf, src, dst, 0, iUpscaling=LANCZOS3, plan="passes:", strip=True, period=(4, 3, 5),
                             route=("passes:", "kernel=fused_period:surface(rows=4:3,taps=5,")))
        out.append(_case("surface", f"{tag}_5x3_to_7x5", cf, (5, 3), (7, 5), 0, iUpscaling=LANCZOS3, plan="passes:", strip=True, route=("passes:", "kernel=fused_strip:surface(")))
    # a planar sample whose source rect is off the 4 x 2 grid of the fused convert stage: the convert draw is a kernel of its own
    for tag, cf, ex in (("p010_pq", P010, HDR10), ("nv12", NV12, SDR)):
        out.append(_case("surface", f"{tag}_rect_off_grid_10x6_to_13x7", cf, (16, 10), (13, 7), ex, src_rect=(3, 1, 13, 7), iUpscaling=LANCZOS3, plan="passes:convert",
                         strip=True, route=("passes:convert", "kernel=fused_strip:surface(")))
    return out


def _plain():
    """1 x 1 .. 3 x 2 sources through all six upscalers and all six downscalers to 1 x 1, 2x, 3x and 7 x 3, every rotation of one of them.
    The family's tier is MPCVR_FLAG_NO_FUSED (`passes:`, bit-exact); the default tier draws them too, with whatever the planner picks."""
    out = []
    sources = ((1, 1), (1, 5), (5, 1), (2, 2), (3, 2))
    formats = (("rgb32", RGB32, 0), ("y8", Y8, SDR), ("yv24", YV24, SDR), ("nv12", NV12, SDR), ("p010", P010, SDR))
    n = 0
    for src in sources:
        for dst in ((1, 1), (2 * src[0], 2 * src[1]), (3 * src[0], 3 * src[1]), (7, 3)):
            if dst == src:
                continue
            for k in range(2):              # two formats and two scalers per geometry, taking turns: every scaler meets every source size
                tag, cf, ex = formats[n % (5 if src == (2, 2) else 3)]
                up, down = n % 6, (n // 2) % 6
                n += 1
                out.append(_case("plain", f"{tag}_{_x(src)}_to_{_x(dst)}_up{up}_down{down}", cf, src, dst, ex, iUpscaling=up, iDownscaling=down,
                                 bInterpolateAt50pct=n % 2, plan="passes:", route=("passes:",)))
    for down in range(6):                   # every downscaler really drawing (above, the ratio decides whether the setting is used)
        tag, cf, ex = formats[down % 3]
        src, dst = (((5, 1), (2, 1)), ((1, 5), (1, 2)), ((3, 2), (1, 1)))[down % 3]
        out.append(_case("plain", f"{tag}_{_x(src)}_to_{_x(dst)}_downscaler{down}", cf, src, dst, ex, iUpscaling=CATMULL, iDownscaling=down, bInterpolateAt50pct=0,
                         plan="passes:", route=("passes:",)))
    for rot in (90, 180, 270):
        dst = (6, 9) if rot in (90, 270) else (9, 6)
        out.append(_case("plain", f"yv24_3x2_to_{_x(dst)}_rot{rot}", YV24, (3, 2), dst, SDR, iUpscaling=LANCZOS3, rotation=rot, plan="passes:", route=("passes:",)))
    out.append(_case("plain", "rgb32_3x2_to_9x6_flip", RGB32, (3, 2), (9, 6), 0, iUpscaling=CATMULL, flip=1, plan="passes:", route=("passes:",)))
    return out


# ---- error diffusion (bUseDither = 2): P010 frames whose diffused rect (video rect ∩ window) is `rect` wide and high.  Bands are 21 rows and
# two columns of skew from row to row: 21 / 22 and 42 / 43 rows straddle a hand-off, and in a rect 1 .. 3 wide the skew exceeds the width
def _errdiff():
    ed = dict(bUseDither=2)
    return [
        _case("errdiff", "1x1_clipped_same_size", P010, (8, 8), (8, 8), SDR, window=(4, 3), offset=(3, -7), rect=(1, 1), plan="direct:", **ed),
        _case("errdiff", "1x50_clipped_same_size", P010, (8, 50), (8, 50), HDR10, window=(6, 54), offset=(5, 2), rect=(1, 50), plan="direct:", **ed),
        _case("errdiff", "70x1_clipped_same_size", P010, (70, 8), (70, 8), SDR, window=(74, 4), offset=(2, -7), rect=(70, 1), plan="direct:", **ed),
        _case("errdiff", "2x22_same_size", P010, (2, 22), (2, 22), SDR, rect=(2, 22), plan="direct:", **ed),
        _case("errdiff", "3x21_clipped_same_size", P010, (4, 22), (4, 22), HDR10, window=(5, 23), offset=(2, -1), rect=(3, 21), plan="direct:", **ed),
        _case("errdiff", "8x43_clipped_2x", P010, (8, 22), (16, 44), HDR10, iUpscaling=LANCZOS3, window=(8, 43), offset=(-4, 0), rect=(8, 43), plan="passes:", **ed),
        _case("errdiff", "9x2_clipped_same_size", P010, (10, 2), (10, 2), SDR, window=(9, 2), rect=(9, 2), plan="direct:", **ed),
        _case("errdiff", "16x16_exact_2x", P010, (8, 8), (16, 16), HDR10, iUpscaling=LANCZOS3, rect=(16, 16), plan="fused_up2x", **ed),
        _case("errdiff", "8x2_same_size", P010, (8, 2), (8, 2), HDR10, rect=(8, 2), plan="direct:", **ed),
    ]


FAMILIES = {"up2x": _up2x(), "jinc2x": _jinc2x(), "same": _same_size(), "period": _period(), "strip": _strip(), "surface": _surface(), "plain": _plain(),
            "errdiff": _errdiff()}
CASES = {c["name"]: c for cases in FAMILIES.values() for c in cases}
assert len(CASES) == sum(len(v) for v in FAMILIES.values()), "case names are unique"

# one gate-size case per fused family: what the sample's neighbours do, and batches
GATE_CASES = ("up2x_p010_pq_8x8_taps5", "jinc2x_p010_pq_8x8", "same_p010_pq_8x2", "same_nv12_10x2", "period_p010_pq_lanczos3_3to2_8x2_to_12x3",
              "period_p010_pq_lanczos3_1to2_8x2_to_4x1", "strip_p010_pq_8x2_to_9x5", "surface_rgb32_1x1_to_3x5", "surface_r210_3x3_to_4x4")


def source_size(c):
    """(w1, h1) of the rect the draws read"""
    r = c.get("src_rect", (0, 0, c["w"], c["h"]))
    return r[2] - r[0], r[3] - r[1]


def resizers(c):
    """((kind, method) of the X draw, of the Y draw): kind 1 = the upscaler, 2 = the downscaler, 0 = none (DecidePlan, vp_plan.cpp: the
    downscaler where the source is more than k times the target, k = 2 with bInterpolateAt50pct).  Unrotated cases."""
    k = 2 if c.get("bInterpolateAt50pct", 1) else 1
    up, down = c.get("iUpscaling", 2), c.get("iDownscaling", 2)       # (the settings' defaults: Catmull-Rom, Hamming)
    (w1, h1), (w2, h2) = source_size(c), c["dst"]
    pick = lambda a, b: (0, 0) if a == b else (2, down) if a > k * b else (1, up)
    return pick(w1, w2), pick(h1, h2)


def groups(family, size):
    """the family's cases in groups of at most `size` -> [(id, [case, ...])] for pytest.mark.parametrize"""
    cases = FAMILIES[family]
    return [(f"{family}_{i // size}", cases[i:i + size]) for i in range(0, len(cases), size)]
