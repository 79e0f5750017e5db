"""Every launch the gate of k_fused_up2x_bp (FusedUp2xBpTakes, csrc/vp_fused_up2x_bp.hip) admits, and its neighbours that it must refuse:
the case table of tests/test_up2x_bp_cases.py (CPU) and tests/test_up2x_bp_sweep_gpu.py (GPU).  Importable without a GPU.

The twin stands on a lane identity (lane j takes the chroma of its odd column from lane j + 1; lane 63 has no neighbour), a row identity
(chroma row n + 1 of an iteration is carried into the next one; a segment's first convert loads both rows) and the host gate that decides
once per launch whether both hold.  The rows below walk the geometry those three depend on:

  * strips are S = 120 source columns, lane l of a strip converts rect columns X = x0 - 4 + 2l, x0 = (blockIdx.x * 4 + wave) * 120.  The
    lane that owns the rect's last block (X == W - 2) is (W - x0) / 2 + 1: lanes 2 .. 61 in the last strip, lanes 62 and 63 in the strip in
    front of a last strip of 2 and of 4 columns (W = 122, 124, 242, 244, 482, 484).  `edge_wave` (x0 == 0 || x0 + 122 > W - 2) is on in
    front of a 2-column last strip and off in front of a 4-column one unless the strip is the frame's first;
  * the fifth strip (W > 480) starts a second workgroup;
  * LaunchFusedUp2x cuts a single small frame into 24-row segments (no candidate of its ladder 180 .. 36 gives strips x segments >= 3,840
    waves, so the loop ends at 24): seams at source rows 24 and 48, a last segment of H - 24 or H - 48 rows.  A batch takes the cheapest
    rounds x (rows + 6) instead: 3 frames of 124 x 200 are 2 strips x ceil(200 / cand) x 3 items — one round of the resident waves for
    every candidate, so the cost is cand + 6 and the shortest one wins: 24-row segments, seams at 24, 48, .. 192, a last segment of 8 rows;
    33 / 34 frames of 64 x 8 are one segment each (every candidate costs min(cand, 8) + 6; the first stays, cut to 8 rows);
  * a source rect with rect_l = 4, 8, 120, 124 whose right edge is the frame's: the left-edge lanes clamp to the rect, c0 = (rect_l + Xg) / 2;
    rect_l = 2, 6 switch `fast_convert` off (CHipVideoProcessor::FillFusedParams: rect_l % 4 == 0), and with it FusedUp2xSupported — UpdatePlan
    then plans no exact-2x kernel at all: a convert kernel of its own and the surface variant of the any-ratio kernel draw the frame;
  * a batch above 32 frames leaves the by-value frame table of the kernel arguments for the one in device memory.

A row is a case dict in the style of tests/golden/cases.py (make_vp / case_frame / oracle_params read it) plus
    name      unique, group first
    group     the parametrised GPU test the row belongs to
    form      "bp", "generic", or None where no exact-2x kernel runs (GetUp2xForm)
    route     fragments GetVPInfo must all show; no_route: fragments it must not show
    why       one line
    batch     frames of a ProcessBatch call cycling through three distinct samples (absent: one frame through Process)
    sample_off / target_off   the first byte of the sample / of the render target this many bytes behind a 256-byte boundary
P016 is served: FusedSourceKind (csrc/vp_fused.hip) returns SRC_P01X for every bi-planar 16-bit format (`biplanar_fast && c.fmt.bytes == 2`).
"""
from tests.golden.cases import COSITED, HDR10, HLG, M709, M2020, MPEG1, P2020, TPQ, TV, ext

SDR = ext(matrix=M709)
NV12, P010, P016 = 1, 2, 3
CATMULL, LANCZOS3 = 2, 4
TAPS = {4: dict(iUpscaling=CATMULL), 5: dict(iUpscaling=LANCZOS3), 6: dict(iUpscaling=LANCZOS3, flags=1)}      # (flags=1: MPCVR_FLAG_LANCZOS3_FIXED)
PLANS = {
    "p010_pq_dither8": dict(cformat=P010, exfmt=HDR10),
    "nv12_fast_direct10": dict(cformat=NV12, exfmt=SDR, iTexFormat=10, output_format=1),
    "p010_hlg_dither8": dict(cformat=P010, exfmt=HLG),
    "p010_pq_direct10": dict(cformat=P010, exfmt=HDR10, output_format=1),
}

S, WAVES, LANES = 120, 4, 64                   # csrc/vp_fused_dev.h
SMALL_FRAME = 64 * 40                          # source pixels below which a frame's identical-channel share is pooled per test
SEGMENT_LADDER = (180, 144, 120, 108, 90, 72, 60, 48, 36, 24)

WIDTHS = tuple(range(8, 132, 2)) + tuple(range(236, 252, 2)) + tuple(range(478, 488, 2))
WIDTHS_OTHER_PLANS = (8, 10, 118, 120, 122, 124, 126, 242, 244, 482, 484)
HEADLINE_WIDTHS = (1920, 3840)
HEIGHTS = tuple(range(8, 58, 2))
HEIGHT_WIDTHS = (64, 124)
SEAM_ROWS = (24, 48)                           # source rows at which a single frame of the height rows starts a new segment

UP2X = dict(route=("fused_up2x",), no_route=())
_seed = [9600]


def _row(group, tag, plan, w, h, form, why, taps=5, **kw):
    _seed[0] += 1
    c = dict(PLANS[plan] if isinstance(plan, str) else plan, name=f"{group}_{tag}", group=group, w=w, h=h, kind="noise", seed=_seed[0], form=form, why=why)
    c.update(TAPS[taps])
    c.update(kw)
    if "dst" not in c:
        l, t, r, b = c.get("src_rect", (0, 0, w, h))
        c["dst"] = (2 * (r - l), 2 * (b - t))
    if "route" not in c:
        c.update(UP2X)
    return c


def _widths():
    out = []
    for w in WIDTHS:
        out.append(_row("widths_p010_pq_dither8", f"{w}x24", "p010_pq_dither8", w, 24, "bp", f"W = {w}: one segment, 15 iterations, the last block's lane and the strips of this width"))
    for w in HEADLINE_WIDTHS:
        out.append(_row("widths_headline", f"{w}x8", "p010_pq_dither8", w, 8, "bp", f"the headline width {w} must never lose the twin"))
    for plan in ("nv12_fast_direct10", "p010_hlg_dither8", "p010_pq_direct10"):
        for w in WIDTHS_OTHER_PLANS:
            out.append(_row(f"widths_{plan}", f"{w}x24", plan, w, 24, "bp", f"W = {w} on the {plan} instantiation"))
    return out


def _heights():
    out = []
    for w in HEIGHT_WIDTHS:
        for h in HEIGHTS:
            n = (h + 23) // 24
            out.append(_row(f"heights_{w}", f"{w}x{h}", "p010_pq_dither8", w, h, "bp",
                            f"H = {h}: {n} segment(s) of 24 rows, seams at {[s for s in SEAM_ROWS if s < h]}, a last segment of {h - 24 * (n - 1)} rows"))
        out.append(_row(f"heights_{w}", f"{w}x6_refused", "p010_pq_dither8", w, 6, None, "H = 6 is below FusedUp2xSupported's eight rows: k_fused_strip draws the frame",
                        route=("passes:", "kernel=fused_strip("), no_route=("fused_up2x",)))
    return out


def _rects():
    out = []
    for w in (248, 132):
        for l in (4, 8, 120, 124):
            why = f"rect_l = {l} on a {w}-wide frame: the left-edge lanes clamp to the rect, c0 = (rect_l + Xg) / 2"
            if (w, l) == (248, 124):
                why += "; rect width 124: lane 63 owns the last block of a rect that does not start at 0"
            out.append(_row("rects", f"{w}_left{l}", "p010_pq_dither8", w, 24, "bp", why, src_rect=(l, 0, w, 24)))
        for l in (2, 6):
            out.append(_row("rects", f"{w}_left{l}_refused", "p010_pq_dither8", w, 24, None,
                            f"rect_l = {l}: rect_l % 4 != 0 turns fast_convert off, FusedUp2xSupported refuses, UpdatePlan plans no exact-2x kernel",
                            src_rect=(l, 0, w, 24), route=("passes:convert", "kernel=fused_strip:surface("), no_route=("fused_up2x",)))
    out.append(_row("rects", "132_left4_x40_seam", "p010_pq_dither8", 132, 40, "bp", "left edge x seam: rect_l = 4 with a second segment at row 24", src_rect=(4, 0, 132, 40)))
    return out


def _settings():
    out = []
    out.append(_row("settings", "procamp_all_124x40", "p010_pq_dither8", 124, 40, "bp", "brightness, contrast and saturation keep m[1] == m[8] == 0: the twin with a non-default matrix",
                    procamp=(10.0, 1.2, 0.0, 1.3)))
    for tag, pa in (("brightness", (10.0, 1.0, 0.0, 1.0)), ("contrast", (0.0, 1.2, 0.0, 1.0)), ("saturation", (0.0, 1.0, 0.0, 1.3))):
        out.append(_row("settings", f"procamp_{tag}_64x24", "p010_pq_dither8", 64, 24, "bp", f"{tag} alone: no hue rotation, the structural zeros stay", procamp=pa))
    for taps in (4, 6):
        for w in (122, 124):
            out.append(_row("settings", f"taps{taps}_{w}x26", "p010_pq_dither8", w, 26, "bp", f"{taps} taps at W = {w} (lane {w // 2 + 1} owns the last block), a 2-row last segment",
                            taps=taps))
    # six taps are the only count whose stage X reads A column 126, lane 63's even column: lanes 62 / 63 behind a first strip as well
    for w in (242, 244):
        out.append(_row("settings", f"taps6_{w}x26", "p010_pq_dither8", w, 26, "bp", f"6 taps at W = {w} (lane {(w - 120) // 2 + 1} of the second strip owns the last block)", taps=6))
    out.append(_row("settings", "p016_124x26", dict(cformat=P016, exfmt=HDR10), 124, 26, "bp", "P016: FusedSourceKind maps every bi-planar 16-bit format to SRC_P01X"))
    out.append(_row("settings", "padded_pitch_124x24", "p010_pq_dither8", 124, 24, "bp", "row pitch 248 + 64 bytes", pitch=312))
    out.append(_row("settings", "sample_at_plus4_124x24", "p010_pq_dither8", 124, 24, "bp", "the sample's first byte 4 bytes behind a 256-byte boundary", sample_off=4))
    return out


def _refusals():
    r = []
    r.append(_row("refusals", "target_at_plus4", "p010_pq_dither8", 124, 24, "generic", "a target whose first byte is at +4 leaves the aligned epilogues (EPI_GENERIC: no twin instantiation)",
                  target_off=4))
    r.append(_row("refusals", "window_clipped", "p010_pq_dither8", 124, 24, None, "a video rect the window clips: DecidePlan keeps the exact-2x kernels for rects inside the window",
                  window=(248 - 10, 48 - 6), offset=(-4, -2), route=("passes:",), no_route=("fused_up2x",)))
    r.append(_row("refusals", "cosited", dict(cformat=P010, exfmt=ext(COSITED, TV, M2020, P2020, TPQ)), 124, 24, "generic",
                  "co-sited chroma: vk3 = 0, the clamped rows above the rect repeat rows (0, 1) — the row identity fails"))
    r.append(_row("refusals", "mpeg1", dict(cformat=P010, exfmt=ext(MPEG1, TV, M2020, P2020, TPQ)), 124, 24, "generic",
                  "MPEG-1 chroma is centred horizontally (center_h; FusedSourceKind: SRC_GENERIC): the odd column is not the mean of c0 and c0 + 1"))
    r.append(_row("refusals", "nearest_chroma", "p010_pq_dither8", 124, 24, "generic", "iChromaScaling nearest: cw_own = 1, one chroma row per row pair", iChromaScaling=0))
    r.append(_row("refusals", "catmull_chroma", "p010_pq_dither8", 124, 24, None, "Catmull-Rom chroma is no layout of the exact-2x kernels (DecidePlan: fused_layout)",
                  iChromaScaling=2, route=("passes:",), no_route=("fused_up2x",)))
    return r


def _batches():
    out = []
    for n in (33, 34):
        out.append(_row("batches", f"{n}_frames_64x8", "p010_pq_dither8", 64, 8, "bp", f"{n} frames: past the 32 rows of the by-value frame table, one 8-row segment each", batch=n,
                        seed=9990))          # (one seed: both batches cycle through the same three samples)
    out.append(_row("batches", "3_frames_124x200", "p010_pq_dither8", 124, 200, "bp", "3 frames of 2 strips: the batch cost rule takes 24-row segments, seams at 24 .. 192, a last segment of 8 rows",
                    batch=3))
    return out


ROWS = _widths() + _heights() + _rects() + _settings() + _refusals() + _batches()
CASES = {c["name"]: c for c in ROWS}
assert len(CASES) == len(ROWS), "row names are unique"
GROUPS = sorted({c["group"] for c in ROWS})


def rows_of(group):
    return [c for c in ROWS if c["group"] == group]


def chunks(group, size):
    """the group's rows in chunks of at most `size` -> [(id, [row, ..])] for pytest.mark.parametrize"""
    rows = rows_of(group)
    return [(f"{group}_{i // size}", rows[i:i + size]) for i in range(0, len(rows), size)]


def rect_of(c):
    """(rect_l, rect_t, W, H) of the rect the kernel reads"""
    l, t, r, b = c.get("src_rect", (0, 0, c["w"], c["h"]))
    return l, t, r - l, b - t


def is_small(c):
    _, _, w, h = rect_of(c)
    return w * h < SMALL_FRAME


# ---- the kernel's own strip arithmetic (csrc/vp_fused_up2x.h: fused_up2x_body) ----
def strips(W):
    """[(strip index, blockIdx.x, x0, edge_wave)] of a rect W columns wide"""
    out = []
    for k in range((W + S - 1) // S):
        x0 = k * S
        out.append((k, k // WAVES, x0, x0 == 0 or x0 + 2 * 63 - 4 > W - 2))
    return out


def last_block_lanes(W):
    """{strip index: lane} of every lane whose block is the rect's last one unclamped: X = x0 - 4 + 2 * lane == W - 2"""
    out = {}
    for k, _, x0, _ in strips(W):
        lane, odd = divmod(W - 2 - x0 + 4, 2)
        if not odd and 0 <= lane < LANES:
            out[k] = lane
    return out


# ---- LaunchFusedUp2x's segment rule (csrc/vp_fused.hip) ----
def segment_rows(W, H, n_frames=1, inflight=1, cus=256):
    """seg_rows of a launch: the single-frame ladder, the batch cost rule (resident waves: 4 SIMDs x 3 waves per compute unit), even, at most H"""
    n_strips = (W + S - 1) // S
    side = n_frames * max(inflight, 1)
    want = 12288 if n_frames > 1 else 3840
    seg = 24
    for cand in SEGMENT_LADDER:
        if n_strips * ((H + cand - 1) // cand) * side >= want or cand == 24:
            seg = cand
            break
    if n_frames > 1:
        resident, best = cus * 4 * 3, -1
        for cand in SEGMENT_LADDER:
            items = n_strips * ((H + cand - 1) // cand) * side
            cost = ((items + resident - 1) // resident) * (min(cand, H) + 6)
            if best < 0 or cost < best:
                best, seg = cost, cand
    seg = (seg + 1) & ~1
    return min(seg, H)


def segments(W, H, n_frames=1):
    """[(s0, s1)] of a launch"""
    seg = segment_rows(W, H, n_frames)
    return [(s0, min(s0 + seg, H)) for s0 in range(0, H, seg)]
