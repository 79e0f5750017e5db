"""The arguments of the tone curves: the table and the frame of tests/test_tone_params.py (CPU) and tests/test_tone_params_gpu.py (GPU).
Importable without a GPU and without a built library.

Three ranges are walked here, each of which the rest of the suite touches at one or two values:
  * SDR_NITS       iSDRDisplayNits 25 .. 400 (LuminanceScale = 10000 / nits: the PQ -> SDR and HLG -> SDR tails of every convert route, the
                   4096-entry table of BuildPqSdrLut, and kinds 3 .. 5 of mpcvr_correction_pass);
  * HDR10_ROWS     (min mastering, max mastering, MaxCLL, MaxFALL, display peak) in front of the six operators of the HDR10 tone-mapping step
                   (hdr10_tonemap, vp_device.h; orc_hdr10_tonemap, the oracle), each row labelled with the branches it is meant to enter;
  * DOVI_ROWS      the two ways a Dolby Vision RPU reaches that step: level 1 replaces the metadata (and operator 5 becomes 6), a selected
                   level-2 block runs the trims inside the step.

THE FRAME (frame()): one P010 source, 256 x 32, built here code by code so that the operator's input is known:
  rows  0 ..  7   luma code (y * 256 + x) // 2 under neutral chroma: every 10-bit code 0 .. 1023 twice.  Codes below 64 and above 940 reach
                  the saturates of the convert; codes <= 64 are the exactly-black pixels of operator 5's `avg <= 1e-6` and operator 6's
                  `x_nits > 0`;
  rows  8 .. 15   a luma ramp over the legal range (64 .. 940) under the eight saturated chroma corners (U, V in {64, 512, 960}, without the
                  neutral pair): the bright saturated BT.2020 colours whose 2020 -> 709 row cancels;
  rows 16 .. 31   seeded noise over all 1024 codes in luma and chroma.

branches(texture, k, op) restates the branch PREDICATES of the step in numpy (float64) over the 10-bit texture the operator reads and the
sanitised constants: the population of every branch, nothing about what a pixel becomes.

Two branches of the step are not entered by any row, and no input is invented for them (tests/test_tone_params.py):
  * BT.2390's `KS = max(0, 1.5 PQ(display) - 0.5 PQ(content))`.  The sanitised display peak is at least 100 nits and 1.5 PQ(100) = 0.762;
    0.5 PQ(content) stays below that for every content peak up to 65535 nits, the most a 16-bit MaxCLL / mastering field of HDR10 metadata
    carries (KS = +0.168 there).  This is an ASSUMPTION ABOUT CALLERS: mpcvr_set_hdr_metadata takes floats and SanitiseHdr10Params, like the
    reference, has no upper clamp, so a caller who passes a content peak of some 3 million nits or more does reach the clamp (KS = -0.024 at 1e7);
  * ST 2094-10's `maxFALL > 0 ? PQ(maxFALL) : lerp(src_min, src_max, 0.4)`: a MaxFALL of 1 or less is replaced by MaxCLL, which is above 10 —
    unreachable whatever the caller passes (shown through mpcvr_plan_hdr10_params).
"""
import numpy as np

from tests.golden.cases import HDR10, HLG, MPEG2, TV, ext

P010 = 2
W, H = 256, 32
PITCH = 2 * W
TVONLY = ext(MPEG2, TV)           # the tag of the suite's Dolby Vision cases: the RPU carries the colourimetry

SDR_NITS = (25, 26, 60, 100, 125, 203, 300, 399, 400)
SDR_TAILS = {"pq": HDR10, "hlg": HLG}

OPERATORS = (1, 2, 3, 4, 5, 6)
GEOMETRIES = {"same": (256, 32), "1p5x": (384, 48), "1p25x": (320, 40), "2x": (512, 64)}

CORNERS = tuple((u, v) for u in (64, 512, 960) for v in (64, 512, 960) if (u, v) != (512, 512))


def frame():
    """(uint8 buffer in the P010 sample layout, pitch): see the module docstring."""
    y = np.zeros((H, W), np.uint16)
    u = np.full((H // 2, W // 2), 512, np.uint16)
    v = np.full((H // 2, W // 2), 512, np.uint16)
    yy, xx = np.mgrid[0:8, 0:W]
    y[0:8] = (yy * W + xx) // 2
    ramp = (64 + (np.arange(W // 2) * (940 - 64) + (W // 2 - 1) // 2) // (W // 2 - 1)).astype(np.uint16)          # 64 .. 940 over 128 columns
    for i, (cu, cv) in enumerate(CORNERS):
        r, half = 8 + 2 * (i // 2), i % 2
        y[r:r + 2, half * 128:half * 128 + 128] = ramp
        u[r // 2, half * 64:half * 64 + 64] = cu
        v[r // 2, half * 64:half * 64 + 64] = cv
    rng = np.random.default_rng(20251)
    y[16:32] = rng.integers(0, 1024, size=(16, W), dtype=np.uint16)
    u[8:16] = rng.integers(0, 1024, size=(8, W // 2), dtype=np.uint16)
    v[8:16] = rng.integers(0, 1024, size=(8, W // 2), dtype=np.uint16)
    uv = np.stack([u, v], -1).reshape(H // 2, W)
    buf = np.concatenate([(y << 6).astype("<u2").reshape(-1), (uv << 6).astype("<u2").reshape(-1)]).view(np.uint8).copy()
    buf.setflags(write=False)
    return buf, PITCH


# ---- the HDR10 rows -----------------------------------------------------------------------------------------------------------------
# meta = (min mastering, max mastering, MaxCLL, MaxFALL) as a caller passes them to mpcvr_set_hdr_metadata, display = the display peak of
# mpcvr_set_hdr_output.  The labels (what test_tone_params.py holds branches() to, on the frame above):
#   op5      the branches of BT.2390 the row populates: "inactive" (display >= content: the early return, every pixel) or a subset of
#            "black", "below", "above" (the knee)
#   op6      "inactive" or "mapped" (ST 2094-10; black pixels come with every mapped row), src / dst: which way the source and destination
#            knees clamp ("low", "free", "high")
#   eff      operators 1 .. 4: which of base = max(display, max mastering) and MaxCLL is the smaller; fall = min(base / MaxFALL, 1);
#            clipped: "none", "some" or "most" (more than half) of the channels exceed eff and meet the saturate
def _row(name, meta, display, what, op5, op6, src=None, dst=None, eff="cll", fall=1.0, clipped="some"):
    return dict(name=name, meta=tuple(float(x) for x in meta), display=float(display), what=what, op5=tuple(op5), op6=op6, src=src, dst=dst, eff=eff, fall=fall,
                clipped=clipped)


_ACTIVE = ("black", "below", "above")
HDR10_ROWS = (
    _row("typical_400", (0.005, 1000, 1000, 400), 400, "operators 5 and 6 active, source knee clamped high", _ACTIVE, "mapped", src="high", dst="free"),
    _row("no_cll_4000", (0.005, 4000, 0, 0), 400, "MaxCLL falls back to mastering, MaxFALL to that", _ACTIVE, "mapped", src="high", dst="free"),
    _row("display_brighter", (0.005, 1000, 800, 200), 1000, "display >= content: the early return of operators 5 and 6", ("inactive",), "inactive"),
    _row("all_fallbacks_100", (0, 0, 0, 0), 100, "every fallback, the lowest display", _ACTIVE, "mapped", src="high", dst="free"),
    _row("knee_free_600", (0.05, 4000, 4000, 2), 600, "source knee free (mid)", _ACTIVE, "mapped", src="free", dst="free"),
    _row("fall_equals_cll_203", (0.005, 1000, 1000, 1000), 203, "MaxFALL = MaxCLL: the source knee at the top of its range", _ACTIVE, "mapped", src="high", dst="free"),
    _row("fall_above_base_300", (0.005, 1000, 1000, 5000), 300, "MaxFALL above base: fall = 0.2", _ACTIVE, "mapped", src="high", dst="free", fall=0.2),
    _row("base_below_cll_100", (0.005, 400, 4000, 300), 100, "eff = base < MaxCLL: more channels clipped than on any other row", _ACTIVE, "mapped", src="free",
         dst="free", eff="base", clipped="most"),
    _row("nothing_clipped_10000", (1.0, 10000, 10000, 4000), 10000, "nothing clipped, nothing mapped", ("inactive",), "inactive", clipped="none"),
    _row("display_out_of_range_50", (0.005, 1000, 1000, 400), 50, "display peak out of range: drawn as 1000", ("inactive",), "inactive"),
    # the rows that clamp the ST 2094-10 source knee LOW: PQ(MaxFALL) below src_min + 0.1 (src_max - src_min) needs a bright mastering black
    # and a small MaxFALL (a MaxFALL of 1 or less is replaced by MaxCLL)
    _row("src_knee_low_400", (1.0, 4000, 4000, 1.5), 400, "source knee clamped low, destination knee free", _ACTIVE, "mapped", src="low", dst="free"),
    # ... and the destination knee HIGH: a MaxCLL far above what PQ codes (the widest source range over the dimmest display).  Where the SOURCE
    # knee clamps, the destination knee equals its own bound analytically (target = 0.1 or 0.8, adaptation = 1): that clamp moves nothing
    # beyond an ulp, and branches() reports it as "free" (see _clamp_way's margin).  No legal metadata clamps the destination knee LOW other
    # than through such a tie (a grid over min 0 .. 50, MaxCLL 11 .. 65535, MaxFALL 1.01 .. 65535, display 100 .. 10000 finds none)
    _row("dst_knee_high_100", (0.005, 10000, 65535, 400), 100, "destination knee clamped high, MaxCLL beyond the PQ range", _ACTIVE, "mapped", src="free",
         dst="high", eff="base", clipped="none"),
)
ROWS_BY_NAME = {r["name"]: r for r in HDR10_ROWS}

# Dolby Vision rows (synth.dovi_metadata as the golden cases use it).  meta is what mpcvr_set_hdr_metadata is given; with level 1 present the
# step takes min / max / MaxCLL / MaxFALL from L1 instead (62 / 4095 PQ, 1400 nits, 60 nits) and operator 5 becomes 6.
DOVI_ROWS = (
    dict(name="dovi_l1", dovi=dict(kind="poly", l1=True), meta=(0.005, 1000.0, 1000.0, 400.0), display=400.0, l1=True, l2=False,
         what="level 1 present: operator 5 becomes 6, the metadata comes from L1"),
    dict(name="dovi_l2", dovi=dict(kind="poly", l2=(100, 600, 1000)), meta=(0.005, 1000.0, 1000.0, 400.0), display=600.0, l1=False, l2=True,
         what="level 2 selected for the display peak: the trims run inside the step"),
)


def hdr_case(row, op, geo="same", **over):
    """the case dict (tests/golden/cases.py style; the frame is frame(), not a synth kind) of a row through operator `op` (0: the step absent)"""
    c = dict(name=f"{row['name']}_op{op}_{geo}", cformat=P010, w=W, h=H, dst=GEOMETRIES[geo], exfmt=HDR10, iUpscaling=4, output_format=1, hdr_output=1,
             hdr_tonemap=op, hdr_display=row["display"], hdr_meta=row["meta"])
    if "dovi" in row:
        c.update(exfmt=TVONLY, dovi=row["dovi"])
    c.update(over)
    return c


def sdr_case(tail, nits, geo="same", **over):
    c = dict(name=f"{tail}_{nits}nits_{geo}", cformat=P010, w=W, h=H, dst=GEOMETRIES[geo], exfmt=SDR_TAILS[tail], iUpscaling=4, iSDRDisplayNits=nits)
    c.update(over)
    return c


# ---- the branch predicates ----------------------------------------------------------------------------------------------------------
_M1, _M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
_C1, _C2, _C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0


def pq_to_nits(e):
    p = np.power(np.clip(np.asarray(e, np.float64), 0.0, 1.0), 1.0 / _M2)
    return 10000.0 * np.power(np.maximum(p - _C1, 0.0) / (_C2 - _C3 * p), 1.0 / _M1)


def nits_to_pq(n):
    y = np.power(np.maximum(np.asarray(n, np.float64), 0.0) / 10000.0, _M1)
    return np.power((_C1 + _C2 * y) / (1.0 + _C3 * y), _M2)


def constants(words):
    """the six words of mpcvr_plan_hdr10_params -> dict(min, max, cll, fall, display, selection)"""
    f = np.array(list(words)[:5], np.uint32).view(np.float32).astype(np.float64)
    return dict(min=float(f[0]), max=float(f[1]), cll=float(f[2]), fall=float(f[3]), display=float(f[4]), selection=int(list(words)[5]))


def _lerp(a, b, t):
    return a + t * (b - a)


def _smoothstep(e0, e1, x):
    t = min(max((x - e0) / (e1 - e0), 0.0), 1.0)
    return t * t * (3.0 - 2.0 * t)


def _clamp_way(x, lo, hi, margin=1e-6):
    """which way min(max(x, lo), hi) clamps; within `margin` of a bound (PQ units: a thousandth of a 10-bit code) counts as free"""
    return "low" if x < lo - margin else "high" if x > hi + margin else "free"


def branches(texture_codes, k, op):
    """Populations of the branches operator `op` enters on a texture of 10-bit codes ((h, w, 3), R G B) with the sanitised constants k
    (constants()).  Pixels for operators 5 and 6, channels for 1 .. 4."""
    nits = pq_to_nits(np.asarray(texture_codes, np.float64) / 1023.0)
    luma = 0.2627 * nits[..., 0] + 0.6780 * nits[..., 1] + 0.0593 * nits[..., 2]
    n = int(luma.size)
    if op == 5:
        safe = k["cll"]
        if safe <= 10.0:
            safe = k["max"]
        if safe <= 10.0:
            safe = 1000.0
        ks = 1.5 * nits_to_pq(k["display"]) - 0.5 * nits_to_pq(safe)
        out = dict(inactive=0, black=0, below=0, above=0, ks_clamped=bool(ks < 0.0))
        if k["display"] >= safe:
            out["inactive"] = n
            return out
        black = luma <= 1e-6
        e1 = nits_to_pq(luma)
        above = ~black & (e1 > max(ks, 0.0))
        out.update(black=int(black.sum()), above=int(above.sum()), below=int((~black & ~above).sum()))
        return out
    if op == 6:
        out = dict(inactive=0, zero=0, mapped=0, src=None, dst=None, fall_alternative=bool(not k["fall"] > 0.0))
        if k["display"] >= k["cll"]:
            out["inactive"] = n
            return out
        src_min, src_max, src_avg = nits_to_pq(k["min"]), nits_to_pq(k["cll"]), nits_to_pq(k["fall"])
        dst_min, dst_max = nits_to_pq(0.0), nits_to_pq(k["display"])
        lo, hi = _lerp(src_min, src_max, 0.1), _lerp(src_min, src_max, 0.8)
        out["src"] = _clamp_way(src_avg, lo, hi)
        src_knee = min(max(src_avg, lo), hi)
        target = (src_knee - src_min) / (src_max - src_min)
        adapted = _lerp(dst_min, dst_max, target)
        tuning = 1.0 - _smoothstep(0.8, 0.4, target) * _smoothstep(0.1, 0.4, target)
        dst_knee = _lerp(src_knee, adapted, _lerp(0.4, 1.0, tuning))
        out["dst"] = _clamp_way(dst_knee, _lerp(dst_min, dst_max, 0.1), _lerp(dst_min, dst_max, 0.8))
        out.update(zero=int((luma <= 0.0).sum()), mapped=int((luma > 0.0).sum()))
        return out
    base = max(k["display"], k["max"])
    eff = min(base, k["cll"])
    clipped = int((nits > eff).sum())
    return dict(eff="base" if base < k["cll"] else "cll", fall=min(base / k["fall"], 1.0), clipped=clipped, unclipped=int(nits.size) - clipped)


def texture_codes(rgb10):
    """(h, w, 3) R G B codes of an R10G10B10A2 frame given as (h, w, 4) uint8 or (h, w) uint32"""
    a = np.ascontiguousarray(rgb10)
    u = a.view(np.uint32)[..., 0] if a.dtype == np.uint8 else a
    return np.stack([(u >> sh) & 1023 for sh in (0, 10, 20)], -1).astype(np.int32)


# ---- the cases the oracle is pinned to the reference's shader text on (tests/golden/tone_params_pins.json) -------------------------------
PIN_GEOMETRIES_HDR = ("same", "1p5x")         # the step reads the convert output / the post-scale surface
PIN_GEOMETRIES_SDR = ("same", "2x")


def pin_cases():
    """key -> case: every HDR10 and Dolby Vision row x six operators x two geometries, every SDR_NITS value x {PQ, HLG} x two geometries"""
    out = {}
    for row in HDR10_ROWS + DOVI_ROWS:
        for op in OPERATORS:
            for geo in PIN_GEOMETRIES_HDR:
                out[f"hdr10/{row['name']}/op{op}/{geo}"] = hdr_case(row, op, geo)
    for tail in SDR_TAILS:
        for nits in SDR_NITS:
            for geo in PIN_GEOMETRIES_SDR:
                out[f"sdr/{tail}/{nits}nits/{geo}"] = sdr_case(tail, nits, geo)
    return out


def describe(c):
    """what a pin file may say about a case: its settings, no pixel"""
    keep = ("cformat", "w", "h", "dst", "exfmt", "iUpscaling", "iSDRDisplayNits", "output_format", "hdr_output", "hdr_tonemap", "hdr_display", "hdr_meta", "dovi")
    return {k: (list(c[k]) if isinstance(c[k], tuple) else c[k]) for k in keep if k in c}
