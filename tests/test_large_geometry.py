"""The large-geometry table (tests/large_geometry.py) on the CPU: every case sits where its name claims — tap counts, live zero-weight
padding, strip plans (ring, tap variant, convert passes, acols), the spans at the LDS gates, routes — the refused set is exactly family F,
refused by the planner and by the oracle alike, and the exact-2x predictor is computed and printed for every exact-2x case of family E.
"""
import numpy as np
import pytest

from tests import large_geometry as G
from tests.golden.cases import SETTING_KEYS, case_frame, case_geometry, oracle_params

E_NOTIMPL = -2147467263


def settings_of(api, c):
    return api.default_settings(**{k: c[k] for k in SETTING_KEYS if k in c})


def tables(api, c):
    (ww, wh), vr = case_geometry(c)
    return api.plan_draw_tables(settings_of(api, c), c["cformat"], c["w"], c["h"], c.get("src_rect"), vr, ww, wh)


def describe(api, c):
    (ww, wh), vr = case_geometry(c)
    w1, h1 = G.source_size(c)
    return api.plan_describe(settings_of(api, c), c["cformat"], w1, h1, vr, ww, wh)


def packs(t):
    """{"x": pack of the draw along screen x, "y": along screen y} of a plan_draw_tables result (a one-draw resize keeps its only pack in t["x"])"""
    if t["y"] is not None:
        return {"x": t["x"], "y": t["y"]}
    return {"xy"[t["first_axis"]]: t["x"]} if t["x"] is not None else {}


def axis_taps(api, c, axis):
    (kind, method) = G.resizers(c)[0 if axis == "x" else 1]
    return api.plan_axis_taps(kind, method, *G.axis_geometry(c, axis), flags=c.get("flags", 0))


def strip_plan(api, c):
    (kx, mx), (ky, my) = G.resizers(c)
    (w1, h1), (w2, h2) = G.source_size(c), c["dst"]
    return api.plan_strip(kx, mx, ky, my, w1, h1, w2, h2, flags=c.get("flags", 0))


@pytest.mark.parametrize("family", sorted(G.FAMILIES))
def test_the_refused_set_is_family_f_and_nothing_else(mpcvr, family):
    """The planner builds tables for every case but family F's, and describes every accepted case as the table says."""
    from videorenderer_amd import api
    for c in G.FAMILIES[family]:
        try:
            t = tables(api, c)
        except api.MpcvrError as e:
            assert c.get("refused") and e.hr == E_NOTIMPL, (c["name"], str(e))
            continue
        assert not c.get("refused"), c["name"]
        assert describe(api, c).startswith(c.get("plan", "passes:")), (c["name"], describe(api, c))
        assert bool(t["strip_planned"]) == bool(c.get("strip")), (c["name"], t["strip_planned"])
        if "period" in c:
            assert (t["P"], t["Q"], t["strip"]["period_taps"]) == c["period"], c["name"]
        elif c.get("strip"):
            assert t["P"] == 0, (c["name"], t["P"], t["Q"])


def test_family_f_is_refused_by_the_planner_and_by_the_oracle(mpcvr, oracle):
    from videorenderer_amd import api
    assert len(G.FAMILIES["refused"]) == 6 and {c["iDownscaling"] for c in G.FAMILIES["refused"]} == set(range(6))
    for c in G.FAMILIES["refused"]:
        failed = []
        for a, axis in enumerate("xy"):
            if G.source_size(c)[a] == c["dst"][a]:
                continue
            try:
                axis_taps(api, c, axis)
            except api.MpcvrError as e:
                assert e.hr == E_NOTIMPL, (c["name"], axis, str(e))
                failed.append(axis)
        assert failed, c["name"]
        frame, pitch = case_frame(c)
        with pytest.raises(RuntimeError, match="orc_process failed: -2"):
            oracle.process(oracle_params(oracle, c), frame, pitch)
        # the video rect the context goes back to is accepted
        assert max(p["ntaps"] for p in packs(tables(api, dict(c, dst=c["back_to"]))).values()) <= G.MAX_TAPS, c["name"]


def test_the_ladder_has_its_tap_counts_and_live_padding(mpcvr):
    from videorenderer_amd import api
    seen = set()
    for c in G.FAMILIES["ladder"]:
        pk = packs(tables(api, c))
        assert {a: p["ntaps"] for a, p in pk.items()} == c["taps"], (c["name"], {a: p["ntaps"] for a, p in pk.items()})
        for axis, n in c["taps"].items():
            idx, w, wsum = axis_taps(api, c, axis)
            assert len(idx[0]) == n, (c["name"], axis, len(idx[0]))
            if n < 16:
                continue
            assert wsum is not None and len(idx) >= G.N_FILTERED
            # a row whose own window is shorter than the table's ntaps: the tail repeats the window's first index with weight zero (interior
            # rows: the indices of a real window rise strictly)
            tex = G.axis_geometry(c, axis)[3]
            padded = [i for i in range(len(idx)) if idx[i][0] > 0 and max(idx[i]) < tex - 1 and idx[i][-1] == idx[i][0] and w[i][-1] == 0.0]
            assert padded, (c["name"], axis, "no interior output row is padded")
            seen.add((c["iDownscaling"], n))
        (kx, mx), (ky, my) = G.resizers(c)
        if c["strip"]:
            sp = strip_plan(api, c)
            assert sp is not None and sp["taps"] == 16 == c["strip_nt"], c["name"]
        elif 17 in c["taps"].values() and len(c["taps"]) == 2:
            assert strip_plan(api, c) is None, c["name"]
    assert seen == {(m, r) for m in range(6) for r in G.RUNGS}, sorted(seen)
    assert {c["cformat"] for c in G.FAMILIES["ladder"]} == {G.P010, G.NV12, G.RGB32}
    for rung in G.RUNGS:
        at = [c for c in G.FAMILIES["ladder"] if rung in c["taps"].values()]
        assert any(c.get("iTexFormat") == 16 for c in at) and any(c.get("output_format") == 1 for c in at), rung


def test_the_strip_edges_have_their_plans(mpcvr):
    from videorenderer_amd import api
    acols = {}
    for c in G.FAMILIES["strip"]:
        sp = strip_plan(api, c)
        t = tables(api, c)
        if not c["strip"]:
            assert sp is None and max(p["ntaps"] for p in packs(t).values()) == 17, c["name"]
            continue
        assert sp is not None and sp["taps"] == c["strip_nt"] == t["strip"]["taps"], (c["name"], sp and sp["taps"])
        assert (t["strip"]["ring"], t["strip"]["acols"], t["strip"]["strip_w"]) == (sp["ring"], sp["acols"], sp["strip_w"]), c["name"]
        acols[c["name"]] = sp["acols"]
        if "ring" in c:
            assert sp["ring"] == c["ring"], (c["name"], sp["ring"])
        if "yspan" in c:
            assert int((sp["yrange"][:, 1] - sp["yrange"][:, 0] + 1).max()) == c["yspan"], c["name"]
        if "tapsxy" in c:
            pk = packs(t)
            assert (pk["x"]["ntaps"], pk["y"]["ntaps"]) == c["tapsxy"], c["name"]
        if "passes" in c:
            assert sp["acols"] == c["acols"] and (sp["acols"] // 2 + 63) // 64 == c["passes"] >= 3, (c["name"], sp["acols"])
    widest = {n: a for n, a in acols.items() if G.CASES[n].get("widest")}
    assert widest and min(widest.values()) == max(acols.values()) == 994
    # ... and no accepted plan is wider: one more source column per output is the 17th tap (Box, the widest window per tap)
    assert api.plan_strip(2, G.BOX, 2, G.BOX, 1280, 40, 80, 16) is None and api.plan_strip(2, G.BOX, 2, G.BOX, 1240, 40, 80, 16)["acols"] == 994
    assert {c["fused"] for c in G.FAMILIES["strip"]} == {"kernel=fused_strip(", "kernel=fused_strip:surface(", None}


def test_the_gate_cases_sit_at_the_gates(mpcvr):
    from videorenderer_amd import api
    gate = {"blk_span": G.K_RESIZE_SPAN_MAX, "blk32_span": G.K_RESIZE_TILE_ROWS_MAX, "blk8_span": G.K_RESIZE_ROW_SPAN_MAX}
    assert gate == {"blk_span": 192, "blk32_span": 72, "blk8_span": 14}
    sides = {k: set() for k in gate}
    pays = set()
    for c in G.FAMILIES["gates"]:
        t = tables(api, c)
        for pack, want in c["spans"].items():
            p = t[pack]
            for field in gate:
                if field in want:
                    assert p[field] == want[field], (c["name"], pack, field, p[field])
                    sides[field].add(p[field] - gate[field])
            if "row_window" in want:
                # RowWindowPays (vp_kernels.hip): the window fits and the 8 rows of a group share their source rows at least 3:1
                assert p["ntaps"] == want["ntaps"]
                assert (p["blk8_span"] <= gate["blk8_span"] and p["blk8_span"] * 3 <= p["ntaps"] * 8) == want["row_window"], c["name"]
                pays.add((p["ntaps"], want["row_window"]))
    assert sides["blk_span"] == {0, 1} and sides["blk32_span"] == {0, 1} and {0, 1} <= sides["blk8_span"], sides
    assert pays == {(4, True), (4, False), (6, True), (6, False)}
    both = [c for c in G.FAMILIES["gates"] if len(c["spans"]) == 2]
    inside = {(c["spans"]["x"]["blk_span"] <= 192, c["spans"]["y"]["blk32_span"] <= 72) for c in both}
    assert inside == {(True, False), (False, True), (True, True)}


def test_the_large_upscales_have_their_routes(mpcvr):
    from videorenderer_amd import api
    seen = set()
    for c in G.FAMILIES["bigup"]:
        (w1, h1), (w2, h2) = G.source_size(c), c["dst"]
        assert {w2 // w1, h2 // h1} <= {1, c["ratio"]} and w2 % w1 == 0 and h2 % h1 == 0, c["name"]
        sp = strip_plan(api, c) if c["iUpscaling"] != G.JINC2 and w1 != w2 and h1 != h2 else None
        assert (sp is not None) == c["strip"], c["name"]
        if sp:
            assert (sp["taps"], sp["ring"]) == (c["strip_nt"], 8), (c["name"], sp["taps"], sp["ring"])
            assert int((sp["yrange"][1:, 0] == sp["yrange"][:-1, 0]).sum()) >= h2 - 2 * h1, c["name"]      # many output rows share a window
        seen.add((c["iUpscaling"], c["ratio"], (w1 != w2) + 2 * (h1 != h2)))
    assert {s[0] for s in seen} == {G.MITCHELL, G.LANCZOS3, G.JINC2} and {s[1] for s in seen} == {16, 64, 127} and {s[2] for s in seen} == {1, 2, 3}


# ---- family E -------------------------------------------------------------------------------------------------------------------------
def predictor(api, method, flags, src_l, src_len, tex_len):
    """max over the outputs of an exact-2x axis of sum_k |w_real - w_nominal| (nominal: t = 0.75 for even outputs, 0.25 for odd)"""
    _, w, _ = api.plan_axis_taps(1, method, src_l, src_len, 2 * src_len, tex_len, flags=flags)
    w = np.array(w, np.float64)
    nominal = [np.array(api.plan_upscale_weights(method, t), np.float64) for t in (0.75, 0.25)]
    d = np.abs(w - np.stack([nominal[i & 1] for i in range(len(w))])).sum(axis=1)
    return float(d.max())


def tex_center(org, length, tex_len, n_out):
    """TexCenter (csrc/vp_params.h) of every output of an axis, restated: fp32 corner coordinates, interpolated in double, rounded once"""
    f = np.float32
    d = f(1.0) / f(tex_len)
    lo, hi = np.float64(d * f(org)), np.float64(d * f(org + length))
    a = (np.arange(n_out, dtype=np.float64) + 0.5) / n_out
    return ((lo + (hi - lo) * a).astype(f) * f(tex_len)).astype(np.float64)


def jinc_weights(pcx, pcy):
    """the 16 normalised weights of ps_resize_onepass_jinc2.hlsl at a pixel whose coordinate is (pcx, pcy)"""
    wa, wb = 0.416 * np.pi, 0.985 * np.pi
    tcx, tcy = np.floor(pcx - 0.5) + 0.5, np.floor(pcy - 0.5) + 0.5
    vx, vy = np.meshgrid(tcx + np.arange(-1, 3) - pcx, tcy + np.arange(-1, 3) - pcy)
    dd = np.sqrt(vx * vx + vy * vy)
    w = np.sin(dd * wa) * np.sin(dd * wb) / (dd * dd)
    return w / w.sum()


def jinc_predictor(length, axis):
    """the same quantity for the Jinc2m draw: the 16 weights at the output whose coordinate is furthest from its nominal position along
    `axis`, against the nominal phases' (the four phases of a 2x draw, either side)"""
    n = 2 * length
    off = float(np.abs(tex_center(0, length, length, n) - (np.arange(n) + 0.5) * 0.5).max())
    worst = 0.0
    for pcy in (0.25, 0.75):
        for pcx in (0.25, 0.75):
            for sg in (-off, off):
                moved = jinc_weights(pcx + sg, pcy) if axis == 0 else jinc_weights(pcx, pcy + sg)
                worst = max(worst, float(np.abs(moved - jinc_weights(pcx, pcy)).sum()))
    return worst


def case_predictor(api, c):
    """the worse axis of an exact-2x case, in codes of its target"""
    quant = 1023 if c.get("output_format", 0) == 1 else 255
    if c["iUpscaling"] == G.JINC2:
        return quant * max(jinc_predictor(G.source_size(c)[a], a) for a in (0, 1))
    return quant * max(predictor(api, c["iUpscaling"], c.get("flags", 0), *(G.axis_geometry(c, a)[i] for i in (0, 1, 3))) for a in "xy")


def test_the_exact_2x_predictor_of_the_wide_frames(mpcvr):
    """sum_k |w_real - w_nominal| x quant for every exact-2x and Jinc2m case of family E: the table holds cases at 0 (powers of two) and above
    one ten-bit code (16380, 15360), so the wide frames exercise the phase drift and do not dodge it."""
    from videorenderer_amd import api
    values = {}
    for c in G.FAMILIES["extent"]:
        if c.get("predict"):
            values[c["name"]] = case_predictor(api, c)
            print(f"PREDICTOR {c['name']}: {values[c['name']]:.3f} codes of {10 if c.get('output_format', 0) == 1 else 8} bits")
    assert len(values) >= 40
    # the planner's threshold (vp_plan.h: kNominalPhaseMaxCodes = 0.5 codes of the target per axis): the cases above it are the table's `aside`
    # cases and no case sits near it; the separable ones are then no longer described as the exact-2x kernel's
    for name, v in values.items():
        c = G.CASES[name]
        assert (v > 0.5) == bool(c.get("aside")) and not 0.4 < v < 0.6, (name, v)
        if c["iUpscaling"] != G.JINC2:
            assert describe(api, c).startswith("passes:" if c.get("aside") else "fused_up2x"), (name, v, describe(api, c))
    assert sum(1 for n in values if G.CASES[n].get("aside")) >= 9
    assert min(values.values()) == 0.0 and max(values.values()) > 1.0, (min(values.values()), max(values.values()))
    ten = {n: v for n, v in values.items() if G.CASES[n].get("output_format", 0) == 1}
    assert any(v == 0.0 for v in ten.values()) and any(v > 1.0 for v in ten.values()), ten
    # the geometries the suite and the benchmark already hold to one code at full size (Lanczos3, one axis, in units of a weight)
    headline = predictor(api, G.LANCZOS3, 0, 0, 3840, 3840)
    twice = predictor(api, G.LANCZOS3, 0, 0, 7680, 7680)
    print(f"PREDICTOR 3840 -> 7680: {headline:.3e} = {255 * headline:.3f} / {1023 * headline:.3f} codes of 8 / 10 bits")
    print(f"PREDICTOR 7680 -> 15360: {twice:.3e} = {255 * twice:.3f} / {1023 * twice:.3f} codes of 8 / 10 bits")
    assert 2.9e-4 < headline < 3.2e-4 and 5.9e-4 < twice < 6.3e-4, (headline, twice)
    worst = predictor(api, G.LANCZOS3, 0, 0, 16380, 16380)
    assert 1.2e-3 < worst < 1.3e-3 and predictor(api, G.LANCZOS3, 0, 0, 16384, 16384) == 0.0, worst


def test_the_extent_table_reaches_every_route_and_extent():
    ext = G.FAMILIES["extent"]
    longs = lambda cs: {max(c["w"], c["h"]) for c in cs}
    for frag in ("up2x_taps4", "up2x_taps5", "up2x_taps6", "jinc2x", "strip_1p5x", "same_size", "down_2p5x"):
        cs = [c for c in ext if c["name"].startswith("extent_" + frag)]
        assert {16384, 16380, 15360} <= longs(cs), frag
        assert {c["w"] > c["h"] for c in cs} == {True, False}, frag
    assert {16380, 15360} <= longs([c for c in ext if "period" in c])
    assert all(max(c["w"], c["h"]) <= G.MAX_EXTENT for c in ext) and any(max(c["w"], c["h"]) == G.MAX_EXTENT for c in ext)
    rects = [c for c in ext if "src_rect" in c]
    for c in rects:
        l, t, r, b = c["src_rect"]
        assert max(l, t) >= 13900 and l % 4 == 0 and t % 2 == 0 and 64 <= max(r - l, b - t) <= 256, c["name"]
    assert {c["cformat"] for c in rects} == {G.P010, G.NV12, G.RGB32}
    assert any(c.get("output_format") == 1 and c.get("hdr_output") for c in ext) and any(c.get("output_format", 0) == 0 and c["cformat"] == G.P010 for c in ext)
    assert set(G.BATCH_CASES) <= set(G.CASES) and len({G.CASES[n].get("fused") for n in G.BATCH_CASES}) >= 5
