"""The tiny-frame table (tests/tiny_frames.py) on the CPU: every case is legal for the oracle and for the product's planner, the planner
agrees with the table on the route, the oracle's own answer is defined to one code on every tail-carrying case (the condition under which
tests/test_tiny_frames_gpu.py holds tails to <= 1 LSB with no witness and no cap), and the table reaches every gate value it is there for.
"""
import numpy as np
import pytest

from tests import tiny_frames as T
from tests.golden.cases import SETTING_KEYS, case_frame, case_geometry, oracle_params
from tests.test_parity_gpu import BG, POW_ULPS, _codes10, has_tail

ALL = sorted(T.CASES)


def settings_of(api, c):
    return api.default_settings(**{k: c[k] for k in SETTING_KEYS if k in c})


def describe(api, c):
    (ww, wh), vr = case_geometry(c)
    w1, h1 = T.source_size(c)
    return api.plan_describe(settings_of(api, c), c["cformat"], w1, h1, vr, ww, wh)


@pytest.mark.parametrize("family", sorted(T.FAMILIES))
def test_every_case_is_legal_for_the_oracle_and_the_planner(mpcvr, oracle, family):
    from videorenderer_amd import api
    for c in T.FAMILIES[family]:
        frame, pitch = case_frame(c)
        p = oracle_params(oracle, c)
        (ww, wh), _ = case_geometry(c)
        out = oracle.process_errdiff(p, frame, pitch) if family == "errdiff" else oracle.process(p, frame, pitch)
        assert out.shape == (wh, ww, 4), c["name"]
        d = describe(api, c)                      # (raises where the planner refuses the geometry)
        assert d.startswith(c["plan"]), (c["name"], d)
        assert ("errdiff" in d) == (family == "errdiff"), (c["name"], d)


@pytest.mark.parametrize("family", ["up2x", "period", "strip", "surface"])
def test_strip_and_periodic_planners_agree_with_the_table(mpcvr, family):
    """api.plan_strip / api.plan_period (the context-free planners) accept the geometries the table sends to k_fused_strip / k_fused_period, and
    the processor's own plan (api.plan_draw_tables: what UpdatePlan builds and uploads) holds a strip plan and the table's (P, Q, taps) —
    or none where the table says the draw is not the fused resize kernels' (one axis only; an X draw through the downscaler at 1:2 rows)."""
    from videorenderer_amd import api
    for c in T.FAMILIES[family]:
        (ww, wh), vr = case_geometry(c)
        (w1, h1), (w2, h2) = T.source_size(c), c["dst"]
        t = api.plan_draw_tables(settings_of(api, c), c["cformat"], c["w"], c["h"], c.get("src_rect"), vr, ww, wh)
        flags = c.get("flags", 0)
        if c.get("one_axis"):
            assert not t["strip_planned"] and t["P"] == 0, c["name"]
            continue
        if "strip" in c or c.get("below_gate"):
            (kx, mx), (ky, my) = T.resizers(c)
            sp = api.plan_strip(kx, mx, ky, my, w1, h1, w2, h2, flags=flags)
            assert sp is not None and t["strip_planned"], c["name"]          # (the tables fit; below the gate it is the convert stage that declines)
            assert (t["strip"]["taps"], t["strip"]["px_per_lane"], t["strip"]["strip_w"]) == (sp["taps"], sp["px_per_lane"], sp["strip_w"]), c["name"]
            assert 1 <= sp["strips"] and sp["xstrip"].min() >= 0 and sp["xstrip"].max() <= w1 - 1, c["name"]
            assert sp["yi"].min() >= 0 and sp["yi"].max() <= h1 - 1 and sp["xi_t"].min() >= 0 and sp["xi_t"].max() <= w1 - 1, c["name"]
        if "period" in c:
            P, Q, nt = c["period"]
            pp = api.plan_period(c["iUpscaling"], w1, h1, w2, h2, flags=flags)
            assert pp is not None and (pp["P"], pp["Q"], pp["taps"]) == (P, Q, nt), c["name"]
            assert (t["P"], t["Q"], t["strip"]["period_taps"]) == (P, Q, nt), c["name"]
            assert pp["xi_t"].min() >= 0 and pp["xi_t"].max() <= w1 - 1, c["name"]
        elif family in ("period", "strip", "surface"):
            assert t["P"] == 0, (c["name"], t["P"], t["Q"])
    if family == "strip":
        # the geometry the periodic planner takes on its own and the processor does not: 8 columns onto 3 go through the downscaler
        assert api.plan_period(T.LANCZOS3, 8, 2, 3, 1) is not None


def test_exact_2x_gate_in_the_planner(mpcvr):
    from videorenderer_amd import api
    s = api.default_settings(iUpscaling=T.LANCZOS3)
    d = lambda w, h: api.plan_describe(s, T.P010, w, h, (0, 0, 2 * w, 2 * h), 2 * w, 2 * h)
    assert d(8, 8).startswith("fused_up2x") and d(10, 8).startswith("fused_up2x") and d(8, 10).startswith("fused_up2x")
    for w, h in ((8, 6), (6, 8), (8, 2)):
        assert d(w, h).startswith("passes:"), (w, h)
    j = api.default_settings(iUpscaling=T.JINC2)
    assert api.plan_describe(j, T.P010, 8, 8, (0, 0, 16, 16), 16, 16).startswith("fused_jinc2x")
    assert api.plan_describe(j, T.P010, 6, 6, (0, 0, 12, 12), 12, 12).startswith("passes:")


TAILS = [n for n in ALL if has_tail(T.CASES[n]) and T.CASES[n]["family"] != "errdiff"]


def test_the_oracles_own_answer_is_defined_to_one_code_behind_every_tail(oracle):
    """The ten oracle runs of compare_behind_tail (every pow() POW_ULPS ulps low, high, and eight hash-drawn mixes) span at most ONE code of the
    render target on every channel of every tail-carrying case: no channel of the table is ill-conditioned, so the GPU tests need no witness."""
    assert len(TAILS) >= 60
    worst = {}
    for name in TAILS:
        c = T.CASES[name]
        frame, pitch = case_frame(c)
        p = oracle_params(oracle, c)
        codes = _codes10 if c.get("output_format", 0) == 1 else (lambda a: a[..., :3].astype(np.int16))
        bg = np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8)
        want = codes(oracle.process(p, frame, pitch, dst=bg.copy()))
        lo, hi = want.copy(), want.copy()
        for bias, seed in [(-POW_ULPS, 0), (POW_ULPS, 0)] + [(POW_ULPS, k) for k in range(1, 9)]:
            run = codes(oracle.process_with_pow_bias(p, frame, pitch, bias, dst=bg.copy(), seed=seed))
            lo = np.minimum(lo, run); hi = np.maximum(hi, run)
        span = int((hi - lo).max())
        if span > 1:
            worst[name] = span
    assert not worst, f"cases whose oracle answer spans more than one code under +-{POW_ULPS} ulp of pow() (change their seed): {worst}"


def test_the_table_reaches_every_gate_value():
    """What a later edit must not quietly drop: the edge sizes themselves."""
    fam = T.FAMILIES
    gate = lambda cases: [c for c in cases if not c.get("below_gate")]
    below = lambda cases: [c for c in cases if c.get("below_gate")]
    src = lambda cases: {T.source_size(c) for c in cases}
    # exact 2x and Jinc2m 2x: 8 x 8, one step up on either axis, one step down on either axis
    assert {(8, 8), (10, 8), (8, 10), (14, 12)} <= src(gate(fam["up2x"])) and {(8, 6), (6, 8), (8, 2)} <= src(below(fam["up2x"]))
    assert {(8, 8), (10, 8), (8, 10)} <= src(gate(fam["jinc2x"])) and {(6, 6)} <= src(below(fam["jinc2x"]))
    up = gate(fam["up2x"])
    assert {c["iUpscaling"] for c in up} >= {T.MITCHELL, T.LANCZOS3, T.SPLINE36} and any(c.get("flags", 0) & T.FLAG_LANCZOS3_FIXED for c in up)
    assert {(c["cformat"], c["exfmt"]) for c in up} >= {(cf, ex) for _, cf, ex in T.FORMATS_AND_TAILS}
    offs = {c["offset"][0] % 4 for c in up if "offset" in c}
    assert 0 in offs and offs - {0}, offs
    assert any(c.get("output_format") == 1 for c in up)
    # same size: widths 8, 12 (the streaming kernel) and 10, 14 (the block kernel), heights 2 and up; below: 6 x 2 and 4 x 4
    assert {(8, 2), (8, 4), (12, 2), (10, 2), (14, 6)} <= src(gate(fam["same"])) and {(6, 2), (4, 4)} <= src(below(fam["same"]))
    assert {c["cformat"] for c in fam["same"]} >= {T.P010, T.NV12, T.YUV420P10, T.YUY2, T.Y8, T.AYUV}
    assert sum(1 for c in fam["same"] if c.get("iChromaScaling") == 2) >= 2 and {c["dovi"]["kind"] for c in fam["same"] if "dovi" in c} == {"poly", "mmr"}
    # periodic ratios: every built (P, Q), output heights 1 and 3, an odd output width, widths 8 and heights 2
    per = fam["period"]
    assert {c["period"][:2] for c in per} == {(4, 3), (3, 2), (2, 3), (1, 2), (3, 1)}
    assert {c["period"][2] for c in per} == {4, 5}
    assert {1, 3} <= {c["dst"][1] for c in per} and any(c["dst"][0] & 1 for c in per)
    assert {8} <= {c["w"] for c in per} and {2} <= {c["h"] for c in per}
    for c in per:                                   # an odd width sits in an even window: the kernel's 8-byte rows
        assert case_geometry(c)[0][0] % 2 == 0, c["name"]
    # any ratio: a 2-row source, an output of one row, odd output widths, downscaler taps; surface mode from 1 x 1
    st = gate(fam["strip"])
    assert {(8, 2), (10, 4), (14, 6), (16, 2)} <= src(st) and {1, 5} <= {c["dst"][1] for c in st}
    assert {c.get("iDownscaling") for c in st} >= {2, 3} and {c["cformat"] for c in st} >= {cf for _, cf, _ in T.FORMATS_AND_TAILS}
    assert {(1, 1), (3, 3), (5, 3)} <= src(fam["surface"]) and {T.RGB32, T.R210} <= {c["cformat"] for c in fam["surface"]}
    assert any("src_rect" in c and (c["src_rect"][0] % 4 or c["src_rect"][1] % 2) for c in fam["surface"])
    # plain kernels: every source size, all six upscalers and downscalers, every rotation
    pl = fam["plain"]
    assert {(1, 1), (1, 5), (5, 1), (2, 2), (3, 2)} <= src(pl)
    assert {c["iUpscaling"] for c in pl} >= set(range(6)) and {c["iDownscaling"] for c in pl if "iDownscaling" in c} >= set(range(6))
    used = {km for c in pl if not c.get("rotation") for km in T.resizers(c)}          # (kind, method) of the draws that really run
    assert used >= {(1, m) for m in range(1, 6)} | {(2, m) for m in range(6)} and any(c["iUpscaling"] == 0 for c in pl), sorted(used)
    assert {c.get("rotation", 0) for c in pl} == {0, 90, 180, 270}
    assert {(1, 1), (7, 3)} <= {c["dst"] for c in pl}
    # error diffusion: the rects on either side of a band hand-off, one column, one row
    from tests.test_errdiff import region
    rects = set()
    for c in fam["errdiff"]:
        (x0, y0, x1, y1), _ = region(c)
        assert (x1 - x0, y1 - y0) == c["rect"], c["name"]
        rects.add(c["rect"])
    assert {(1, 1), (1, 50), (70, 1), (2, 22), (3, 21), (8, 43), (9, 2), (16, 16)} <= rects
    # every case meant for a kernel that loads raw samples as dwords has rows those loads can take
    for c in T.CASES.values():
        if not c.get("below_gate") and any(f in ("fused_up2x", "fused_jinc2x", "kernel=fused_strip(") or f.startswith("kernel=fused_period(") for f in c.get("route", ())):
            assert T.rows_dword_aligned(c["cformat"], c["w"]), c["name"]
    # one gate-size case per fused family for the neighbour and batch tests
    assert {T.CASES[n]["family"] for n in T.GATE_CASES} == {"up2x", "jinc2x", "same", "period", "strip", "surface"}
    assert all(not T.CASES[n].get("below_gate") for n in T.GATE_CASES)
