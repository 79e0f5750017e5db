"""The table of tests/up2x_bp_cases.py on the CPU: every row reports the form a restatement of the twin's gate gives it, and the table reaches
what it is there for — every lane 2 .. 63 owning a rect's last block, both outcomes of `edge_wave` in front of a 2-column and a 4-column last
strip, a strip in a second workgroup, last segments of 2, 4 and 6 rows, frames of one, two and three segments.  The coverage assertions are
set equalities: a sweep thinned later fails here.
"""
import pytest

from tests import up2x_bp_cases as T
from tests.golden.cases import COSITED, MPEG1, SETTING_KEYS, case_geometry
from tests.test_parity_gpu import has_tail, internal_is_8bit
from tests.test_up2x_bp_loop import SITINGS           # (vk1, vk2, vk3) per siting as FillFusedArgs emits them
from videorenderer_amd import synth


def settings_of(api, c):
    return api.default_settings(**{k: c[k] for k in SETTING_KEYS if k in c})


def plan_name(api, c):
    (ww, wh), vr = case_geometry(c)
    _, _, W, H = T.rect_of(c)
    return api.plan_describe(settings_of(api, c), c["cformat"], W, H, vr, ww, wh)


def fast_convert(c):
    """CHipVideoProcessor::FillFusedParams: dword loads need a rect that starts on a 4 x 2 grid and rows that start on multiples of 4 bytes
    (the chroma plane of a bi-planar sample has the luma pitch and starts pitch * h bytes in)"""
    l, t, _, _ = T.rect_of(c)
    pitch = c.get("pitch") or synth.default_pitch(c["cformat"], c["w"])
    return l % 4 == 0 and t % 2 == 0 and pitch % 4 == 0 and (pitch * c["h"]) % 4 == 0


def aligned_epilogue(c):
    """LaunchFusedUp2xNT: the specialised epilogues take a target on a 16-byte boundary, rows 16 bytes apart and off_x % 4 == 0"""
    (ww, _), vr = case_geometry(c)
    off = c.get("target_off", 0)
    pitch = ww * 4 + (4 if off else 0)              # (a target at +4 is drawn with a pitch of window_w * 4 + 4: the `off4` layout)
    return off % 16 == 0 and pitch % 16 == 0 and vr[0] % 4 == 0


def gate(api, c):
    """The form FusedUp2xBpTakes must give the row: None where no exact-2x kernel is planned, else "bp" / "generic"."""
    l, t, W, H = T.rect_of(c)
    if not plan_name(api, c).startswith("fused_up2x"):
        return None                                   # DecidePlan: rect inside the window, a layout of the fused kernels, >= 8 x 8
    if not fast_convert(c) or W < 8 or H < 8 or W % 2 or H % 2:
        return None                                   # FusedUp2xSupported (UpdatePlan)
    # an instantiation that exists, in the fast form of the convert stage
    tail = has_tail(c)
    if c["cformat"] in (T.P010, T.P016):
        planned = aligned_epilogue(c) and not (internal_is_8bit(c) and not tail)
    else:
        planned = c["cformat"] == T.NV12 and not tail and aligned_epilogue(c) and not internal_is_8bit(c) and c.get("output_format", 0) == 1
    if not planned:
        return "generic"
    # the chroma filter: bilinear, not centred; the siting's row rule
    chroma = (c.get("exfmt", 0) >> 8) & 0xf
    nearest = c.get("iChromaScaling", 1) == 0
    if nearest or chroma == MPEG1:
        return "generic"
    vk = SITINGS["4:2:0 co-sited" if chroma == COSITED else "4:2:0 MPEG-2"]
    # the matrix' structural zeros
    m, _ = api.plan_color_matrix(c["cformat"], W, H, c.get("exfmt", 0), *c.get("procamp", (0.0, 1.0, 0.0, 1.0)))
    if m[1] != 0.0 or m[8] != 0.0:
        return "generic"
    # the lane identity: even W and rect_l, the rect reaching the frame's chroma end; the row identity: rect_t even, the carry granted
    cw, ch = (c["w"] + 1) // 2, (c["h"] + 1) // 2
    if W % 2 or l % 2 or W < 2 or ((l + W - 2) >> 1) < cw - 1 or t % 2:
        return "generic"
    return "bp" if api.plan_up2x_row_carry(*vk, t, H, ch) else "generic"


@pytest.mark.parametrize("group", T.GROUPS)
def test_every_row_reports_the_form_the_gate_gives_it(mpcvr, group):
    from videorenderer_amd import api
    for c in T.rows_of(group):
        assert gate(api, c) == c["form"], (c["name"], gate(api, c), c["form"], c["why"])
        assert c["why"] and c["kind"] == "noise"
        if c["form"] is not None:
            assert "fused_up2x" in c["route"], c["name"]
        else:
            assert "fused_up2x" in c["no_route"], c["name"]


def test_the_gate_restated_here_refuses_what_the_existing_refusals_draw(mpcvr):
    """the restatement is not a rubber stamp: the refusals tests/test_up2x_bp_gpu.py draws come out `generic` (or None) of it as well"""
    from videorenderer_amd import api
    from tests.test_up2x_bp_gpu import NOT_TWIN
    for name, c in NOT_TWIN.items():
        c = dict(c, kind="noise", seed=1, iUpscaling=4)
        if c["cformat"] in (T.NV12, T.P010):             # (the restatement covers the bi-planar 4:2:0 formats the table draws)
            # (an odd rect top switches fast_convert off: no exact-2x kernel at all)
            assert gate(api, c) == (None if name == "odd_rect_top" else "generic"), (name, gate(api, c))
    base = dict(T.PLANS["p010_pq_dither8"], w=128, h=40, dst=(256, 80), kind="noise", seed=1, iUpscaling=4)
    assert gate(api, base) == "bp"
    assert gate(api, dict(base, src_rect=(2, 0, 128, 40), dst=(252, 80))) is None
    assert gate(api, dict(base, procamp=(0.0, 1.0, 1.0, 1.0))) == "generic"
    assert gate(api, dict(base, w=1920, h=1080, dst=(3840, 2160))) == "bp" and gate(api, dict(base, w=3840, h=2160, dst=(7680, 4320))) == "bp"


def sweep_widths():
    rows = T.rows_of("widths_p010_pq_dither8")
    assert [c["w"] for c in rows] == list(T.WIDTHS) and all(c["h"] == 24 and c["form"] == "bp" for c in rows)
    return [c["w"] for c in rows]


def test_the_last_block_is_owned_by_every_lane_from_2_to_63():
    lanes = set()
    for W in sweep_widths():
        own = T.last_block_lanes(W)
        assert own, W                                    # some lane holds the last block unclamped
        for k, lane in own.items():
            x0 = k * T.S
            assert x0 - 4 + 2 * lane == W - 2
            lanes.add(lane)
    assert lanes == set(range(2, 64)), sorted(set(range(2, 64)) ^ lanes)
    # lanes 62 and 63 are the strip in front of a last strip of 2 and of 4 columns — the widths where lane 63's missing neighbour matters
    for W, lane in ((122, 62), (124, 63), (242, 62), (244, 63), (482, 62), (484, 63)):
        assert T.last_block_lanes(W)[len(T.strips(W)) - 2] == lane, W
    # ... and every other plan of the sweep draws both of them, in a first strip and behind one
    for plan in ("nv12_fast_direct10", "p010_hlg_dither8", "p010_pq_direct10"):
        ws = [c["w"] for c in T.rows_of(f"widths_{plan}")]
        assert ws == list(T.WIDTHS_OTHER_PLANS)
        assert {(k, lane) for W in ws for k, lane in T.last_block_lanes(W).items() if lane >= 62} == {(0, 62), (0, 63), (1, 62), (1, 63), (3, 62), (3, 63)}


def test_both_edge_wave_outcomes_in_front_of_short_last_strips():
    seen = set()
    for W in sweep_widths():
        st = T.strips(W)
        last_cols = W - st[-1][2]
        if len(st) >= 2 and last_cols in (2, 4):
            _, _, x0, edge = st[-2]
            assert edge == (x0 == 0 or x0 + 122 > W - 2)
            seen.add((last_cols, x0 == 0, edge))
    # (columns of the last strip, the strip in front of it is the frame's first, its edge_wave)
    assert seen == {(2, True, True), (2, False, True), (4, True, True), (4, False, False)}, seen


def test_a_strip_in_a_second_workgroup():
    blocks = {b for W in sweep_widths() for _, b, _, _ in T.strips(W)}
    assert blocks == {0, 1}, blocks
    fifth = sorted(W for W in sweep_widths() if len(T.strips(W)) == 5)
    assert fifth == [482, 484, 486], fifth
    for W in fifth:
        k, b, x0, edge = T.strips(W)[4]
        assert (k, b, x0, edge) == (4, 1, 480, True)
    assert {len(T.strips(W)) for W in sweep_widths()} == {1, 2, 3, 4, 5}
    assert [len(T.strips(W)) for W in T.HEADLINE_WIDTHS] == [16, 32]


def test_segments_of_the_height_rows():
    for w in T.HEIGHT_WIDTHS:
        rows = [c for c in T.rows_of(f"heights_{w}") if c["form"] == "bp"]
        assert [c["h"] for c in rows] == list(T.HEIGHTS)
        last, counts, seams = set(), set(), set()
        for c in rows:
            segs = T.segments(c["w"], c["h"])
            assert T.segment_rows(c["w"], c["h"]) == min(24, c["h"]), c["name"]
            assert all(s0 % 2 == 0 for s0, _ in segs) and segs[-1][1] == c["h"]
            counts.add(len(segs))
            last.add(segs[-1][1] - segs[-1][0])
            seams.update(s0 for s0, _ in segs[1:])
            assert str(segs[-1][1] - segs[-1][0]) + " rows" in c["why"] and f"{len(segs)} segment" in c["why"]
        assert counts == {1, 2, 3}
        assert last == set(range(2, 26, 2)), sorted(last)               # 2, 4 and 6 rows — shorter than the four-times-unrolled loop — and every longer one
        assert seams == set(T.SEAM_ROWS)
        assert [c["h"] for c in T.rows_of(f"heights_{w}") if c["form"] is None] == [6]
    # the width rows: one segment of 24 rows = 15 iterations
    assert all(T.segments(W, 24) == [(0, 24)] for W in T.WIDTHS) and (24 + 1) // 2 + 3 == 15
    assert all(T.segments(W, 8) == [(0, 8)] for W in T.HEADLINE_WIDTHS)


def test_segments_and_tables_of_the_batch_rows():
    by = {c["name"]: c for c in T.rows_of("batches")}
    assert sorted(c["batch"] for c in by.values()) == [3, 33, 34]
    for n in (33, 34):
        c = by[f"batches_{n}_frames_64x8"]
        assert c["batch"] > 32 and T.segments(c["w"], c["h"], n) == [(0, 8)]           # FrameTable32: 32 rows by value
    c = by["batches_3_frames_124x200"]
    segs = T.segments(c["w"], c["h"], 3)
    assert [s0 for s0, _ in segs] == list(range(0, 200, 24)) and segs[-1] == (192, 200)
    # on any device of 64 compute units or more the batch is one round of the resident waves for every candidate
    assert all(T.segment_rows(124, 200, 3, cus=cus) == 24 for cus in (64, 256, 304))


def test_rect_rows_reach_both_left_edges_and_lane_63():
    rows = {c["name"]: c for c in T.rows_of("rects")}
    assert sorted(T.rect_of(c)[0] for c in rows.values() if c["form"] == "bp") == [4, 4, 4, 8, 8, 120, 120, 124, 124]
    assert sorted(T.rect_of(c)[0] for c in rows.values() if c["form"] is None) == [2, 2, 6, 6]
    l, _, W, _ = T.rect_of(rows["rects_248_left124"])
    assert (l, W) == (124, 124) and T.last_block_lanes(W)[0] == 63
    assert T.rect_of(rows["rects_132_left4_x40_seam"]) == (4, 0, 128, 40) and len(T.segments(128, 40)) == 2
    for c in rows.values():                               # every rect ends at the frame's right edge and starts at its top
        l, t, W, H = T.rect_of(c)
        assert l + W == c["w"] and t == 0 and H == c["h"]
