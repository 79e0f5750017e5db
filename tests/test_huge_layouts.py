"""The inputs of tests/test_huge_layouts_gpu.py are the ones intended — shown with the restated arithmetic alone (tests/huge_layouts.py): for every
(case, class) drawn there the pitch is one mpcvr_set_input / mpcvr_process accept, the product lies on the side of the boundary the class names,
the restated guard says what the class name says, the allocation stays within 10 GiB, and `over` puts at least 8 drawn rows beyond the boundary."""
import pytest

from tests import huge_layouts as HL
from tests.golden.cases import case_geometry
from tests.sample_layouts import frame_bytes, row_bytes
from tests.test_sample_layout_gpu import chroma_layout, takes_fast_convert
from videorenderer_amd import synth

TARGET_LAYOUTS = [(n, cls) for n in HL.TARGETS for cls in HL.TARGET_CLASSES]
SAMPLE_LAYOUTS = [(n, cls) for n, (_, _, classes) in HL.SAMPLES.items() for cls in classes]


@pytest.mark.parametrize("name,cls", TARGET_LAYOUTS)
def test_target_pitches(name, cls):
    c = HL.TARGETS[name][0]
    (ww, wh), vr = case_geometry(c)
    rows, drawn, window_rows = HL.target_rows(c)
    pitch = HL.target_pitch(c, cls)
    assert pitch % 16 == 0 and ww * 4 <= pitch <= HL.INT32_MAX
    assert rows == max(vr[1], 0) + c["dst"][1] and drawn <= window_rows == wh
    excluded = HL.g3(pitch, vr[1], c["dst"][1])
    if cls == "under":
        assert pitch * rows < HL.B32 <= (pitch + 16) * rows and not excluded
    elif cls == "at":
        assert (pitch - 16) * rows < HL.B32 <= pitch * rows and excluded
    else:
        assert excluded and pitch & (pitch - 1) and pitch >= HL.pitch_at(rows, HL.B32) * 5 // 4
        assert HL.rows_beyond(pitch, drawn, HL.B32) >= 8
        # a row that wraps lands neither on itself nor on the pixels of another row
        assert HL.wrapped_rows_clear(pitch, drawn, HL.B32) and ww * 4 + HL.BATCH_BASES[-1] <= HL.CLEAR
    assert HL.target_alloc(pitch, wh) <= HL.LIMIT


def test_batches_and_far_targets_fit():
    for route in HL.BATCH_ROUTES:
        c = HL.TARGETS[route][0]
        (ww, wh), _ = case_geometry(c)
        for cls in HL.BATCH_CLASSES:
            pitch = HL.target_pitch(c, cls)
            assert HL.BATCH_BASES[-1] + ww * 4 <= HL.CLEAR <= pitch       # side by side inside the row's padding, clear of a wrapped row
            assert all(b % 16 == 0 for b in HL.BATCH_BASES)
            assert HL.target_alloc(pitch, wh) <= HL.LIMIT
    (ww, wh), _ = case_geometry(HL.TARGETS["up2x_lanczos3"][0])
    assert max(HL.FAR_BASES) - min(HL.FAR_BASES) > HL.B32 and HL.target_alloc(ww * 4, wh, max(HL.FAR_BASES)) <= HL.LIMIT


@pytest.mark.parametrize("name,cls", SAMPLE_LAYOUTS)
def test_sample_pitches(name, cls):
    c = HL.SAMPLES[name][0]
    cf, w, h = c["cformat"], c["w"], c["h"]
    pitch = HL.sample_pitch(c, cls)
    assert pitch % 16 == 0 and HL.legal_pitch(cf, w, pitch) and pitch >= row_bytes(cf, w)
    assert takes_fast_convert(cf, h, pitch), "nothing but the 32-bit guards decides the route"
    _, off1, off2 = chroma_layout(cf, h, pitch)
    r = c.get("src_rect", (0, 0, w, h))
    excluded = HL.sample_excluded(c, pitch)
    assert excluded == (cls != "under")
    # G2 fires before G1 (tests/huge_layouts.py): wherever G1 holds, G2 does
    assert not HL.g1(pitch, r[1], r[3] - r[1]) or HL.g2(cf, h, pitch)
    assert off2 > off1 == pitch * h
    if cls == "under":
        assert off2 < HL.B31 <= chroma_layout(cf, h, pitch + 16)[2]
    elif cls == "at":
        # the second clause of G2 has its own boundary: the third plane (or, for fewer planes, the sum the library forms all the same) is at
        # or beyond 2^31 while the second is still below
        assert chroma_layout(cf, h, pitch - 16)[2] < HL.B31 <= off2 and off1 < HL.B31
    elif cls == "over":
        assert off1 >= HL.B31 and pitch & (pitch - 1) and HL.rows_beyond(pitch, h, HL.B31) >= 8
    else:
        assert cls == "beyond" and 1.09 * HL.B32 <= off1 <= 1.11 * HL.B32 and pitch & (pitch - 1)
    assert HL.sample_alloc(cf, w, h, pitch) <= HL.LIMIT


def test_every_route_and_class_of_the_issue_is_drawn():
    assert {k for _, k, g in HL.TARGETS.values() if g} >= {"fused_up2x", "fused_jinc2x", "kernel=fused_period(", "kernel=fused_strip("}
    assert all(set(classes) <= set(HL.SAMPLE_CLASSES) for _, _, classes in HL.SAMPLES.values())
    assert synth.FORMATS[HL.SAMPLES["yuv420p10_third_plane"][0]["cformat"]][0] == 3
    assert HL.SAMPLES["rgb32_beyond"][2] == HL.SAMPLES["v210_beyond"][2] == ("beyond",)
    # every target case names a kernel: "" would make the `under` class's route assertion hold for anything
    assert all(k for _, k, _ in HL.TARGETS.values())
    # the clipped geometry cannot be the exact-2x kernel's (the video rect starts above and left of the window): it pins the max(off_y, 0) of G3
    c = HL.TARGETS["up2x_clipped"][0]
    assert c["offset"][1] < 0 and HL.target_rows(c)[0] == c["dst"][1] > HL.target_rows(c)[1]


def test_standalone_pass_surface_spans_4_gib():
    # (the rows span 4 GiB; the last of them start beyond 2^31, where a signed 32-bit row offset goes negative)
    assert HL.PASS_PITCH * HL.PASS_H >= HL.B32 and HL.PASS_PITCH * (HL.PASS_H - 1) >= HL.B31 and HL.PASS_PITCH % 16 == 0 and HL.PASS_PITCH & (HL.PASS_PITCH - 1)
    # the RGB surface alone, and the luma plane with the chroma plane behind it (PASS_H / 2 rows at the same pitch)
    assert HL.LEAD + HL.PASS_PITCH * (HL.PASS_H + HL.PASS_H // 2) + HL.CHECK_TEMP <= HL.LIMIT
