"""The smallest frames every fused route accepts, on the GPU (tests/tiny_frames.py holds the table, tests/test_tiny_frames.py its CPU half).

Per family, every case is drawn through run_layouts (all four render-target layouts, the patterned guard bytes around a target of 1 to 28
pixels per row checked) on two tiers:
  * the plain tier (MPCVR_FLAG_NO_FUSED): `passes:`, bit-exact with the oracle, tails included;
  * the default tier: GetVPInfo of the `tight` layout shows the case's route, and every frame is within ONE code of the render target on
    every channel — behind PQ / HLG / Dolby Vision tails too, with no witness and no cap: tests/test_tiny_frames.py shows that the oracle's own
    +-4-ulp pow() interval spans at most one code on every channel of every case.  (R10G10B10A2 targets and 8-bit internal formats in front
    of them keep compare_rgb10's limits.)
The helpers' per-frame share of identical channels does not apply to frames of 12 to 2,000 channels (one channel of an 8 x 2 frame is 2 %):
the colour channels of a family's default-tier frames are pooled and the pool is held to 0.98, the project's floor for small frames on the
default tier (test_random_geometries_tiers_agree, test_random_formats_and_tails_vs_oracle) — here over the colour channels alone, without
the alpha bytes those count as identical.  test_pooled_identical_share_per_family asserts and prints the pools.

Measured on an MI355X when the file was written (default-tier frames over all four layouts; worst |delta| 1 code everywhere):
    exact 2x 136 frames 0.99968 | Jinc2m 2x 48 frames 0.99928 | same size 128 frames 0.99978 | periodic 164 frames 0.99971 (the same through
    MPCVR_FLAG_NO_PERIOD; k_fused_period == k_fused_strip bit for bit on all of them) | any ratio 128 frames 1.00000 | surface mode 48 frames
    1.00000 | plain-family sources through the default planner 192 frames 1.00000.  No frame missed its bar: no bug was found at these sizes.
What the table had to learn from the planner is written into tests/tiny_frames.py and DESIGN.md §4.3 (odd widths in tight windows, 8 x 2 -> 3 x 1,
one-axis resizes, the surface route below the raw-sample gate, rows that are not dword multiples).
"""
import numpy as np
import pytest

from tests import tiny_frames as T
from tests.golden.cases import case_frame, oracle_params
from tests.sample_layouts import frame_bytes, pitch_of, poison_pattern, relayout
from tests.test_parity_gpu import (BG, MIXED_BASES, _codes10, batch_vs_singles_in_carved_targets, has_tail, internal_is_8bit, kernel_under,
                                   layout_of, make_vp, run_layouts, run_product)

pytestmark = pytest.mark.gpu

POOL_FLOOR = 0.98          # identical colour channels over a family's default-tier frames
TWIN_FLOOR = 0.99          # k_fused_period against k_fused_strip on the same launch: the share test_period_kernel_vs_oracle_and_strip_kernel holds
#                            frames under 100 columns to, pooled over the family for the reason above (each frame: <= 1 code)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


_WANT = {}


def oracle_frame(oracle, c):
    """the oracle's window for a case, untouched pixels = BG: computed once, read-only"""
    if c["name"] not in _WANT:
        frame, pitch = case_frame(c)
        p = oracle_params(oracle, c)
        want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
        want.setflags(write=False)
        _WANT[c["name"]] = want
    return _WANT[c["name"]]


def limit_of(c):
    """codes of the render target a default-tier frame may be off by (compare_rgb10's limits for a 10-bit target)"""
    if c.get("output_format", 0) != 1:
        return 1
    return 5 if internal_is_8bit(c) else 2 if has_tail(c) else 1


def hold(c, got, want, what, lim):
    """|delta| <= lim codes on every colour channel, alpha identical; a miss is located (rows and columns).  -> (identical, channels, worst)"""
    assert got.shape == want.shape, what
    if c.get("output_format", 0) == 1:
        g, w = _codes10(got), _codes10(want)
        assert np.array_equal(got.view(np.uint32) >> 30, want.view(np.uint32) >> 30), f"{what}: alpha bits differ"
    else:
        g, w = got[..., :3].astype(np.int16), want[..., :3].astype(np.int16)
        assert np.array_equal(got[..., 3], want[..., 3]), f"{what}: alpha differs"
    d = np.abs(g - w)
    if d.max() > lim:
        bad = np.argwhere(d > lim)
        raise AssertionError(f"{what}: max |delta| = {int(d.max())} > {lim}; {len(bad)} channels, rows {sorted(set(bad[:, 0].tolist()))}, columns "
                             f"{sorted(set(bad[:, 1].tolist()))} of a {got.shape[1]} x {got.shape[0]} window; first (y, x, ch) = {tuple(bad[0])}: got {g[tuple(bad[0])]}, "
                             f"oracle {w[tuple(bad[0])]}")
    return int((d == 0).sum()), int(d.size), int(d.max())


POOL = {}          # pool name -> {case name: (identical, channels, worst, frames)}


def pooled(pool):
    v = list(POOL.get(pool, {}).values())
    same, total = sum(x[0] for x in v), sum(x[1] for x in v)
    return (same / total if total else 1.0), max([x[2] for x in v] or [0]), sum(x[3] for x in v), total


def shows(info, c, layout="tight"):
    for frag in c["route"]:
        assert kernel_under(layout, frag) in info, (c["name"], layout, f"expected {frag}", info)
    for frag in c.get("no_route", ()):
        assert frag not in info, (c["name"], layout, f"must not show {frag}", info)


def check_case(mpcvr, oracle, torch, c):
    """one case on both tiers against the oracle, its route, its twins; the default tier's channels go into the family's pool"""
    from videorenderer_amd import api
    name, family = c["name"], c["family"]
    want = oracle_frame(oracle, c)
    plain = run_layouts(mpcvr, torch, c, extra_flags=api.FLAG_NO_FUSED, what=f"{name} plain")
    for layout, (got, info) in plain.items():
        assert info.startswith("passes:") and "kernel=" not in info and "fused" not in info, (name, layout, info)
        hold(c, got, want, f"{name} plain <{layout}> [{info}]", 0)
    if family == "plain":
        for frag in c["route"]:
            assert frag in plain["tight"][1], (name, plain["tight"][1])
    default = run_layouts(mpcvr, torch, c, what=name)
    lim = limit_of(c)
    exact = bool(c.get("below_gate")) and not has_tail(c) and tuple(c.get("no_route", ())) in (T.FUSED_NAMES, ("kernel=",))
    acc = [0, 0, 0, 0]
    for layout, (got, info) in default.items():
        if family != "plain":
            shows(info, c, layout) if "period" in c else (layout == "tight" and shows(info, c))
        s, n, worst = hold(c, got, want, f"{name} <{layout}> [{info}]", 0 if exact else lim)
        acc = [acc[0] + s, acc[1] + n, max(acc[2], worst), acc[3] + 1]
    POOL.setdefault(family, {})[name] = tuple(acc)

    if "period" in c:            # the twin: the same launch through k_fused_strip, held to the oracle like the case itself and to the case
        strips = run_layouts(mpcvr, torch, c, extra_flags=api.FLAG_NO_PERIOD, what=f"{name} no-period")
        frag = "kernel=fused_strip:surface(" if family == "surface" else "kernel=fused_strip("
        acc, twin = [0, 0, 0, 0], [0, 0, 0, 0]
        for layout, (alt, info_alt) in strips.items():
            assert frag in info_alt and "fused_period" not in info_alt, (name, layout, info_alt)
            s, n, worst = hold(c, alt, want, f"{name} <{layout}> [{info_alt}]", lim)
            acc = [acc[0] + s, acc[1] + n, max(acc[2], worst), acc[3] + 1]
            s, n, worst = hold(c, default[layout][0], alt, f"{name} <{layout}> period vs strip", 1)
            twin = [twin[0] + s, twin[1] + n, max(twin[2], worst), twin[3] + 1]
        POOL.setdefault(family + " (MPCVR_FLAG_NO_PERIOD)", {})[name] = tuple(acc)
        POOL.setdefault(family + " period vs strip", {})[name] = tuple(twin)
        if family == "period" and c["dst"][0] & 1:
            # the same frame in a tight window of its odd width: rows of 44 bytes are not k_fused_period's (8-byte stores) — k_fused_strip draws it
            odd = {k: v for k, v in c.items() if k != "window"}
            odd["name"] = name + "_tight_odd_window"
            got, info = run_product(mpcvr, torch, odd)
            assert "kernel=fused_strip(" in info, (odd["name"], info)
            hold(odd, got, oracle_frame(oracle, odd), f"{odd['name']} [{info}]", lim)
    if family in ("up2x", "strip"):          # folded kernels == plain kernels, bit for bit, where no transcendental tail sits in the convert
        folded, info_f = run_product(mpcvr, torch, c, extra_flags=api.FLAG_NO_FAST_CONVERT)
        assert not any(k in info_f for k in T.FUSED_NAMES), (name, info_f)
        if has_tail(c):
            hold(c, folded, want, f"{name} folded [{info_f}]", lim)
        else:
            assert np.array_equal(folded, plain["tight"][0]), (name, info_f, int((folded != plain["tight"][0]).sum()))


def check_group(mpcvr, oracle, torch, cases):
    for c in cases:
        check_case(mpcvr, oracle, torch, c)


def _params(family, size):
    g = T.groups(family, size)
    return pytest.mark.parametrize("cases", [x[1] for x in g], ids=[x[0] for x in g])


@_params("up2x", 9)
def test_exact_2x_at_the_gate(mpcvr, oracle, torch_cuda, cases):
    """k_fused_up2x on sources of 8 x 8, 10 x 8, 8 x 10 and 14 x 12 (the row prefetch runs past a frame of four row pairs, the halo is wider than
    what is left of the frame), 4 / 5 / 6 taps, nine formats and tails, both epilogues, a 10-bit target; 8 x 6, 8 x 2 (k_fused_strip) and 6 x 8
    (plain kernels) below the gate."""
    check_group(mpcvr, oracle, torch_cuda, cases)


@_params("jinc2x", 6)
def test_jinc_2x_at_the_gate(mpcvr, oracle, torch_cuda, cases):
    check_group(mpcvr, oracle, torch_cuda, cases)


@_params("same", 11)
def test_same_size_at_the_gate(mpcvr, oracle, torch_cuda, cases):
    """k_convert_stream (width % 4 == 0) and k_convert_blocks from 8 x 2, Catmull-Rom chroma over one chroma row, Dolby Vision; 6 x 2 and 4 x 4
    through the per-pixel kernel, bit-exact."""
    check_group(mpcvr, oracle, torch_cuda, cases)


@_params("period", 8)
def test_periodic_ratios_at_the_gate(mpcvr, oracle, torch_cuda, cases):
    """k_fused_period at every built (P, Q) over sources of one to three row pairs (its three-row-pair body runs past the frame, one wave per
    workgroup), odd output widths, one output row; `off4` and MPCVR_FLAG_NO_PERIOD send the same launch through k_fused_strip."""
    check_group(mpcvr, oracle, torch_cuda, cases)


@_params("strip", 8)
def test_any_ratio_at_the_gate(mpcvr, oracle, torch_cuda, cases):
    check_group(mpcvr, oracle, torch_cuda, cases)


@_params("surface", 6)
def test_surface_mode_from_one_pixel(mpcvr, oracle, torch_cuda, cases):
    check_group(mpcvr, oracle, torch_cuda, cases)


@_params("plain", 11)
def test_plain_kernels_on_one_to_six_pixel_sources(mpcvr, oracle, torch_cuda, cases):
    """1 x 1, 1 x 5, 5 x 1, 2 x 2 and 3 x 2 sources to 1 x 1, 2x, 3x and 7 x 3 through all six upscalers and downscalers, every rotation: the plain
    tier bit-exact, the default planner's choice (the surface variants of the fused kernels, mostly) within one code."""
    check_group(mpcvr, oracle, torch_cuda, cases)


def test_pooled_identical_share_per_family(mpcvr, oracle, torch_cuda):
    """The floor the per-frame comparisons cannot carry: >= 0.98 of the colour channels of a family's default-tier frames identical to the
    oracle (and >= 0.99 between k_fused_period and k_fused_strip on the same launch).  Families the tests above did not draw in this
    session (a test selected on its own) are drawn here."""
    for family, cases in T.FAMILIES.items():
        if family != "errdiff":
            check_group(mpcvr, oracle, torch_cuda, [c for c in cases if c["name"] not in POOL.get(family, {})])
    low = []
    for pool in sorted(POOL):
        share, worst, frames, channels = pooled(pool)
        floor = TWIN_FLOOR if pool.endswith("period vs strip") else POOL_FLOOR
        print(f"TINY {pool}: {frames} frames, {channels} colour channels, identical {share:.5f}, worst |delta| {worst}")
        if share < floor:
            low.append((pool, share, floor, sorted((v[0] / v[1], k) for k, v in POOL[pool].items())[:5]))
    assert not low, low


# ---- what the sample's neighbours do ------------------------------------------------------------------------------------------------
GUARD = 4096           # bytes in front of and behind the sample (a multiple of 256: the sample keeps the alignment of a buffer of its own)


@pytest.mark.parametrize("name", T.GATE_CASES)
def test_a_sample_inside_a_larger_buffer_reads_nothing_around_it(mpcvr, torch_cuda, name):
    """The sample as a slice of a larger device buffer, at a row pitch wider than the row, drawn twice with the guard and padding bytes
    holding two different patterns: identical frames, equal to the tight sample's.  A row prefetch or a halo read that runs past a 2-row
    plane into its neighbour (or past the sample) shows here without faulting."""
    torch = torch_cuda
    c = T.CASES[name]
    cf, w, h = c["cformat"], c["w"], c["h"]
    tight, info_tight = run_product(mpcvr, torch, c)
    frame, _ = case_frame(c)
    wide = pitch_of("wide", cf, w)
    vp, (ww, wh) = make_vp(mpcvr, dict(c, pitch=wide))
    assert vp.GetFrameBytes() == (frame_bytes(cf, w, h, wide), wide)
    outs = []
    for poison in (1, 2):
        body = relayout(frame, cf, w, h, wide, poison)
        buf = np.concatenate([poison_pattern(GUARD, poison + 40), body, poison_pattern(GUARD, poison + 80)])
        dev = torch.from_numpy(buf).cuda()
        assert dev.data_ptr() % 256 == 0
        dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        vp.CopySample(dev[GUARD:GUARD + body.size], wide)
        vp.Process(dst, ww * 4)
        vp.Synchronize()
        outs.append(dst.cpu().numpy())
        assert np.array_equal(dev.cpu().numpy(), buf), f"{name}: the sample or its guard bytes were written"
    info = vp.GetVPInfo()
    vp.close()
    assert info == info_tight, (name, info, info_tight)
    shows(info, c)
    assert np.array_equal(outs[0], outs[1]), f"{name} [{info}]: {int((outs[0] != outs[1]).sum())} bytes depend on the bytes around the sample"
    assert np.array_equal(outs[0], tight), f"{name} [{info}]: {int((outs[0] != tight).sum())} bytes differ from the tight sample's frame"


# ---- batches ------------------------------------------------------------------------------------------------------------------------
def batch_equals_singles(torch, vp, c, ww, wh, what):
    c = dict(c, kind="noise")
    frames = [torch.from_numpy(case_frame(dict(c, seed=c["seed"] + 100 * (i + 1)))[0]).cuda() for i in range(5)]
    pitch = vp.GetFrameBytes()[1]
    singles = []
    for f in frames:
        dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        vp.CopySample(f, pitch)
        vp.Process(dst, ww * 4)
        singles.append(dst)
    vp.Synchronize()
    info = vp.GetVPInfo()
    dsts = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in frames]
    vp.ProcessBatch(frames, dsts, ww * 4)
    vp.Synchronize()
    route = vp.GetLastBatchInfo()
    assert route["frames"] == 5, (what, route)
    for i in range(5):
        assert torch.equal(singles[i], dsts[i]), (what, i, info, route)
    assert any(not torch.equal(dsts[0], d) for d in dsts[1:]), what
    # the targets as slices of one patterned buffer with mixed first bytes, at `off8`'s pitch, then `off4`'s
    for layout in ("off8", "off4"):
        mixed = batch_vs_singles_in_carved_targets(torch, vp, frames, pitch, ww, wh, layout_of(layout, ww)[1], MIXED_BASES[:5], f"{what} <{layout}>")
        assert mixed["frames"] == 5, (what, layout, mixed)
    return info, route


@pytest.mark.parametrize("name", T.GATE_CASES)
def test_batches_of_gate_size_frames_equal_single_frames(mpcvr, torch_cuda, name):
    """ProcessBatch of five frames equals the five single frames bit for bit, into targets of their own and into carved targets with mixed
    first bytes: the frame dimension live where a segment is clamped to the frame's height, one slot and one wave per workgroup remain."""
    c = T.CASES[name]
    vp, (ww, wh) = make_vp(mpcvr, c)
    info, _ = batch_equals_singles(torch_cuda, vp, c, ww, wh, name)
    vp.close()
    shows(info, c)


# ---- error diffusion ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in T.FAMILIES["errdiff"]])
def test_error_diffusion_on_rects_of_one_column_one_row_and_a_band_hand_off(mpcvr, oracle, torch_cuda, name):
    """k_error_diffusion against the serial model on the product's own 10-bit frame, every layout: rects 1 .. 3 wide (the two-column skew of the
    bands exceeds the width), one row, 21 / 22 and 43 rows (bands are 21 rows), behind same-size, exact-2x and clipped draws."""
    from tests.test_errdiff import product_10bit_and_diffused, region
    c = T.CASES[name]
    ten, outs, info10, info = product_10bit_and_diffused(mpcvr, torch_cuda, c)
    assert "errdiff" in info and "errdiff" not in info10 and info.startswith(c["plan"]), (info10, info)
    rect, (ww, wh) = region(c)
    assert (rect[2] - rect[0], rect[3] - rect[1]) == c["rect"]
    want = oracle.error_diffusion(ten, rect, dst=np.full((wh, ww, 4), BG, dtype=np.uint8))
    for layout, out in outs.items():
        assert np.array_equal(out, want), f"{name} <{layout}> [{info}]: {int((out != want).any(axis=2).sum())} pixels differ"


@pytest.mark.parametrize("name", ["errdiff_3x21_clipped_same_size", "errdiff_8x43_clipped_2x"])
def test_error_diffusion_batches_equal_single_frames(mpcvr, torch_cuda, name):
    c = T.CASES[name]
    vp, (ww, wh) = make_vp(mpcvr, c)
    info, _ = batch_equals_singles(torch_cuda, vp, c, ww, wh, name)
    vp.close()
    assert "errdiff" in info, info
