"""k_fused_up2x_bp, the bi-planar twin of the exact-2x fused kernel (csrc/vp_fused_up2x_bp.h), on the GPU.

The twin loads and converts every chroma texel once (one chroma load per iteration: the row above is carried, the column to the right
comes from the next lane) and leaves out the two matrix FMAs whose coefficient is a structural zero.  It computes the generic kernel's
values with the generic kernel's operations, so

  * twin == generic kernel (MPCVR_UP2X_NO_BP=1, read at every launch) BIT FOR BIT, and both within the bars tests/test_parity_gpu.py
    holds this plan to against the oracle (8-bit targets: compare(): <= 1 code, >= 0.99 identical; 10-bit targets: compare_rgb10()):
      - P010 PQ -> 8-bit with dither (the headline plan), NV12 BT.709 behind a 10-bit internal format -> 10-bit direct store (the fast
        form of the convert stage: the only NV12 plan the twin serves.  NV12 -> 8-bit direct takes an 8-bit internal format and with it
        the EXACT form of the convert stage, k_fused_up2x<.., XC_ALWAYS>, which the twin does not have: that launch must report `generic`);
      - width 384: three strips — a left-edge wave, an interior one, a right-edge one (24 columns); width 122: one wave that is both edges;
      - height 40: the launcher's segment rule gives small frames 24-row segments (what MPCVR_FUSED_SEG=24 would force; that knob is read
        once per process), so two segments, a seam at row 24, and the top and bottom clamps inside the run-in / run-out;
      - height 8, the lowest frame the exact-2x route accepts (FusedUp2xSupported: out_h >= 8), barely longer than the run-in of three
        iterations; height 6 is drawn too: the route refuses it, no exact-2x kernel runs, and the frame still equals the oracle's bars;
      - a two-frame batch; each of the three tap counts;
  * every instantiation of the twin is launched and compared with its generic counterpart (tests/test_kernel_coverage.py needs a
    witness for each: taps x {PQ, HLG, none} x {dither8, direct10} for P010, taps x direct10 for NV12);
  * launches that must NOT take the twin report `generic` (or no exact-2x kernel at all) and still match the oracle: a source rect whose
    top row is odd, a hue-rotated ProcAmp matrix (m[1] != 0), a rect that ends short of the frame's right edge or starts below its top,
    NV12 in the exact convert form, 4:2:2 and 4:4:4 samples.
"""
import os

import numpy as np
import pytest

from tests.golden.cases import case_frame, oracle_params
from tests.test_parity_gpu import BG, _HLG, _PQ, _SDR, CarvedTargets, compare, compare_rgb10, has_tail, internal_is_8bit, make_vp

KNOB = "MPCVR_UP2X_NO_BP"
TAPS = {4: dict(iUpscaling=2), 5: dict(iUpscaling=4), 6: dict(iUpscaling=4, flags=1)}      # Catmull-Rom, Lanczos3 (Q1 folded), Lanczos3 fixed
PLANS = {
    "p010_pq_dither8": dict(cformat=2, exfmt=_PQ),
    "nv12_fast_direct10": dict(cformat=1, exfmt=_SDR, iTexFormat=10, output_format=1),
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def case_of(plan, w, h, taps=5, seed=9100, **over):
    c = dict(PLANS[plan] if isinstance(plan, str) else plan, w=w, h=h, kind="noise", seed=seed + w + 7 * h + taps, dst=(2 * w, 2 * h))
    c.update(TAPS[taps])
    c.update(over)
    return c


def draw(mpcvr, torch, c, generic, batch=0, distinct=2, sample_off=0, target_off=0):
    """The case as a single frame (batch = 0) or a batch of `batch` frames that cycle through `distinct` samples (sample k: the case's seed
    + 1000 k), with the twin allowed or the generic kernel forced -> ([pixels per frame], GetVPInfo, reported form).  sample_off / target_off:
    a single frame whose sample / render target starts that many bytes behind a 256-byte boundary (the target then in the `off4` layout
    of tests/test_parity_gpu.py: a patterned buffer around it, a pitch of window_w * 4 + 4)."""
    old = os.environ.pop(KNOB, None)
    if generic:
        os.environ[KNOB] = "1"
    try:
        vp, (ww, wh) = make_vp(mpcvr, c)
        frames = []
        for i in range(distinct if batch else 1):
            f, pitch = case_frame(dict(c, seed=c["seed"] + 1000 * i))
            frames.append(torch.from_numpy(f).cuda())
        if batch:
            dsts = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in range(batch)]
            vp.ProcessBatch([frames[i % distinct] for i in range(batch)], dsts, ww * 4)
        else:
            if sample_off:
                big = torch.zeros(frames[0].numel() + 256, dtype=torch.uint8, device="cuda")
                big[sample_off:sample_off + frames[0].numel()] = frames[0]
                frames[0] = big[sample_off:sample_off + frames[0].numel()]
                assert frames[0].data_ptr() % 256 == sample_off
            carved = CarvedTargets(torch, ww, wh, ww * 4 + 4, [target_off]) if target_off else None
            dsts = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")]
            vp.CopySample(frames[0], pitch)
            if carved:
                assert carved.ptrs[0] % 256 == target_off
                vp.Process(carved.ptrs[0], carved.pitch)
            else:
                vp.Process(dsts[0], ww * 4)
        vp.Synchronize()
        if not batch and carved:
            carved.assert_guards_intact(f"target at +{target_off} [{vp.GetVPInfo()}]")
            dsts = [carved.window(0).contiguous()]
        out = [d.cpu().numpy() for d in dsts], vp.GetVPInfo(), vp.GetUp2xForm()
        vp.close()
        return out
    finally:
        os.environ.pop(KNOB, None)
        if old is not None:
            os.environ[KNOB] = old


def against_oracle(oracle, c, got, what, seed_shift=0):
    cc = dict(c, seed=c["seed"] + seed_shift)
    frame, pitch = case_frame(cc)
    po = oracle_params(oracle, cc)
    want = oracle.process(po, frame, pitch, dst=np.full((po.window_h, po.window_w, 4), BG, dtype=np.uint8))
    if c.get("output_format", 0) == 1:
        compare_rgb10(got, want, what, tail=has_tail(c), internal8=internal_is_8bit(c))
    else:
        compare(got, want, what, min_same=0.99)


def twin_equals_generic(mpcvr, torch, c, what, batch=0, **layout):
    twin, info, form = draw(mpcvr, torch, c, False, batch, **layout)
    assert info == "fused_up2x" and form == "bp", (what, info, form)
    gen, info_g, form_g = draw(mpcvr, torch, c, True, batch, **layout)
    assert info_g == "fused_up2x" and form_g == "generic", (what, info_g, form_g)
    for i, (a, b) in enumerate(zip(twin, gen)):
        assert not bool((a[..., :3] == BG).all()), (what, i)
        if not np.array_equal(a, b):
            d = np.argwhere(a != b)
            raise AssertionError(f"{what}: frame {i}: the twin differs from the generic kernel in {len(d)} bytes, first at (y, x, ch) = {tuple(d[0])}: "
                                 f"{a[tuple(d[0])]} where the generic kernel has {b[tuple(d[0])]}; rows {sorted(set(d[:, 0]))[:8]}, columns {sorted(set(d[:, 1]))[:8]}")
    return twin


@pytest.mark.gpu
@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("w,h", [(384, 40), (122, 40), (384, 8)], ids=["three_strips_two_segments", "one_wave_both_edges", "lowest_frame"])
def test_twin_equals_generic_kernel_and_meets_the_oracle(mpcvr, oracle, torch_cuda, plan, w, h):
    c = case_of(plan, w, h)
    twin = twin_equals_generic(mpcvr, torch_cuda, c, f"{plan} {w}x{h}")
    against_oracle(oracle, c, twin[0], f"{plan} {w}x{h} [twin]")


@pytest.mark.gpu
@pytest.mark.parametrize("taps", [4, 6])
def test_other_tap_counts(mpcvr, oracle, torch_cuda, taps):
    c = case_of("p010_pq_dither8", 122, 40, taps=taps)
    twin = twin_equals_generic(mpcvr, torch_cuda, c, f"{taps} taps")
    against_oracle(oracle, c, twin[0], f"{taps} taps [twin]")


@pytest.mark.gpu
def test_two_frame_batch(mpcvr, oracle, torch_cuda):
    c = case_of("p010_pq_dither8", 384, 40)
    twin = twin_equals_generic(mpcvr, torch_cuda, c, "batch of two", batch=2)
    single = twin_equals_generic(mpcvr, torch_cuda, c, "single frame")
    assert np.array_equal(twin[0], single[0])
    assert not np.array_equal(twin[0], twin[1])
    against_oracle(oracle, c, twin[1], "batch of two, second frame [twin]", seed_shift=1000)


@pytest.mark.gpu
def test_frames_the_exact_2x_route_refuses_run_no_twin(mpcvr, oracle, torch_cuda):
    c = case_of("p010_pq_dither8", 384, 6)           # shorter than the run-in: below the route's eight rows
    (got,), info, form = draw(mpcvr, torch_cuda, c, False)
    assert info != "fused_up2x" and form is None, (info, form)
    against_oracle(oracle, c, got, f"384x6 [{info}]")


_TAILS = {"pq": _PQ, "hlg": _HLG, "none": _SDR}
_EPIS = {"dither8": {}, "direct10": dict(output_format=1)}


@pytest.mark.gpu
@pytest.mark.parametrize("taps", sorted(TAPS))
@pytest.mark.parametrize("tail", sorted(_TAILS))
def test_every_instantiation_of_the_twin(mpcvr, torch_cuda, tail, taps):
    """k_fused_up2x_bp<taps, tail, P01x, dither8 | direct> and, without a tail, <taps, none, NV12, direct>: each against the generic
    instantiation it stands in for (which this also keeps launched, now that default launches of these plans take the twin)."""
    for epi, over in sorted(_EPIS.items()):
        c = case_of(dict(cformat=2, exfmt=_TAILS[tail], **over), 64, 40, taps=taps, seed=9300)
        twin_equals_generic(mpcvr, torch_cuda, c, f"p010 {tail} {epi} {taps} taps")
    if tail == "none":
        c = case_of("nv12_fast_direct10", 64, 40, taps=taps, seed=9400)
        twin_equals_generic(mpcvr, torch_cuda, c, f"nv12 direct10 {taps} taps")


NOT_TWIN = {
    # rect top 1: odd rows pair with other chroma rows
    "odd_rect_top": dict(PLANS["p010_pq_dither8"], w=128, h=42, src_rect=(0, 1, 128, 41), dst=(256, 80)),
    # a rect that starts below the frame's top on an even row: the rows clamped above it repeat a chroma row pair that is not the frame's first
    "rect_below_the_top": dict(PLANS["p010_pq_dither8"], w=128, h=44, src_rect=(0, 4, 128, 44), dst=(256, 80)),
    # a rect that ends short of the frame's right edge: the lanes clamped there need a texel beyond the rect
    "rect_short_of_the_right_edge": dict(PLANS["p010_pq_dither8"], w=136, h=40, src_rect=(0, 0, 128, 40), dst=(256, 80)),
    # hue rotation: R depends on U and B on V (m[1], m[8] != 0)
    "hue_rotated_procamp": dict(PLANS["p010_pq_dither8"], w=128, h=40, dst=(256, 80), procamp=(0.0, 1.0, 30.0, 1.0)),
    # NV12 -> 8-bit direct: the exact form of the convert stage
    "nv12_exact_direct8": dict(cformat=1, exfmt=_SDR, w=128, h=40, dst=(256, 80)),
    "p210_422": dict(cformat=6, exfmt=_PQ, w=128, h=40, dst=(256, 80)),
    "yuv444p10": dict(cformat=24, exfmt=_PQ, w=128, h=40, dst=(256, 80)),
    "y410_444": dict(cformat=12, exfmt=_PQ, w=128, h=40, dst=(256, 80)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(NOT_TWIN))
def test_launches_that_must_not_take_the_twin(mpcvr, oracle, torch_cuda, name):
    c = dict(NOT_TWIN[name], kind="noise", seed=9500 + len(name), iUpscaling=4)
    (got,), info, form = draw(mpcvr, torch_cuda, c, False)
    assert form != "bp", (name, info, form)
    if info == "fused_up2x":
        assert form == "generic", (name, info, form)
    against_oracle(oracle, c, got, f"{name} [{info}, {form}]")
