"""The two exact rescalings k_fused_up2x_bp folds into neighbouring FMAs (csrc/vp_fused_up2x_bp.h, stage C of csrc/vp_fused_up2x.h), on the GPU.

  A. the convert output's read-back: (2^23 + q) * inv - 2^23 * inv in one FMA instead of ((2^23 + q) - 2^23) * inv;
  B. the odd luma column's chroma: Un + U0 into matrix coefficients halved on the host instead of fma(Un, .5, U0 * .5) into the matrix' own.

Both are identities (tests/test_up2x_bp_folds.py proves them on the CPU), so the twin must still equal the generic kernel — which has
neither fold and is the reference here (MPCVR_UP2X_NO_BP=1, read at every launch) — BYTE FOR BYTE.  Nothing is compared with the twin alone.

Inputs aimed at the folds' corners:
  * `ramp_neutral` / `ramp_extreme`: a luma ramp through every code of the sample's depth (0 .. 1023 << 6 for P010: below black, the legal
    range, above white) under neutral chroma and under chroma texels drawn from {0, 64, 512, 960, 1023} (NV12: {0, 16, 128, 240, 255}),
    in bands three texels wide — luma below black takes every channel of the convert output to q = 0 and luma above white to the top
    the plan's curve allows, the extreme chroma pushes single channels past either end (fold A's ends), and the sums of fold B run from
    0 + 0 to the largest code twice, equal neighbours inside a band and different ones at its seams;
  * `noise`: seeded full-range noise.
Shapes: 248 x 24 (two strips and an edge wave, one segment), 8 x 8 (the smallest frame the route takes), 126 x 10 (lane 63 holds the rect's
last block), and a batch of three frames.  Plans: P010 behind the PQ table (the headline's instantiation), P010 HLG, P010 without a tail
into R10G10B10A2, NV12 behind a 10-bit internal format, 4 and 6 taps, a ProcAmp setting without hue (a matrix that is not the standard's).
Every launch must report the twin (";up2x=bp"); a matrix with hue has no structural zeros and must report `generic`.
"""
import os

import numpy as np
import pytest

from videorenderer_amd import synth
from tests.test_parity_gpu import BG, _HLG, _PQ, _SDR, make_vp

KNOB = "MPCVR_UP2X_NO_BP"
NV12, P010 = 1, 2
CATMULL, LANCZOS3 = 2, 4
PLANS = {
    "p010_pq_dither8": dict(cformat=P010, exfmt=_PQ, iUpscaling=LANCZOS3),
    "p010_hlg_dither8": dict(cformat=P010, exfmt=_HLG, iUpscaling=LANCZOS3),
    "p010_none_direct10": dict(cformat=P010, exfmt=_SDR, output_format=1, iUpscaling=LANCZOS3),
    "nv12_fast_direct10": dict(cformat=NV12, exfmt=_SDR, iTexFormat=10, output_format=1, iUpscaling=LANCZOS3),
    "p010_pq_4taps": dict(cformat=P010, exfmt=_PQ, iUpscaling=CATMULL),
    "p010_pq_6taps": dict(cformat=P010, exfmt=_PQ, iUpscaling=LANCZOS3, flags=1),
    "p010_pq_procamp": dict(cformat=P010, exfmt=_PQ, iUpscaling=LANCZOS3, procamp=(10.0, 1.2, 0.0, 1.3)),
}
SHAPES = [(248, 24), (8, 8), (126, 10)]
INPUTS = ("ramp_neutral", "ramp_extreme", "noise")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def make_input(cformat, w, h, kind, seed):
    """(uint8 buffer in the bi-planar sample layout, pitch): luma plane, then the interleaved chroma plane of h / 2 rows"""
    wide = cformat == P010
    top = 1023 if wide else 255
    levels = np.array([0, 64, 512, 960, 1023] if wide else [0, 16, 128, 240, 255], np.uint32)
    cw, ch = w // 2, h // 2
    if kind == "noise":
        r = np.random.default_rng(seed)
        y, u, v = r.integers(0, top + 1, (h, w)), r.integers(0, top + 1, (ch, cw)), r.integers(0, top + 1, (ch, cw))
    else:
        i = np.arange(w * h, dtype=np.int64)
        y = (i % (top + 1) if w * h > top else (i * top) // (w * h - 1)).reshape(h, w)       # every code, or the range end to end
        cy, cx = np.mgrid[0:ch, 0:cw]
        if kind == "ramp_neutral":
            u = v = np.full((ch, cw), (top + 1) // 2)
        else:
            # bands three texels wide, so that a band's inside converts from one chroma pair and its seams from two different ones
            u, v = levels[(cx // 3 + cy) % 5], levels[(cx // 15 + 2 * cy + 1) % 5]
    dt = np.uint16 if wide else np.uint8
    shift = 6 if wide else 0
    pitch = synth.default_pitch(cformat, w)                # bytes per row of both planes
    plane = np.zeros((h + ch, pitch // (2 if wide else 1)), dt)
    plane[:h, :w] = (np.asarray(y, np.uint32) << shift).astype(dt)
    plane[h:, 0:w:2] = (np.asarray(u, np.uint32) << shift).astype(dt)
    plane[h:, 1:w:2] = (np.asarray(v, np.uint32) << shift).astype(dt)
    return plane.reshape(-1).view(np.uint8).copy(), pitch


def draw(mpcvr, torch, c, frames, pitch, generic, batch):
    """the frames through Process (one frame) or one ProcessBatch call, the twin allowed or the generic kernel forced
    -> ([pixels per frame], GetVPInfo, reported form)"""
    old = os.environ.pop(KNOB, None)
    if generic:
        os.environ[KNOB] = "1"
    try:
        vp, (ww, wh) = make_vp(mpcvr, c)
        assert vp.GetFrameBytes() == (frames[0].size, pitch)
        dev = [torch.from_numpy(f).cuda() for f in frames]
        dsts = [torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda") for _ in dev]
        if batch:
            vp.ProcessBatch(dev, dsts, ww * 4)
        else:
            vp.CopySample(dev[0], pitch)
            vp.Process(dsts[0], ww * 4)
        vp.Synchronize()
        out = [d.cpu().numpy() for d in dsts], vp.GetVPInfo(), vp.GetUp2xForm()
        vp.close()
        return out
    finally:
        os.environ.pop(KNOB, None)
        if old is not None:
            os.environ[KNOB] = old


def twin_equals_generic(mpcvr, torch, plan, w, h, kinds, batch=False):
    c = dict(PLANS[plan], w=w, h=h, dst=(2 * w, 2 * h))
    made = [make_input(c["cformat"], w, h, k, 2400 + w + 7 * h + n) for n, k in enumerate(kinds)]
    frames, pitch = [m[0] for m in made], made[0][1]
    what = f"{plan} {w}x{h} {'+'.join(kinds)}"
    twin, info, form = draw(mpcvr, torch, c, frames, pitch, False, batch)
    assert info.startswith("fused_up2x") and form == "bp", (what, info, form)
    gen, info_g, form_g = draw(mpcvr, torch, c, frames, pitch, True, batch)
    assert info_g.startswith("fused_up2x") and form_g == "generic", (what, info_g, form_g)
    for i, (a, b) in enumerate(zip(twin, gen)):
        assert not bool((a[..., :3] == BG).all()), (what, i)
        if not np.array_equal(a, b):
            d = np.argwhere(a != b)
            raise AssertionError(f"{what}: frame {i}: the twin differs from the generic kernel in {len(d)} bytes, first at (y, x, ch) = {tuple(d[0])}: "
                                 f"{a[tuple(d[0])]} where the generic kernel has {b[tuple(d[0])]}; rows {sorted(set(d[:, 0]))[:8]}, columns {sorted(set(d[:, 1]))[:8]}")
    return twin


@pytest.mark.gpu
@pytest.mark.parametrize("plan", sorted(PLANS))
def test_folded_twin_equals_generic_kernel(mpcvr, torch_cuda, plan):
    for w, h in SHAPES:
        for kind in INPUTS:
            twin_equals_generic(mpcvr, torch_cuda, plan, w, h, [kind])


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["p010_pq_dither8", "nv12_fast_direct10"])
def test_folded_twin_batch_of_three(mpcvr, torch_cuda, plan):
    out = twin_equals_generic(mpcvr, torch_cuda, plan, 248, 24, list(INPUTS), batch=True)
    assert not np.array_equal(out[0], out[1]) and not np.array_equal(out[1], out[2])
    for i, kind in enumerate(INPUTS):          # a frame of the batch is the frame drawn alone
        single = twin_equals_generic(mpcvr, torch_cuda, plan, 248, 24, [kind])
        # (the single frame's seed differs from its batch seed for noise only: compare the deterministic inputs)
        if kind != "noise":
            assert np.array_equal(out[i], single[0]), (plan, kind)


@pytest.mark.gpu
def test_a_matrix_with_hue_keeps_the_generic_kernel(mpcvr, torch_cuda):
    c = dict(PLANS["p010_pq_dither8"], w=248, h=24, dst=(496, 48), procamp=(0.0, 1.0, 30.0, 1.0))
    f, pitch = make_input(P010, 248, 24, "ramp_extreme", 2499)
    (got,), info, form = draw(mpcvr, torch_cuda, c, [f], pitch, False, False)
    assert info.startswith("fused_up2x") and form == "generic", (info, form)
    (ref,), _, form_g = draw(mpcvr, torch_cuda, c, [f], pitch, True, False)
    assert form_g == "generic" and np.array_equal(got, ref)
