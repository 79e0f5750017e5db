"""Frames whose rows span 2 GiB and 4 GiB (tests/huge_layouts.py has the guards, the pitches and the buffer; tests/test_huge_layouts.py shows on the
CPU that every layout drawn here lies where its class says).

Tiny pictures (64 x 32) at pitches of tens of MiB — a tile of a video wall inside one pooled surface looks like that — on the default tier and on
the plain tier (MPCVR_FLAG_NO_FUSED), each drawn twice into / from a buffer filled with byte 1, then byte 2:
  * the bars of tests/test_parity_gpu.py against the oracle's frame of the TIGHT sample: plain tier exact, default tier <= 1 code and >= 99 %
    identical, behind a PQ / HLG tail compare_behind_tail with its defaults;
  * fill 1 == fill 2, bit for bit;
  * just below a limit == the tight layout's frame, bit for bit, where GetVPInfo is the same string; on the plain tier every class == tight;
  * every byte of the allocation outside the drawn rows' pixels still holds the fill byte (2 GiB in front of the frame included): a row
    addressed modulo 2^32 shows up as a written word with its row and column, not as a fault;
  * just below a limit GetVPInfo names the route's fast kernel; at and beyond it, read after the frame, it names none the restated guard excludes.
"""
import numpy as np
import pytest

from tests import encode_model as EM
from tests import huge_layouts as HL
from tests import measure_model as MM
from tests.golden.cases import case_frame, case_geometry, oracle_params
from tests.sample_layouts import frame_bytes, plane_walk
from tests.test_encode_gpu import NV12, P010, description, noise_surface
from tests.test_parity_gpu import BG, compare, compare_behind_tail, compare_rgb10, has_tail, internal_is_8bit, make_vp
from tests.test_sample_layout_gpu import FAST_KERNELS, TIERS, names, tier_flags
pytestmark = pytest.mark.gpu

FILLS = (1, 2)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


# ---- drawing ---------------------------------------------------------------------------------------------------------------------------
def tight_sample(c):
    """the case's picture at the default pitch: (uint8 bytes, pitch)"""
    frame, pitch = case_frame(dict(c, bottom_up=0, pitch=None))
    return np.ascontiguousarray(frame).view(np.uint8).ravel(), pitch


def drawn_rect(c):
    (ww, wh), vr = case_geometry(c)
    return max(vr[0], 0), max(vr[1], 0), min(vr[2], ww), min(vr[3], wh)


def target_view(hb, c, pitch, base=0):
    x0, y0, x1, y1 = drawn_rect(c)
    return hb.rows(base + y0 * pitch + x0 * 4, y1 - y0, (x1 - x0) * 4, pitch)


def window_of(hb, c, view):
    """the window as the caller sees it: BG outside the video rect (assert_rest_intact holds those bytes to the fill value), the drawn rows inside"""
    (ww, wh), _ = case_geometry(c)
    x0, y0, x1, y1 = drawn_rect(c)
    out = np.full((wh, ww, 4), BG, dtype=np.uint8)
    out[y0:y1, x0:x1] = hb.read(view).reshape(y1 - y0, x1 - x0, 4)
    return out


def draw_into(vp, hb, c, sample, spitch, pitch, what, base=0):
    """one frame into the huge-pitch target `base` bytes behind the buffer's frame start -> (window, GetVPInfo read after the frame)"""
    vp.CopySample(sample, spitch)
    vp.Process(hb.ptr + base, pitch)
    vp.Synchronize()
    info = vp.GetVPInfo()
    view = target_view(hb, c, pitch, base)
    out = window_of(hb, c, view)
    hb.assert_rest_intact([view], f"{what} [{info}]", pitch)
    return out, info


_TIGHT = {}


def tight_frame(mpcvr, torch, c, tier):
    """(window, GetVPInfo) of the case in tensors of their own at the default pitches: once per (case, tier), read-only"""
    key = (repr(sorted((k, repr(v)) for k, v in c.items())), tier)
    if key not in _TIGHT:
        vp, (ww, wh) = make_vp(mpcvr, c, tier_flags(tier))
        frame, pitch = tight_sample(c)
        dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
        vp.CopySample(torch.from_numpy(frame).cuda(), pitch)
        vp.Process(dst, ww * 4)
        vp.Synchronize()
        out, info = dst.cpu().numpy(), vp.GetVPInfo()
        vp.close()
        out.setflags(write=False)
        _TIGHT[key] = (out, info)
    return _TIGHT[key]


def against_oracle(oracle, c, got, tier, what):
    """the bars of tests/test_parity_gpu.py (test_pass_per_kernel_path_vs_oracle, test_default_path_vs_oracle) against the oracle's frame of the
    tight sample: the oracle reads no padding byte (tests/test_sample_layouts.py)"""
    frame, pitch = tight_sample(c)
    p = oracle_params(oracle, c)
    want = oracle.process(p, frame, pitch, dst=np.full((p.window_h, p.window_w, 4), BG, dtype=np.uint8))
    if c.get("output_format", 0) == 1:
        if tier == "plain":
            compare_rgb10(got, want, what, exact=True)
        else:
            compare_rgb10(got, want, what, tail=has_tail(c), internal8=internal_is_8bit(c))
    elif tier == "plain":
        compare(got, want, what, exact=True)
    elif has_tail(c):
        compare_behind_tail(oracle, p, frame, pitch, got, want, what, min_same=0.99)
    else:
        compare(got, want, what, min_same=0.99)


def no_fast_kernel(info):
    return not any(k in info for k in FAST_KERNELS)


# ---- the render target (G3) --------------------------------------------------------------------------------------------------------------
def check_tight(mpcvr, torch, oracle, name, c, kernel, tier):
    """the tight layout's frame of a case, held to the oracle and to its route once per (case, tier)"""
    ref, ref_info = tight_frame(mpcvr, torch, c, tier)
    if (name, tier) not in _CHECKED:
        if c.get("bUseDither") == 2:
            # (no oracle draws this plan: the pass against its serial model on the tier's own 10-bit frame, as smoke() has it)
            ten, _ = tight_frame(mpcvr, torch, dict(c, output_format=1), tier)
            assert np.array_equal(ref, oracle.error_diffusion(np.ascontiguousarray(ten).view(np.uint32)[:, :, 0])), f"{name} <{tier}> tight"
        else:
            against_oracle(oracle, c, ref, tier, f"{name} <tight> <{tier}> [{ref_info}]")
        assert ref_info.startswith("passes:") if tier == "plain" else names(ref_info, kernel), (name, tier, ref_info)
        _CHECKED.add((name, tier))
    return ref, ref_info


_CHECKED = set()


@pytest.mark.parametrize("cls", HL.TARGET_CLASSES)
@pytest.mark.parametrize("name", sorted(HL.TARGETS))
def test_target_rows_span_4_gib(mpcvr, oracle, torch_cuda, name, cls):
    torch = torch_cuda
    c, kernel, guarded = HL.TARGETS[name]
    errdiff = c.get("bUseDither") == 2
    (ww, wh), vr = case_geometry(c)
    pitch = HL.target_pitch(c, cls)
    assert HL.g3(pitch, vr[1], c["dst"][1]) == (cls != "under")
    frame, spitch = tight_sample(c)
    sample = torch.from_numpy(frame).cuda()
    hb = HL.HugeBuffer(torch, pitch * wh, FILLS[0])
    try:
        for tier in TIERS:
            ref, ref_info = check_tight(mpcvr, torch, oracle, name, c, kernel, tier)
            vp, _ = make_vp(mpcvr, c, tier_flags(tier))
            what = f"{name} <{cls}: dst_pitch {pitch}> <{tier}>"
            outs = []
            for fill in FILLS:
                hb.refill(fill)
                got, info = draw_into(vp, hb, c, sample, spitch, pitch, f"{what} fill {fill}")
                outs.append(got)
            vp.close()
            what += f" [{info}]"
            print("HUGE", "target", name, cls, pitch, tier, info, sep="\t")
            assert np.array_equal(outs[0], outs[1]), f"{what}: {int((outs[0] != outs[1]).sum())} bytes depend on the bytes around the target"
            if tier == "plain":
                assert info.startswith("passes:"), what
                assert np.array_equal(outs[0], ref), f"{what}: {int((outs[0] != ref).sum())} bytes differ from the tight target's frame"
            elif cls == "under":
                # a fix must not switch the fast path off for padded targets
                assert info == ref_info, f"{what}: the tight target runs [{ref_info}]"
                assert np.array_equal(outs[0], ref), f"{what}: {int((outs[0] != ref).sum())} bytes differ from the tight target's frame"
            elif guarded:
                assert no_fast_kernel(info), f"{what}: a kernel with 32-bit row offsets is named for rows that span 4 GiB"
            if not guarded and not kernel.startswith("direct:convert"):
                # the pitch reaches k_errdiff / k_hdr10_tonemap alone, and they store through size_t: the fused kernel in front of them draws
                # into a surface of the context's at every class — the same kernels, the same frame
                assert info == ref_info, f"{what}: the tight target runs [{ref_info}]"
                assert np.array_equal(outs[0], ref), f"{what}: {int((outs[0] != ref).sum())} bytes differ from the tight target's frame"
            if not errdiff:
                against_oracle(oracle, c, outs[0], tier, what)
    finally:
        del sample
        hb.free()


# ---- batches -------------------------------------------------------------------------------------------------------------------------------
def batch_into(vp, hb, c, samples, spitch, pitch, bases, what):
    views = [target_view(hb, c, pitch, b) for b in bases]
    vp.ProcessBatch(samples, [hb.ptr + b for b in bases], pitch)
    vp.Synchronize()
    info = vp.GetVPInfo()
    assert vp.GetLastBatchInfo()["frames"] == len(bases)
    outs = [window_of(hb, c, v) for v in views]
    hb.assert_rest_intact(views, f"{what} [{info}]", pitch)
    return outs, info


def check_batch(mpcvr, torch, oracle, hb, c0, kernel, pitch, bases, expect, what):
    """Three different pictures of case c0 into the targets at `bases` of `hb`, on both tiers and with both fill bytes: every frame == the single
    frame of the same layout (drawn at bases[0]) bit for bit, fill 1 == fill 2, on the plain tier == the tight target's frame, the rest of the
    allocation intact after every draw.  expect: "fast" — GetVPInfo of the default tier names `kernel`, "aside" — it names no fast kernel."""
    cases = [dict(c0, seed=c0["seed"] + 50 * k) for k in range(len(bases))]
    samples = [torch.from_numpy(tight_sample(c)[0]).cuda() for c in cases]
    spitch = tight_sample(c0)[1]
    for tier in TIERS:
        vp, _ = make_vp(mpcvr, c0, tier_flags(tier))
        per_fill = []
        for fill in FILLS:
            hb.refill(fill)
            singles = []
            for k, c in enumerate(cases):
                got, info = draw_into(vp, hb, c, samples[k], spitch, pitch, f"{what} <{tier}> fill {fill} single frame {k}", bases[0])
                singles.append(got)
            outs, binfo = batch_into(vp, hb, c0, samples, spitch, pitch, bases, f"{what} <{tier}> fill {fill}")
            for k in range(len(bases)):
                assert np.array_equal(outs[k], singles[k]), (f"{what} <{tier}> fill {fill}: frame {k} of the batch differs from the single frame in "
                                                             f"{int((outs[k] != singles[k]).sum())} bytes [{binfo}]")
            per_fill.append(outs)
        vp.close()
        print("HUGE", "batch", what, pitch, tier, binfo, sep="\t")
        assert not np.array_equal(per_fill[0][0], per_fill[0][1])
        for k, c in enumerate(cases):
            assert np.array_equal(per_fill[0][k], per_fill[1][k]), f"{what} <{tier}>: frame {k} of the batch depends on the bytes around the targets [{binfo}]"
            ref, ref_info = tight_frame(mpcvr, torch, c, tier)
            if tier == "plain":
                assert info.startswith("passes:") and binfo.startswith("passes:"), (what, info, binfo)
                assert np.array_equal(per_fill[0][k], ref), f"{what} <plain>: frame {k} differs from the tight target's frame"
            elif expect == "fast":
                assert names(info, kernel) and binfo == ref_info, (what, info, binfo, ref_info)
                assert np.array_equal(per_fill[0][k], ref), f"{what} <default>: frame {k} differs from the tight target's frame [{binfo}]"
            else:
                assert no_fast_kernel(info) and no_fast_kernel(binfo), (what, info, binfo)
            against_oracle(oracle, c, per_fill[0][k], tier, f"{what} <{tier}> batch frame {k} [{binfo}]")
    del samples


@pytest.mark.parametrize("cls", HL.BATCH_CLASSES)
@pytest.mark.parametrize("route", HL.BATCH_ROUTES)
def test_batch_into_targets_side_by_side_in_huge_rows(mpcvr, oracle, torch_cuda, route, cls):
    """three targets that share the same huge-pitch rows (byte 0, 1024 and 2048 of the row)"""
    torch = torch_cuda
    c0, kernel, _ = HL.TARGETS[route]
    (ww, wh), _ = case_geometry(c0)
    pitch = HL.target_pitch(c0, cls)
    hb = HL.HugeBuffer(torch, pitch * wh, FILLS[0])
    try:
        check_batch(mpcvr, torch, oracle, hb, c0, kernel, pitch, HL.BATCH_BASES, "fast" if cls == "under" else "aside", f"batch {route} <{cls}>")
    finally:
        hb.free()


def test_batch_into_targets_more_than_4_gib_apart(mpcvr, oracle, torch_cuda):
    """the frame table carries 64-bit pointers: three tight targets of one allocation, the second 4 GiB behind the others"""
    torch = torch_cuda
    c0, kernel, _ = HL.TARGETS["up2x_lanczos3"]
    (ww, wh), _ = case_geometry(c0)
    hb = HL.HugeBuffer(torch, max(HL.FAR_BASES) + ww * 4 * wh, FILLS[0])
    try:
        check_batch(mpcvr, torch, oracle, hb, c0, kernel, ww * 4, HL.FAR_BASES, "fast", "batch into targets 4 GiB apart")
    finally:
        hb.free()


# ---- the sample (G2; G1 lies behind it) ------------------------------------------------------------------------------------------------------
def lay_sample(torch, hb, c, pitch):
    """the tight picture, uploaded tight and copied plane by plane into strided views of the buffer at `pitch` (frame_bytes / plane_walk offsets) -> the views"""
    frame, tp = tight_sample(c)
    dev = torch.from_numpy(frame).cuda()
    cf, w, h = c["cformat"], c["w"], c["h"]
    views = []
    for (so, rows, sp, rb), (do, drows, dp, drb) in zip(plane_walk(cf, w, h, tp), plane_walk(cf, w, h, pitch)):
        assert (rows, rb) == (drows, drb)
        views.append(hb.rows(do, rows, rb, dp))
        views[-1].copy_(dev[so: so + rows * sp].view(rows, sp)[:, :rb])
    return views


@pytest.mark.parametrize("name", sorted(HL.SAMPLES))
def test_sample_planes_at_2_gib_and_beyond(mpcvr, oracle, torch_cuda, name):
    from videorenderer_amd import api
    torch = torch_cuda
    c, kernel, classes = HL.SAMPLES[name]
    cf, w, h = c["cformat"], c["w"], c["h"]
    (ww, wh), _ = case_geometry(c)
    pitches = {cls: HL.sample_pitch(c, cls) for cls in classes}
    hb = HL.HugeBuffer(torch, max(frame_bytes(cf, w, h, p) for p in pitches.values()), FILLS[0])
    try:
        for tier in TIERS:
            ref, ref_info = tight_frame(mpcvr, torch, c, tier)
            against_oracle(oracle, c, ref, tier, f"{name} <tight> <{tier}> [{ref_info}]")
            if tier != "plain":
                assert names(ref_info, kernel), (name, ref_info)
            for cls, pitch in pitches.items():
                assert HL.sample_excluded(c, pitch) == (cls != "under")
                vp, _ = make_vp(mpcvr, dict(c, pitch=pitch), tier_flags(tier))
                assert vp.GetFrameBytes() == (frame_bytes(cf, w, h, pitch), pitch), "GetFrameBytes: pitch * lines as a 64-bit value"
                outs = []
                for fill in FILLS:
                    hb.refill(fill)
                    planes = lay_sample(torch, hb, c, pitch)
                    dst = torch.full((wh, ww, 4), BG, dtype=torch.uint8, device="cuda")
                    vp.CopySample(hb.ptr, pitch, mem_kind=api.MEM_DEVICE)
                    vp.Process(dst, ww * 4)
                    vp.Synchronize()
                    outs.append(dst.cpu().numpy())
                    # nothing writes into the caller's sample allocation (its pixel rows are read-only too: they are compared, then refilled)
                    for v, (so, rows, sp, rb) in zip(planes, plane_walk(cf, w, h, tight_sample(c)[1])):
                        assert np.array_equal(hb.read(v), tight_sample(c)[0][so: so + rows * sp].reshape(rows, sp)[:, :rb]), f"{name} <{cls}> <{tier}>: the sample's pixels changed"
                    hb.assert_rest_intact(planes, f"{name} <{cls}: pitch {pitch}> <{tier}> fill {fill}: the sample's allocation", pitch)
                    del planes
                info = vp.GetVPInfo()
                vp.close()
                what = f"{name} <{cls}: pitch {pitch}> <{tier}> [{info}]"
                print("HUGE", "sample", name, cls, pitch, tier, info, sep="\t")
                assert np.array_equal(outs[0], outs[1]), f"{what}: {int((outs[0] != outs[1]).sum())} bytes depend on the bytes around the sample's rows"
                if tier == "plain":
                    assert info.startswith("passes:"), what
                    assert np.array_equal(outs[0], ref), f"{what}: {int((outs[0] != ref).sum())} bytes differ from the tight sample's frame"
                elif cls == "under":
                    assert info == ref_info, f"{what}: the tight sample runs [{ref_info}]"       # (one-plane samples too: the sums are formed anyway)
                    assert np.array_equal(outs[0], ref), f"{what}: {int((outs[0] != ref).sum())} bytes differ from the tight sample's frame"
                else:
                    assert no_fast_kernel(info), f"{what}: a kernel with 32-bit plane offsets is named for planes at or beyond 2 GiB"
                against_oracle(oracle, c, outs[0], tier, what)
    finally:
        hb.free()


# ---- standalone passes over a surface whose rows span more than 4 GiB ------------------------------------------------------------------------
W, H, PITCH = HL.PASS_W, HL.PASS_H, HL.PASS_PITCH


def words(view_bytes):
    return np.ascontiguousarray(view_bytes).view(np.uint32).reshape(H, W)


@pytest.mark.parametrize("side", ["source", "destination"])
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("kind", [5, 1])
def test_correction_pass_over_huge_rows(mpcvr, oracle, torch_cuda, kind, fmt, side):
    """one PQ kind and one matrix kind: against the oracle the way test_correction_passes_vs_oracle does, and == the pass over tight surfaces"""
    from videorenderer_amd import api
    torch = torch_cuda
    rng = np.random.default_rng(2000 + kind * 10 + fmt)
    src = rng.integers(0, 1 << 32, size=(H, W), dtype=np.uint64).astype(np.uint32)
    src[0, :8] = [0, 0xffffffff, 0x3ff, 0x3ff << 10, 0x3ff << 20, 0x00ff0000, 0x0000ff00, 0x000000ff]
    want = oracle.correction_pass(kind, src, 10 if fmt else 8, 10 if fmt else 8, sdr_nits=125)
    d_src = torch.from_numpy(src.view(np.int32)).cuda()
    d_ref = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    api.correction_pass(kind, d_src, W * 4, fmt, d_ref, W * 4, fmt, W, H, sdr_nits=125)
    torch.cuda.synchronize()
    ref = d_ref.cpu().numpy().view(np.uint32)
    hb = HL.HugeBuffer(torch, PITCH * H, FILLS[0])
    try:
        view = hb.rows(0, H, W * 4, PITCH)
        if side == "source":
            view.copy_(d_src.view(torch.uint8).view(H, W * 4))
            d_got = torch.zeros((H, W), dtype=torch.int32, device="cuda")
            api.correction_pass(kind, hb.ptr, PITCH, fmt, d_got, W * 4, fmt, W, H, sdr_nits=125)
            torch.cuda.synchronize()
            got = d_got.cpu().numpy().view(np.uint32)
        else:
            api.correction_pass(kind, d_src, W * 4, fmt, hb.ptr, PITCH, fmt, W, H, sdr_nits=125)
            torch.cuda.synchronize()
            got = words(hb.read(view))
        hb.assert_rest_intact([view], f"correction {kind} fmt {fmt}, huge {side}", PITCH)
    finally:
        view = None
        hb.free()
    what = f"correction {kind} fmt {fmt}, pitch {PITCH} on the {side}"
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f"{what}: {len(bad)} texels differ from the tight surfaces' result, the first in row {bad[0][0]}"
    if fmt:
        compare_rgb10(got.reshape(H, W, 1).view(np.uint8).reshape(H, W, 4), want.reshape(H, W, 1).view(np.uint8).reshape(H, W, 4), what)
    else:
        compare(got.view(np.uint8).reshape(H, W, 4), want.view(np.uint8).reshape(H, W, 4), what, min_same=0.99)


@pytest.mark.parametrize("side", ["rgb", "planes"])
@pytest.mark.parametrize("out_cformat", [NV12, P010])
def test_encode_pass_over_huge_rows(mpcvr, torch_cuda, out_cformat, side):
    """k_encode420 byte for byte against tests/encode_model.py: NV12 from BGRA8, P010 from RGB10A2"""
    from videorenderer_amd import api
    torch = torch_cuda
    out10 = out_cformat == P010
    src_fmt = 1 if out10 else 0
    desc = description(out_cformat, EM.LEFT)
    plan = api.plan_encode(out_cformat, src_fmt, desc)
    surface = noise_surface(W, H, src_fmt, seed=2100 + out_cformat)
    want_y, want_uv = EM.encode420(surface, src_fmt, out10, plan["coef"], plan["off"], plan["shift"], plan["siting"])
    row = W * (2 if out10 else 1)
    d_src = torch.from_numpy(surface.view(np.int32)).cuda()
    hb = HL.HugeBuffer(torch, PITCH * (H if side == "rgb" else H + H // 2), FILLS[0])
    try:
        if side == "rgb":
            view = hb.rows(0, H, W * 4, PITCH)
            view.copy_(d_src.view(torch.uint8).view(H, W * 4))
            y = torch.zeros((H, row), dtype=torch.uint8, device="cuda")
            uv = torch.zeros((H // 2, row), dtype=torch.uint8, device="cuda")
            api.encode_pass(hb.ptr, PITCH, src_fmt, W, H, out_cformat, desc, y, row, uv, row)
            torch.cuda.synchronize()
            got_y, got_uv = y.cpu().numpy(), uv.cpu().numpy()
            hb.assert_rest_intact([view], f"encode {out_cformat}, huge RGB surface", PITCH)
        else:
            vy, vuv = hb.rows(0, H, row, PITCH), hb.rows(H * PITCH, H // 2, row, PITCH)
            api.encode_pass(d_src, W * 4, src_fmt, W, H, out_cformat, desc, hb.ptr, PITCH, hb.ptr + H * PITCH, PITCH)
            torch.cuda.synchronize()
            got_y, got_uv = hb.read(vy), hb.read(vuv)
            hb.assert_rest_intact([vy, vuv], f"encode {out_cformat}, huge planes", PITCH)
    finally:
        view = vy = vuv = None
        hb.free()
    if out10:
        got_y, got_uv = np.ascontiguousarray(got_y).view(np.uint16), np.ascontiguousarray(got_uv).view(np.uint16)
    what = f"encode {out_cformat}, pitch {PITCH} on the {side}"
    assert np.array_equal(got_y, want_y), (what, "Y", np.argwhere(got_y != want_y)[:4])
    assert np.array_equal(got_uv, want_uv), (what, "UV", np.argwhere(got_uv != want_uv)[:4])


@pytest.mark.parametrize("fmt", [0, 1])
def test_measure_pass_over_huge_rows(mpcvr, torch_cuda, fmt):
    """k_measure_maxrgb word for word against tests/measure_model.py over a rectangle that includes the last row"""
    from videorenderer_amd import api
    torch = torch_cuda
    surface = noise_surface(W, H, fmt, seed=2200 + fmt)
    rect = (3, 5, 61, H)
    hb = HL.HugeBuffer(torch, PITCH * H, FILLS[0])
    try:
        view = hb.rows(0, H, W * 4, PITCH)
        view.copy_(torch.from_numpy(surface.view(np.int32)).cuda().view(torch.uint8).view(H, W * 4))
        hist = torch.zeros(MM.BINS, dtype=torch.int32, device="cuda")
        api.measure_pass(hb.ptr, PITCH, fmt, W, H, hist, rect=rect)
        torch.cuda.synchronize()
        got = hist.cpu().numpy().view(np.uint32).astype(np.int64)
        hb.assert_rest_intact([view], f"measure fmt {fmt}", PITCH)
    finally:
        view = None
        hb.free()
    assert np.array_equal(got, MM.hist(surface, fmt, rect)), f"measure fmt {fmt}, pitch {PITCH}"
