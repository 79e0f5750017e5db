"""mpcvr_process_batch_yuv on the GPU (extension: a batch written as NV12 / P010, include/mpcvr.h): the planes against the composition the
header defines them by — mpcvr_process_batch into window-sized RGB targets, then mpcvr_encode_pass per frame — and against the numpy model
of the pass over those RGB targets, per batch route; plane layouts, the letterbox, the refusals, mpcvr_get_last_batch_info, and the batch
lanes against stream order.  Everything is byte-for-byte equality.  The layout integers and the plane-overlap scan: tests/test_batch_yuv.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import encode_model as EM
from tests.golden.cases import GOLDEN_CASES, HDR10, M709, MPEG2, SETTING_KEYS, TV, case_frame, case_geometry, ext
from tests.test_encode_gpu import BGRA8, NV12, P010, RGB10A2, CarvedPlane, description
from tests.test_parity_gpu import make_vp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def noise_frames(torch, c, n, seed0=0):
    c = dict(c, kind="noise")
    return [torch.from_numpy(case_frame(dict(c, seed=c["seed"] + seed0 + 100 * i))[0]).cuda() for i in range(n)]


def plane_pitch(ww, out10):
    """the smallest legal pitch of a plane row: a multiple of 4 (NV12 rows of w = 2 (mod 4) bytes are padded by two)"""
    return (ww * (2 if out10 else 1) + 3) & ~3


def new_planes(torch, n, ww, wh, out10, fill=0):
    pitch = plane_pitch(ww, out10)
    ys = [torch.full((wh, pitch), fill, dtype=torch.uint8, device="cuda") for _ in range(n)]
    uvs = [torch.full((wh // 2, pitch), fill, dtype=torch.uint8, device="cuda") for _ in range(n)]
    return ys, uvs, pitch


def composition(torch, vp, frames, ww, wh, src_fmt, out_cformat, desc):
    """what the header defines the planes by: mpcvr_process_batch into window-sized RGB targets (black: the letterbox is never written), then
    mpcvr_encode_pass per frame.  -> (Y planes, UV planes, the RGB targets read back as (h, w) uint32)"""
    from videorenderer_amd import api
    out10 = out_cformat == P010
    rgb = [torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda") for _ in frames]
    vp.ProcessBatch(frames, rgb, ww * 4)
    vp.Synchronize()
    ys, uvs, pitch = new_planes(torch, len(frames), ww, wh, out10)
    for t, y, uv in zip(rgb, ys, uvs):
        api.encode_pass(t, ww * 4, src_fmt, ww, wh, out_cformat, desc, y, pitch, uv, pitch)
    torch.cuda.synchronize()
    return ys, uvs, [t.cpu().numpy().view(np.uint32).reshape(wh, ww) for t in rgb]


def pixels(t, ww, out10):
    a = t.cpu().numpy()
    return a.view(np.uint16)[:, :ww] if out10 else a[:, :ww]


# ---- 1. the planes equal the composition and the model, per route ---------------------------------------------------------------------
# (case, extra flags, GetVPInfo fragment of the route, lower bound of the launches a 5-frame batch takes when the route is not a whole-batch
# one, RGB format the context renders, output format, siting).  The windows are the smallest at which the pass's frame dimension can go
# wrong: 258 x 38 around a 256 x 36 video rect (a tail lane in a second wavefront, and a letterbox), exactly 256 wide, and under 64 wide.
ROUTES = {
    # exact 2x, 128 x 18 -> 256 x 36 at (1, 1) of a 258 x 38 window
    "FusedUp2x": (dict(cformat=2, w=128, h=18, kind="noise", seed=811, dst=(256, 36), window=(258, 38), offset=(1, 1), exfmt=HDR10, iUpscaling=4),
                  0, "fused_up2x", BGRA8, NV12, EM.LEFT),
    # 1.5x through the strip / periodic kernel, 40 x 24 -> 60 x 36, a 10-bit target
    "Strip": (dict(cformat=2, w=40, h=24, kind="noise", seed=812, dst=(60, 36), iUpscaling=4, output_format=1),
              0, "kernel=fused_", RGB10A2, P010, EM.TOPLEFT),
    # same-size block convert, exactly 256 wide
    "DirectConvert": (dict(cformat=1, w=256, h=36, kind="noise", seed=813, dst=(256, 36), exfmt=ext(matrix=M709)),
                      0, "direct:convert", BGRA8, P010, EM.CENTRE),
    # a quarter turn: the whole-batch launches of the pass-per-kernel path, 48 x 40
    "WholeBatchLaunches": (dict(GOLDEN_CASES["rot90_two_pass_down_up"], output_format=1), 0, "rot90", RGB10A2, NV12, EM.LEFT),
    # interleaved RGB, same size: repacked one by one, frame by frame; 46 = 2 (mod 4), under 64
    "FrameByFrame": (GOLDEN_CASES["rgb24_same_size"], 0, "", BGRA8, NV12, EM.TOPLEFT),
    # the HDR10 tone-mapping step behind the strip kernel (two frame tables per chunk in front of the planes' own)
    "StripToneMap": (GOLDEN_CASES["hdrout_tm2_reinhard"], 0, "hdr10tonemap", RGB10A2, P010, EM.CENTRE),
    # bUseDither = 2: the error-diffusion pass writes the surface, the planes' pass follows it on the context stream
    "ErrorDiffusion": (dict(cformat=2, w=64, h=36, kind="noise", seed=817, dst=(128, 72), exfmt=HDR10, iUpscaling=4, bUseDither=2),
                       0, "errdiff", BGRA8, NV12, EM.LEFT),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_planes_equal_process_batch_then_encode_pass_and_the_model(mpcvr, torch_cuda, route):
    from videorenderer_amd import api
    torch = torch_cuda
    c, flags, fragment, src_fmt, out_cformat, siting = ROUTES[route]
    out10 = out_cformat == P010
    assert c.get("output_format", 0) == src_fmt
    desc = description(out_cformat, siting)
    plan = api.plan_encode(out_cformat, src_fmt, desc)
    assert plan["siting"] == siting
    vp, (ww, wh) = make_vp(mpcvr, c, flags)
    n = 5
    frames = noise_frames(torch, c, n)
    want_y, want_uv, rgb = composition(torch, vp, frames, ww, wh, src_fmt, out_cformat, desc)
    whole = vp.GetLastBatchInfo()
    info = vp.GetVPInfo()
    assert fragment in info, (route, info)
    if route == "FrameByFrame":
        assert whole["launches"] >= n, (route, whole, info)
    elif route != "ErrorDiffusion":
        assert whole["launches"] <= 4, (route, whole, info)
    # chunks of 2, 2 and 1
    lay = api.plan_batch_yuv(ww, wh, n, 0)
    vp.SetBatchYuvBudget(2 * lay["frame_stride"])
    assert api.plan_batch_yuv(ww, wh, n, 2 * lay["frame_stride"])["chunks"] == 3
    ys, uvs, pitch = new_planes(torch, n, ww, wh, out10)
    vp.ProcessBatchYuv(frames, out_cformat, desc, ys, pitch, uvs, pitch)
    vp.Synchronize()
    got = vp.GetLastBatchInfo()
    assert got["frames"] == n and got["yuv_chunks"] == 3 and len(got["yuv_lanes"]) == 3, got
    assert fragment in vp.GetVPInfo(), (route, vp.GetVPInfo())
    for i in range(n):
        assert torch.equal(ys[i], want_y[i]), (route, "Y of frame %d differs from mpcvr_process_batch + mpcvr_encode_pass" % i, got)
        assert torch.equal(uvs[i], want_uv[i]), (route, "UV of frame %d differs from mpcvr_process_batch + mpcvr_encode_pass" % i, got)
        # ... and the model over the RGB targets read back: the test does not rest on the library alone
        my, muv = EM.encode420(rgb[i], src_fmt, out10, plan["coef"], plan["off"], plan["shift"], siting)
        assert np.array_equal(pixels(ys[i], ww, out10), my) and np.array_equal(pixels(uvs[i], ww, out10), muv), (route, "frame %d differs from the model" % i)
    assert not torch.equal(ys[0], ys[1]) and bool((ys[0] != ys[0][0, 0]).any()), route          # (distinct frames, and not flat ones)
    # the same call again with the default budget (one chunk) into fresh planes: the surface is reused, nothing is cleared per call
    vp.SetBatchYuvBudget(0)
    ys2, uvs2, _ = new_planes(torch, n, ww, wh, out10, fill=0x5a)
    vp.ProcessBatchYuv(frames[::-1], out_cformat, desc, ys2, pitch, uvs2, pitch)
    vp.Synchronize()
    assert vp.GetLastBatchInfo()["yuv_chunks"] == 1
    row = ww * (2 if out10 else 1)
    for i in range(n):
        j = n - 1 - i
        assert torch.equal(ys2[i][:, :row], want_y[j][:, :row]) and torch.equal(uvs2[i][:, :row], want_uv[j][:, :row]), (route, "one chunk", i)
        assert bool((ys2[i][:, row:] == 0x5a).all()) and bool((uvs2[i][:, row:] == 0x5a).all()), (route, "pitch padding written", i)
    vp.close()


def test_the_route_cases_cover_formats_sitings_and_window_shapes():
    pairs = {(r[3], r[4]) for r in ROUTES.values()}
    assert pairs == {(BGRA8, NV12), (BGRA8, P010), (RGB10A2, NV12), (RGB10A2, P010)}
    assert {r[5] for r in ROUTES.values()} == {EM.CENTRE, EM.LEFT, EM.TOPLEFT}
    widths = {case_geometry(r[0])[0][0] for r in ROUTES.values()}
    assert 258 in widths and 256 in widths and any(w < 64 for w in widths)


# ---- 2. plane layouts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_cformat", [P010, NV12], ids=["p010", "nv12"])
def test_planes_of_one_batch_at_different_alignments(mpcvr, torch_cuda, out_cformat):
    """The planes of the frames of ONE batch carved at +0, +4 and +8 from 256-byte boundaries at a padded pitch, chunks of two (frames at
    +0 and +4 share a launch: P010's 8-byte stores must step aside for the whole launch; the frame at +8 has one of its own, which takes
    them): every byte outside the planes' pixels survives, and the pixels equal a run into tight planes of their own."""
    from videorenderer_amd import api
    torch = torch_cuda
    c, flags, fragment, src_fmt, _, _ = ROUTES["FusedUp2x"]
    out10 = out_cformat == P010
    siting = EM.TOPLEFT
    desc = description(out_cformat, siting)
    vp, (ww, wh) = make_vp(mpcvr, c, flags)
    bases = (0, 4, 8)
    frames = noise_frames(torch, c, len(bases), seed0=7)
    ys, uvs, pitch = new_planes(torch, len(bases), ww, wh, out10)
    vp.ProcessBatchYuv(frames, out_cformat, desc, ys, pitch, uvs, pitch)
    vp.Synchronize()
    row = ww * (2 if out10 else 1)
    padded = ((row + 15) & ~15) + 24                    # a multiple of 8, not of 16
    assert padded % 8 == 0 and padded % 16 != 0
    for budget_frames in (2, 0):
        vp.SetBatchYuvBudget(budget_frames * api.plan_batch_yuv(ww, wh, 3, 0)["frame_stride"])
        cy = [CarvedPlane(torch, wh, row, padded, b) for b in bases]
        cuv = [CarvedPlane(torch, wh // 2, row, padded, b) for b in bases]
        vp.ProcessBatchYuv(frames, out_cformat, desc, [p.ptr for p in cy], padded, [p.ptr for p in cuv], padded)
        vp.Synchronize()
        assert vp.GetLastBatchInfo()["yuv_chunks"] == (2 if budget_frames else 1)
        for i, b in enumerate(bases):
            what = "frame %d at +%d, pitch %d, chunks of %d" % (i, b, padded, budget_frames)
            cy[i].assert_guards_intact(what + " Y")
            cuv[i].assert_guards_intact(what + " UV")
            assert np.array_equal(cy[i].bytes(), ys[i].cpu().numpy()[:, :row]), what
            assert np.array_equal(cuv[i].bytes(), uvs[i].cpu().numpy()[:, :row]), what
    assert bool(ys[0].any()) and not torch.equal(ys[0], ys[1])
    vp.close()


# ---- 3. the letterbox -------------------------------------------------------------------------------------------------------------------
def test_letterbox_is_black_after_full_window_batches(mpcvr, torch_cuda):
    """Full-window batches fill the context's surface with noise; a batch with a smaller video rect follows.  Process never writes the
    letterbox, so the surface must have been cleared for the new rect: nothing of the earlier frames survives, the letterbox holds the
    code of black (BT.709 limited range: Y 16, C 128), and the planes equal the composition into black RGB targets."""
    torch = torch_cuda
    c = dict(cformat=1, w=96, h=64, kind="noise", seed=831, dst=(96, 64), exfmt=ext(matrix=M709), iUpscaling=2)
    desc = ext(MPEG2, TV, M709)
    vp, (ww, wh) = make_vp(mpcvr, c)
    n = 4
    frames = noise_frames(torch, c, n)
    ys, uvs, pitch = new_planes(torch, n, ww, wh, False)
    for _ in range(2):                                  # (both lanes' surfaces, where the route takes the lanes)
        vp.ProcessBatchYuv(frames, NV12, desc, ys, pitch, uvs, pitch)
    vp.Synchronize()
    assert all(bool((y != 16).any()) for y in ys)
    assert bool((ys[0][:2] != 16).any()) and bool((uvs[0][:, :8] != 128).any())       # the frames reach the window's edges
    vp.SetVideoRect((8, 2, 88, 62))
    want_y, want_uv, _ = composition(torch, vp, frames, ww, wh, BGRA8, NV12, desc)
    for rep in range(2):
        vp.ProcessBatchYuv(frames, NV12, desc, ys, pitch, uvs, pitch)
        vp.Synchronize()
        for i in range(n):
            y, uv = ys[i].cpu().numpy(), uvs[i].cpu().numpy()
            # rows 0-1 and 62-63, columns 0-7 and 88-95 (left siting: the chroma block at column 88 reads column 87)
            for part in (y[:2], y[62:], y[:, :8], y[:, 88:]):
                assert (part == 16).all(), (rep, i, "luma of the letterbox")
            for part in (uv[:1], uv[31:], uv[:, :8], uv[:, 90:]):
                assert (part == 128).all(), (rep, i, "chroma of the letterbox")
            assert (y[2:62, 8:88] != 16).any()
            assert torch.equal(ys[i], want_y[i]) and torch.equal(uvs[i], want_uv[i]), (rep, i)
    vp.close()


# ---- 4. refusals write nothing ------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_keep_the_sample(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    c = GOLDEN_CASES["c1_nv12_bt709_passthrough"]       # 128 x 72, same size
    desc = ext(MPEG2, TV, M709)
    n = 3
    frames = noise_frames(torch, c, n + 1)
    ww, wh = 128, 72
    plane = ww * wh
    buf = torch.full((n * 2 * plane + 4096,), 0x5a, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    y0 = [base + i * 2 * plane for i in range(n)]      # Y, then UV, then half a plane of room, per frame
    uv0 = [p + plane for p in y0]
    arr = C.c_void_p * n

    def call(vp, n=n, srcs="ok", ys=y0, uvs=uv0, yp=ww, uvp=ww, cf=NV12, ex=desc):
        s = arr(*[f.data_ptr() for f in frames[:3]]) if srcs == "ok" else srcs
        return L.mpcvr_process_batch_yuv(vp._ctx, n, s, cf, ex, arr(*ys) if ys is not None else None, yp, arr(*uvs) if uvs is not None else None, uvp)

    # before mpcvr_set_input
    bare = api.VideoProcessor(api.default_settings())
    assert call(bare) == api.E_NOT_VALID_STATE
    bare.close()
    vp, _ = make_vp(mpcvr, c)
    vp.CopySample(frames[n], vp.GetFrameBytes()[1])
    shown = torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda")
    vp.Process(shown, ww * 4)
    vp.Synchronize()
    E, Pn = api.E_INVALIDARG, api.E_POINTER
    some_null = [y0[0], None, y0[2]]
    for kw, hr in ((dict(n=0), E), (dict(n=-1), E),
                   (dict(cf=30), E), (dict(cf=3), E),                                   # neither NV12 nor P010
                   (dict(cf=0), E), (dict(cf=14), E),                                  # none, YV12
                   (dict(yp=ww + 2), E), (dict(uvp=ww + 6), E), (dict(yp=ww - 4), E), (dict(uvp=ww - 4), E),      # multiple-of-4 and row-size rules
                   (dict(ys=[y0[0] + 2] + y0[1:]), E), (dict(uvs=uv0[:2] + [uv0[2] + 1]), E),
                   (dict(uvs=[y0[0] + ww * (wh - 1)] + uv0[1:]), E),                    # UV of frame 0 starts in its own Y's last row
                   (dict(ys=[y0[0], y0[0], y0[2]]), E),                                 # one Y plane given twice
                   (dict(ys=[y0[0], uv0[2] + ww, y0[2]]), E),                           # Y of frame 1 over UV of frame 2
                   (dict(uvs=[uv0[0], uv0[0] + ww * (wh // 2 - 1), uv0[2]]), E),        # UV of frame 1 starts in the last row of UV of frame 0
                   (dict(srcs=None), Pn), (dict(ys=None), Pn), (dict(uvs=None), Pn),
                   (dict(ys=some_null), Pn), (dict(uvs=[uv0[0], uv0[1], None]), Pn),
                   (dict(srcs=arr(frames[0].data_ptr(), None, frames[2].data_ptr())), Pn)):
        assert call(vp, **kw) == hr, kw
    # an odd window width or height
    for odd in ((0, 0, ww - 1, wh), (0, 0, ww, wh - 1)):
        vp.SetWindowRect(odd)
        assert call(vp) == E, odd
    vp.SetWindowRect((0, 0, ww, wh))
    vp.Synchronize()
    torch.cuda.synchronize()
    assert bool((buf == 0x5a).all()), "a refused call wrote into the planes"
    # the sample handed over before is still the current one: Process draws it again, into a second target
    again = torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda")
    vp.Process(again, ww * 4)
    vp.Synchronize()
    assert torch.equal(again, shown) and bool(shown.any())
    # ... and the arguments the refusals were derived from are accepted
    assert call(vp) == 0
    vp.Synchronize()
    want_y, want_uv, _ = composition(torch, vp, frames[:n], ww, wh, BGRA8, NV12, desc)
    for i in range(n):
        off = i * 2 * plane
        assert torch.equal(buf[off:off + plane].view(wh, ww), want_y[i]) and torch.equal(buf[off + plane:off + plane + plane // 2].view(wh // 2, ww), want_uv[i]), i
        assert bool((buf[off + plane + plane // 2:off + 2 * plane] == 0x5a).all())
    vp.close()


# ---- 5. mpcvr_get_last_batch_info ------------------------------------------------------------------------------------------------------
def raw_batch_info(vp):
    b = C.create_string_buffer(512)
    assert vp._L.mpcvr_get_last_batch_info(vp._ctx, b, 512) == 0
    return b.value.decode()


def test_last_batch_info_counts_the_passes_and_names_the_chunks(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    c, flags, fragment, src_fmt, out_cformat, siting = ROUTES["FusedUp2x"]
    desc = description(out_cformat, siting)
    vp, (ww, wh) = make_vp(mpcvr, c, flags)
    n = 8
    frames = noise_frames(torch, c, n)
    rgb = [torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    vp.ProcessBatch(frames, rgb, ww * 4)
    vp.Synchronize()
    plain = vp.GetLastBatchInfo()
    text = raw_batch_info(vp)
    assert "yuv_" not in text and "yuv_chunks" not in plain, text
    assert plain["launches"] == 1 and fragment in vp.GetVPInfo(), (plain, vp.GetVPInfo())        # a one-launch route
    ys, uvs, pitch = new_planes(torch, n, ww, wh, False)
    vp.ProcessBatchYuv(frames, out_cformat, desc, ys, pitch, uvs, pitch)
    vp.Synchronize()
    one = vp.GetLastBatchInfo()
    assert one["frames"] == n and one["launches"] == plain["launches"] + 1 and one["yuv_chunks"] == 1 and len(one["yuv_lanes"]) == 1, one
    assert raw_batch_info(vp).endswith(";yuv_chunks=1;yuv_lanes=%d" % one["yuv_lanes"][0]), raw_batch_info(vp)
    want = [y.clone() for y in ys]
    # one frame per chunk: 8 chunks, a draw and a pass each
    vp.SetBatchYuvBudget(api.plan_batch_yuv(ww, wh, n, 0)["frame_stride"])
    vp.ProcessBatchYuv(frames, out_cformat, desc, ys, pitch, uvs, pitch)
    vp.Synchronize()
    eight = vp.GetLastBatchInfo()
    assert eight["frames"] == n and eight["yuv_chunks"] == 8 and len(eight["yuv_lanes"]) == 8 and eight["launches"] == 16, eight
    assert all(torch.equal(a, b) for a, b in zip(ys, want))
    # a plain batch afterwards: the string is what it was
    vp.ProcessBatch(frames, rgb, ww * 4)
    vp.Synchronize()
    assert raw_batch_info(vp) == text
    vp.close()


# ---- 6. the batch lanes equal stream order ------------------------------------------------------------------------------------------------
LANES_CASE = dict(GOLDEN_CASES["c3hdr_p010_pq_lanczos3_2x"])       # 128 x 72 -> 256 x 144, the exact-2x kernel


def play_lanes(torch, own, expect_lanes):
    """Calls of 8 frames in chunks of 4 over a ring of planes that holds three calls' worth and wraps (the fourth and fifth call write what
    the first and second wrote), the last call's planes again straight away from other samples, then ONE mpcvr_process whose RGB target lies
    over the bytes of planes that call still writes.  All planes are pieces of one allocation (frame i: Y, then UV), returned whole."""
    from videorenderer_amd import api
    c = LANES_CASE
    (ww, wh), vr = case_geometry(c)
    nb, n = 5, 8
    frames = noise_frames(torch, c, nb * n + 1, seed0=3)
    kw = {k: c[k] for k in SETTING_KEYS if k in c}
    desc = description(P010, EM.LEFT)
    row = ww * 2
    ysz, uvsz = row * wh, row * wh // 2
    frame_bytes = ysz + uvsz
    ring = 3 * n
    assert ww * 4 * wh <= 2 * frame_bytes               # the RGB target covers the planes of one frame and reaches into the next
    vp = api.VideoProcessor(api.default_settings(**kw), use_torch_stream=not own)
    vp.InitMediaType(c["cformat"], c["w"], c["h"], extfmt=c.get("exfmt", 0))
    vp.SetWindowRect((0, 0, ww, wh)); vp.SetVideoRect(vr)
    vp.SetBatchYuvBudget(4 * api.plan_batch_yuv(ww, wh, n, 0)["frame_stride"])
    buf = torch.full((ring * frame_bytes,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    at = lambda i: buf.data_ptr() + (i % ring) * frame_bytes
    lanes = []

    def batch(b, first):
        ys = [at(first + i) for i in range(n)]
        vp.ProcessBatchYuv(frames[b * n:(b + 1) * n], P010, desc, ys, row, [p + ysz for p in ys], row)
        info = vp.GetLastBatchInfo()
        assert info["yuv_chunks"] == 2, info
        lanes.extend(info["yuv_lanes"])

    for b in range(nb):
        batch(b, b * n)
    last = (nb - 1) * n
    batch(0, last)
    vp.CopySample(frames[nb * n], vp.GetFrameBytes()[1])
    vp.Process(at(last + 2), ww * 4)                    # over Y and UV of frame last + 2 and into Y of frame last + 3
    vp.Synchronize()
    torch.cuda.synchronize()
    out = buf.clone()
    info = vp.GetVPInfo()
    vp.close()
    assert "fused_up2x" in info, info
    assert set(lanes) == set(expect_lanes), (lanes, expect_lanes)
    return out


def test_chunks_on_the_lanes_equal_chunks_in_stream_order(mpcvr, torch_cuda):
    """A context on a caller's stream keeps every chunk in stream order (yuv_lanes all -1); a context that owns its stream deals the chunks
    to the two batch lanes, each with its own RGB surface, and must leave the same bytes — also where a later call writes planes an earlier
    one still writes and where a single frame's RGB target lies over planes in flight.  Three repetitions; MPCVR_NO_BATCH_LANES=1 (read once
    per process: a child process) keeps a context that owns its stream off the lanes."""
    torch = torch_cuda
    lanes_off = os.environ.get("MPCVR_NO_BATCH_LANES") == "1"
    with torch.cuda.stream(torch.cuda.Stream()):        # (torch's default stream is NULL = "the context's own stream")
        want = play_lanes(torch, False, {-1})
    assert bool((want != 7).any())
    for rep in range(3):
        got = play_lanes(torch, True, {-1} if lanes_off else {0, 1})
        if not torch.equal(got, want):
            bad = torch.nonzero(got != want).flatten()
            raise AssertionError("round %d: %d bytes differ from the stream-ordered run, first at %d" % (rep, bad.numel(), int(bad[0])))
    if lanes_off:
        return
    code = ("import os, sys\nsys.path.insert(0, os.getcwd())\nimport torch\nimport videorenderer_amd as V\nimport tests.test_batch_yuv_gpu as t\n"
            "t.test_chunks_on_the_lanes_equal_chunks_in_stream_order(V, torch)\nprint('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MPCVR_NO_BATCH_LANES="1"), capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
