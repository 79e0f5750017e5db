"""mpcvr_render_lut3d and mpcvr_process_batch_lut3d on the GPU (extension: frames through a 3D LUT, include/mpcvr.h): the targets against
the composition the header defines them by — mpcvr_render / mpcvr_process_batch into window-sized RGB targets, then mpcvr_lut3d_pass per
frame — and against the numpy model over those targets: 8- and 10-bit context output across both target formats, a fused route and the plain
route, chunks under a budget, a single frame, a caller's stream and a context that owns its stream, an error-diffusion plan, queue order
and the refusals.  Everything is byte-for-byte equality."""
import ctypes as C

import numpy as np
import pytest

from tests import lut3d_model as LM
from tests.test_batch_tensor_gpu import LANES_OFF, ROUTES, context, noise_frames
from tests.test_lut3d_gpu import pattern, placement, table
from tests.test_measure_gpu import device_words
from tests.test_tensor_gpu import RENDER_CASES, rendered

pytestmark = pytest.mark.gpu

BGRA8, RGB10A2 = LM.BGRA8, LM.RGB10A2
# the routes of tests/test_batch_tensor_gpu.py (64-ish x 32-ish sources): an exact 2x on the fused kernel into a 259 x 39 window with a
# letterbox (a lane route), a quarter turn through the pass-per-kernel path (the context stream) — each with 8- and 10-bit context output
CASES = {
    "FusedUp2x-8bit": (dict(ROUTES["FusedUp2x"][0], output_format=0), ROUTES["FusedUp2x"][1], True),
    "FusedUp2x-10bit": (dict(ROUTES["FusedUp2x"][0], output_format=1), ROUTES["FusedUp2x"][1], True),
    "WholeBatchLaunches-8bit": (dict(ROUTES["WholeBatchLaunches"][0], output_format=0), ROUTES["WholeBatchLaunches"][1], False),
    "WholeBatchLaunches-10bit": (dict(ROUTES["WholeBatchLaunches"][0], output_format=1), ROUTES["WholeBatchLaunches"][1], False),
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def words_of(t, wh, ww):
    return t.cpu().numpy().view(np.uint32).reshape(wh, ww)


def composition(torch, vp, frames, ww, wh, fmt, dev, n, dst_fmt):
    """what the header defines the targets by: mpcvr_process_batch into window-sized RGB targets (black: the letterbox is never written),
    then mpcvr_lut3d_pass per frame.  -> (the targets as one (k, h, w, 4) uint8 tensor, the RGB frames as (h, w) uint32, the launches the
    batch took)"""
    from videorenderer_amd import api
    rgb = [torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda") for _ in frames]
    vp.ProcessBatch(frames, rgb, ww * 4)
    vp.Synchronize()
    launches = vp.GetLastBatchInfo()["launches"]
    want = torch.zeros((len(frames), wh, ww, 4), dtype=torch.uint8, device="cuda")
    for i, t in enumerate(rgb):
        api.lut3d_pass(t, ww * 4, fmt, ww, wh, dev, n, want[i], ww * 4, dst_fmt, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return want, [words_of(t, wh, ww) for t in rgb], launches


@pytest.mark.parametrize("label", list(RENDER_CASES))
def test_render_lut3d_equals_render_then_the_pass_and_leaves_the_back_buffer(mpcvr, torch_cuda, label):
    from videorenderer_amd import api
    torch = torch_cuda
    c = RENDER_CASES[label]
    fmt = c.get("output_format", 0)
    vp, keep, ww, wh = rendered(mpcvr, torch, c)
    vp2, keep2, _, _ = rendered(mpcvr, torch, c)           # a plain render on a second context: its back buffer is the reference surface
    assert vp2.Render(1) == 0
    vp2.Synchronize()
    ptr2, _, bw, bh = vp2.GetBackBuffer()
    assert (bw, bh) == (ww, wh)
    shown2 = vp2.GetDisplayedImage(deep_color=True)
    for n, dst_fmt in ((17, 1 - fmt), (33, fmt)):
        host, dev = table(torch, n)
        want = torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda")
        api.lut3d_pass(ptr2, ww * 4, fmt, ww, wh, dev, n, want, ww * 4, dst_fmt)
        # into a padded target inside a patterned buffer
        pitch = ww * 4 + 12
        before = pattern(wh * pitch + 512)
        buf = torch.from_numpy(before).cuda()
        got = vp.RenderLut3d(dev, n, dst_fmt, out=buf.data_ptr() + 256, out_pitch=pitch)
        assert got is not None
        vp.Synchronize()
        torch.cuda.synchronize()
        frame = device_words(ptr2, ww * wh).reshape(wh, ww)
        model = LM.apply(frame, host, n, fmt, dst_fmt)
        assert np.array_equal(words_of(want, wh, ww), model), "the pass over the plain render differs from the model"
        assert np.array_equal(buf.cpu().numpy(), LM.place(before.copy(), 256, model, pitch)), (label, n, dst_fmt)
        # the back buffer afterwards is the plain frame
        ptr, _, bw1, bh1 = vp.GetBackBuffer()
        assert (bw1, bh1) == (ww, wh) and np.array_equal(device_words(ptr, ww * wh).reshape(wh, ww), frame)
        assert np.array_equal(vp.GetDisplayedImage(deep_color=True)[0], shown2[0])
    # an allocated target, the context's format
    host, dev = table(torch, 17)
    out = vp.RenderLut3d(dev, 17)
    vp.Synchronize()
    assert np.array_equal(words_of(out, wh, ww), LM.apply(frame, host, 17, fmt, fmt))
    # refusals come before anything is drawn: the target over the back buffer, the table over the target, NULLs, a table size
    L, E = vp._L, api.E_INVALIDARG
    ptr = vp.GetBackBuffer()[0]
    keep_buf = buf.clone()
    assert L.mpcvr_render_lut3d(vp._ctx, 1, C.c_void_p(dev.data_ptr()), 17, C.c_void_p(ptr + 4 * ww), 4 * ww, 0) == E
    assert L.mpcvr_render_lut3d(vp._ctx, 1, C.c_void_p(buf.data_ptr() + 256 + 8), 2, C.c_void_p(buf.data_ptr() + 256), pitch, 0) == E
    assert L.mpcvr_render_lut3d(vp._ctx, 1, C.c_void_p(dev.data_ptr()), 66, C.c_void_p(buf.data_ptr() + 256), pitch, 0) == E
    assert L.mpcvr_render_lut3d(vp._ctx, 1, C.c_void_p(dev.data_ptr()), 17, C.c_void_p(buf.data_ptr() + 256), pitch, 2) == E
    assert L.mpcvr_render_lut3d(vp._ctx, 1, C.c_void_p(dev.data_ptr()), 17, C.c_void_p(buf.data_ptr() + 256), 4 * ww - 4, 0) == E
    assert L.mpcvr_render_lut3d(vp._ctx, 1, None, 17, C.c_void_p(buf.data_ptr() + 256), pitch, 0) == api.E_POINTER
    assert L.mpcvr_render_lut3d(vp._ctx, 1, C.c_void_p(dev.data_ptr()), 17, None, pitch, 0) == api.E_POINTER
    vp.Synchronize()
    assert torch.equal(buf, keep_buf)
    vp.close()
    vp2.close()


def test_render_lut3d_without_a_sample(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    _, dev = table(torch, 17)
    vp = api.VideoProcessor(api.default_settings())
    vp.InitMediaType(1, 96, 64)
    vp.SetWindowRect((0, 0, 96, 64))
    vp.SetVideoRect((0, 0, 96, 64))
    out = torch.full((64, 96, 4), 7, dtype=torch.uint8, device="cuda")
    assert vp.RenderLut3d(dev, 17, out=out) is None
    vp.Synchronize()
    assert bool((out == 7).all())
    vp.close()


@pytest.mark.parametrize("own", [False, True], ids=["callers_stream", "own_stream"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_targets_equal_process_batch_then_the_pass_and_the_model(mpcvr, torch_cuda, case, own):
    from videorenderer_amd import api
    torch = torch_cuda
    c, fragment, lane_route = CASES[case]
    fmt = c["output_format"]
    k = 8               # chunks of 3, 3 and 2: unequal, and none of a single frame (which no route puts on a lane)
    with torch.cuda.stream(torch.cuda.Stream()):        # (torch's default stream is NULL = "the context's own stream")
        vp, ww, wh = context(c, own)
        frames = noise_frames(torch, c, k)
        torch.cuda.synchronize()
        on_lanes = own and lane_route and not LANES_OFF
        lay = api.plan_batch_lut3d(ww, wh, k, 0)
        for n, dst_fmt in ((17, BGRA8), (33, RGB10A2)):
            host, dev = table(torch, n)
            want, rgb, plain = composition(torch, vp, frames, ww, wh, fmt, dev, n, dst_fmt)
            assert fragment in vp.GetVPInfo(), (case, vp.GetVPInfo())
            cut = 0                                     # the launches the composition's batches take when cut as the chunks are
            for at in (0, 3, 6):
                part = frames[at:at + 3]
                vp.ProcessBatch(part, [torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda") for _ in part], ww * 4)
                cut += vp.GetLastBatchInfo()["launches"]
            vp.Synchronize()
            # padded targets inside one patterned buffer: what lies between the rows and the frames survives
            pitch = 4 * ww + 16
            before = pattern(k * wh * pitch)
            for budget, chunks, launches in ((3 * lay["frame_stride"], 3, cut + 3), (0, 1, plain + 1)):
                vp.SetBatchYuvBudget(budget)
                assert api.plan_batch_lut3d(ww, wh, k, budget)["chunks"] == chunks
                buf = torch.from_numpy(before).cuda()
                torch.cuda.synchronize()
                vp.ProcessBatchLut3d(frames, dev, n, [buf.data_ptr() + i * wh * pitch for i in range(k)], pitch, dst_fmt)
                vp.Synchronize()
                got = vp.GetLastBatchInfo()
                assert got["frames"] == k and got["lut3d_chunks"] == chunks and got["launches"] == launches and got["lut3d_table"] == placement(n), (case, got)
                assert "yuv_chunks" not in got and "tensor_chunks" not in got, got
                if on_lanes:            # the chunks take turns on the two batch lanes
                    lanes = set(got["lut3d_lanes"])
                    assert len(got["lut3d_lanes"]) == chunks and lanes <= {0, 1} and (chunks == 1 or lanes == {0, 1}), (case, got)
                else:
                    assert got["lut3d_lanes"] == [-1] * chunks, (case, own, got)
                full = before.copy()
                for i in range(k):
                    LM.place(full, i * wh * pitch, words_of(want[i], wh, ww), pitch)
                assert np.array_equal(buf.cpu().numpy(), full), (case, own, n, dst_fmt, "chunks", chunks, got)
            # ... and the model over the RGB frames read back: the test does not rest on the library alone
            for i in range(k):
                assert np.array_equal(words_of(want[i], wh, ww), LM.apply(rgb[i], host, n, fmt, dst_fmt)), (case, "frame %d differs from the model" % i)
            assert not np.array_equal(words_of(want[0], wh, ww), words_of(want[1], wh, ww))
        vp.close()


@pytest.mark.parametrize("case", ["FusedUp2x-10bit", "WholeBatchLaunches-8bit"])
def test_a_batch_of_one_frame(mpcvr, torch_cuda, case):
    torch = torch_cuda
    c, _, _ = CASES[case]
    fmt = c["output_format"]
    host, dev = table(torch, 17)
    vp, ww, wh = context(c, False)
    frames = noise_frames(torch, c, 1)
    want, rgb, plain = composition(torch, vp, frames, ww, wh, fmt, dev, 17, BGRA8)
    out = torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda")
    vp.ProcessBatchLut3d(frames, dev, 17, [out], ww * 4, BGRA8)
    vp.Synchronize()
    got = vp.GetLastBatchInfo()
    assert got["frames"] == 1 and got["lut3d_chunks"] == 1 and got["launches"] == plain + 1 and got["lut3d_lanes"] == [-1], got
    assert torch.equal(out, want[0]) and np.array_equal(words_of(out, wh, ww), LM.apply(rgb[0], host, 17, fmt, BGRA8))
    vp.close()


def test_an_error_diffusion_plan(mpcvr, torch_cuda):
    """bUseDither = 2: the chunks draw through the error-diffusion pass on the context stream, then the table"""
    from videorenderer_amd import api
    torch = torch_cuda
    c = dict(ROUTES["FusedUp2x"][0], bUseDither=api.DITHER_ErrorDiffusion_EXT, output_format=0)
    host, dev = table(torch, 33)
    vp, ww, wh = context(c, True)
    k = 5
    frames = noise_frames(torch, c, k)
    want, rgb, _ = composition(torch, vp, frames, ww, wh, 0, dev, 33, RGB10A2)
    vp.SetBatchYuvBudget(2 * api.plan_batch_lut3d(ww, wh, k, 0)["frame_stride"])
    out = torch.zeros((k, wh, ww, 4), dtype=torch.uint8, device="cuda")
    vp.ProcessBatchLut3d(frames, dev, 33, [out[i] for i in range(k)], ww * 4, RGB10A2)
    vp.Synchronize()
    got = vp.GetLastBatchInfo()
    assert got["lut3d_chunks"] == 3 and got["lut3d_lanes"] == [-1, -1, -1], got
    assert torch.equal(out, want)
    for i in range(k):
        assert np.array_equal(words_of(out[i], wh, ww), LM.apply(rgb[i], host, 33, 0, RGB10A2))
    vp.close()


def test_two_calls_into_overlapping_targets_stay_in_queue_order(mpcvr, torch_cuda):
    """A context that owns its stream deals chunks to the two batch lanes.  Call A writes targets 0 .. 3 of a buffer of five, call B targets
    1 .. 4 from other samples, without a synchronise in between: target 0 is A's, targets 1 .. 4 are B's.  Several rounds, chunks of two, so
    that both lanes hold both calls' chunks."""
    from videorenderer_amd import api
    torch = torch_cuda
    c = CASES["FusedUp2x-10bit"][0]
    host, dev = table(torch, 17)
    vp, ww, wh = context(c, True)
    k = 4
    a, b = noise_frames(torch, c, k, seed0=1), noise_frames(torch, c, k, seed0=2)
    want_a, _, _ = composition(torch, vp, a, ww, wh, 1, dev, 17, BGRA8)
    want_b, _, _ = composition(torch, vp, b, ww, wh, 1, dev, 17, BGRA8)
    vp.SetBatchYuvBudget(2 * api.plan_batch_lut3d(ww, wh, k, 0)["frame_stride"])
    buf = torch.zeros((k + 1, wh, ww, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lanes = set()
    for r in range(4):
        first, second, wf, ws = (a, b, want_a, want_b) if r & 1 == 0 else (b, a, want_b, want_a)
        vp.ProcessBatchLut3d(first, dev, 17, [buf[i] for i in range(k)], ww * 4, BGRA8)
        lanes |= set(vp.GetLastBatchInfo()["lut3d_lanes"])
        vp.ProcessBatchLut3d(second, dev, 17, [buf[i + 1] for i in range(k)], ww * 4, BGRA8)
        info = vp.GetLastBatchInfo()
        lanes |= set(info["lut3d_lanes"])
        vp.Synchronize()
        assert torch.equal(buf[0], wf[0]), "round %d: target 0 is not the first call's" % r
        assert torch.equal(buf[1:], ws), ("round %d: a chunk of the first call overtook the second call's" % r, info)
    assert lanes == ({-1} if LANES_OFF else {0, 1}), lanes
    vp.close()


def test_refusals_write_nothing(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    c = CASES["FusedUp2x-8bit"][0]
    host, dev = table(torch, 17)
    vp, ww, wh = context(c, False)
    k = 3
    frames = noise_frames(torch, c, k)
    base = torch.full((k + 1, wh, ww, 4), 9, dtype=torch.uint8, device="cuda")
    small = torch.from_numpy(LM.identity_entries(2).view(np.int16)).cuda()
    keep_small = small.clone()
    L = vp._L
    arr = C.c_void_p * k
    srcs, dsts = arr(*[f.data_ptr() for f in frames]), arr(*[base[i].data_ptr() for i in range(k)])
    t, P, E = C.c_void_p(dev.data_ptr()), api.E_POINTER, api.E_INVALIDARG
    f = L.mpcvr_process_batch_lut3d
    pitch = ww * 4
    assert f(vp._ctx, k, None, t, 17, dsts, pitch, 0) == P
    assert f(vp._ctx, k, srcs, None, 17, dsts, pitch, 0) == P
    assert f(vp._ctx, k, srcs, t, 17, None, pitch, 0) == P
    assert f(vp._ctx, k, srcs, t, 17, arr(dsts[0], None, dsts[2]), pitch, 0) == P
    assert f(vp._ctx, k, arr(srcs[0], None, srcs[2]), t, 17, dsts, pitch, 0) == P
    assert f(vp._ctx, 0, srcs, t, 17, dsts, pitch, 0) == E
    assert f(vp._ctx, k, srcs, t, 1, dsts, pitch, 0) == E
    assert f(vp._ctx, k, srcs, t, 66, dsts, pitch, 0) == E
    assert f(vp._ctx, k, srcs, t, 17, dsts, pitch, 2) == E
    assert f(vp._ctx, k, srcs, t, 17, dsts, pitch - 4, 0) == E
    assert f(vp._ctx, k, srcs, t, 17, dsts, pitch + 2, 0) == E
    assert f(vp._ctx, k, srcs, t, 17, arr(dsts[0], dsts[1] + 2, dsts[2]), pitch, 0) == E
    assert f(vp._ctx, k, srcs, C.c_void_p(dev.data_ptr() + 4), 17, dsts, pitch, 0) == E
    assert f(vp._ctx, k, srcs, t, 17, arr(dsts[0], dsts[0] + pitch, dsts[2]), pitch, 0) == E          # targets that overlap each other
    assert f(vp._ctx, k, srcs, t, 17, arr(dsts[0], dsts[1], dsts[1]), pitch, 0) == E                   # one target given twice
    assert f(vp._ctx, k, srcs, C.c_void_p(base[1].data_ptr() + 8), 2, dsts, pitch, 0) == E             # the table inside a target
    assert f(vp._ctx, k, srcs, C.c_void_p(small.data_ptr()), 2, arr(dsts[0], dsts[1], small.data_ptr() + 56 - (wh - 1) * pitch - 4 * ww + 4), pitch, 0) == E      # a target that ends in the table
    bare = api.VideoProcessor(api.default_settings())
    assert f(bare._ctx, k, srcs, t, 17, dsts, pitch, 0) == api.E_NOT_VALID_STATE
    bare.close()
    assert "lut3d_chunks" not in vp.GetLastBatchInfo()
    vp.Synchronize()
    torch.cuda.synchronize()
    assert bool((base == 9).all()) and torch.equal(small, keep_small), "a refused call wrote"
    # ... and the arguments the refusals were derived from are accepted
    assert f(vp._ctx, k, srcs, t, 17, dsts, pitch, 0) == 0
    vp.Synchronize()
    want, _, _ = composition(torch, vp, frames, ww, wh, 0, dev, 17, BGRA8)
    assert torch.equal(base[:k], want) and bool((base[k:] == 9).all())
    vp.close()
