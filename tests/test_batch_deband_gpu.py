"""mpcvr_process_batch_deband on the GPU (extension: debanding of rendered frames, include/mpcvr.h): the targets against the composition
the header defines them by — mpcvr_process_batch into window-sized RGB targets, then mpcvr_deband_pass per frame with seed + i — and
against the numpy model over those targets: 3- and 5-frame batches of 64 x 32-ish sources into small windows, 8- and 10-bit context
output across both target formats, a caller's stream and a context that owns its stream (the batch lanes), a budget that forces more than
one chunk, the info string, and the refusals.  Everything is byte-for-byte equality."""
import ctypes as C

import numpy as np
import pytest

from tests import deband_model as DM
from tests.test_batch_tensor_gpu import LANES_OFF, ROUTES, context, noise_frames
from tests.test_deband import params
from tests.test_deband_gpu import pattern

pytestmark = pytest.mark.gpu

BGRA8, RGB10A2 = DM.BGRA8, DM.RGB10A2
# the routes of tests/test_batch_tensor_gpu.py: an exact 2x on the fused kernel into a 259 x 39 window with a letterbox (a lane route), a
# quarter turn through the pass-per-kernel path (the context stream) — with 8- and 10-bit context output
CASES = {
    "FusedUp2x-10bit": (dict(ROUTES["FusedUp2x"][0], output_format=1), ROUTES["FusedUp2x"][1], True),
    "FusedUp2x-8bit": (dict(ROUTES["FusedUp2x"][0], output_format=0), ROUTES["FusedUp2x"][1], True),
    "WholeBatchLaunches-10bit": (dict(ROUTES["WholeBatchLaunches"][0], output_format=1), ROUTES["WholeBatchLaunches"][1], False),
}
SEED = 0xfffffffe          # frame 2 of a batch takes seed 0: seed + i wraps mod 2^32


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(autouse=True)
def _no_override(monkeypatch):
    monkeypatch.delenv("MPCVR_DEBAND_TAPS", raising=False)


def words_of(t, wh, ww):
    return t.cpu().numpy().view(np.uint32).reshape(wh, ww)


def composition(torch, vp, frames, ww, wh, fmt, P, seed, dst_fmt):
    """what the header defines the targets by: mpcvr_process_batch into window-sized RGB targets (black: the letterbox is never written),
    then mpcvr_deband_pass per frame with seed + i.  -> (the targets as one (k, h, w, 4) uint8 tensor, the RGB frames as (h, w) uint32,
    the launches the batch took)"""
    from videorenderer_amd import api
    rgb = [torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda") for _ in frames]
    vp.ProcessBatch(frames, rgb, ww * 4)
    vp.Synchronize()
    launches = vp.GetLastBatchInfo()["launches"]
    want = torch.zeros((len(frames), wh, ww, 4), dtype=torch.uint8, device="cuda")
    for i, t in enumerate(rgb):
        api.deband_pass(t, ww * 4, fmt, ww, wh, P, (seed + i) & 0xffffffff, want[i], ww * 4, dst_fmt, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return want, [words_of(t, wh, ww) for t in rgb], launches


@pytest.mark.parametrize("own", [False, True], ids=["callers_stream", "own_stream"])
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("case", sorted(CASES))
def test_targets_equal_process_batch_then_the_pass_and_the_model(mpcvr, torch_cuda, case, k, own):
    from videorenderer_amd import api
    torch = torch_cuda
    c, fragment, lane_route = CASES[case]
    fmt = c["output_format"]
    with torch.cuda.stream(torch.cuda.Stream()):        # (torch's default stream is NULL = "the context's own stream")
        vp, ww, wh = context(c, own)
        frames = noise_frames(torch, c, k)
        torch.cuda.synchronize()
        on_lanes = own and lane_route and not LANES_OFF
        lay = api.plan_batch_deband(ww, wh, k, 0)
        for P, dst_fmt in ((params(16, 2, 4 * DM.MAXCODE[fmt], 1), BGRA8), (params(4, 3, 40, 0), RGB10A2)):
            taps = api.plan_deband(fmt, P, ww, wh)[1]
            want, rgb, plain = composition(torch, vp, frames, ww, wh, fmt, P, SEED, dst_fmt)
            assert fragment in vp.GetVPInfo(), (case, vp.GetVPInfo())
            # padded targets inside one patterned buffer: what lies between the rows and the frames survives
            pitch = 4 * ww + 16
            before = pattern(k * wh * pitch)
            for budget, chunks in ((2 * lay["frame_stride"], (k + 1) // 2), (0, 1)):
                vp.SetBatchYuvBudget(budget)
                assert api.plan_batch_deband(ww, wh, k, budget)["chunks"] == chunks
                buf = torch.from_numpy(before).cuda()
                torch.cuda.synchronize()
                vp.ProcessBatchDeband(frames, P, SEED, [buf.data_ptr() + i * wh * pitch for i in range(k)], pitch, dst_fmt)
                vp.Synchronize()
                got = vp.GetLastBatchInfo()
                assert got["frames"] == k and got["deband_chunks"] == chunks and got["deband_taps"] == taps, (case, got)
                assert "yuv_chunks" not in got and "tensor_chunks" not in got and "lut3d_chunks" not in got, got
                if chunks == 1:
                    assert got["launches"] == plain + 1, (got, plain)
                assert len(got["deband_lanes"]) == chunks and set(got["deband_lanes"]) <= {-1, 0, 1}, (case, got)
                if not on_lanes:
                    assert got["deband_lanes"] == [-1] * chunks, (case, own, got)
                elif k == 5 and chunks > 1:            # chunks of two frames go to the batch lanes (a chunk of one frame never does)
                    assert any(lane >= 0 for lane in got["deband_lanes"]), (case, got)
                full = before.copy()
                for i in range(k):
                    DM.place(full, i * wh * pitch, words_of(want[i], wh, ww), pitch)
                assert np.array_equal(buf.cpu().numpy(), full), (case, own, P, dst_fmt, "chunks", chunks, got)
            # ... and the model over the RGB frames read back, with the seed of each frame: the test does not rest on the library alone
            for i in range(k):
                model = DM.apply(rgb[i], fmt, dst_fmt, P["range"], P["iterations"], P["threshold"], P["dither"], (SEED + i) & 0xffffffff)
                assert np.array_equal(words_of(want[i], wh, ww), model), (case, "frame %d differs from the model" % i)
        vp.close()


def test_the_seed_of_a_frame_is_seed_plus_its_index(mpcvr, torch_cuda):
    """the same sample three times in a batch: three different dithered frames, frame i the one a pass with seed + i gives"""
    from videorenderer_amd import api
    torch = torch_cuda
    c = CASES["FusedUp2x-10bit"][0]
    vp, ww, wh = context(c, False)
    f = noise_frames(torch, c, 1)[0]
    P = params(16, 2, 16, 1)
    out = torch.zeros((3, wh, ww, 4), dtype=torch.uint8, device="cuda")
    vp.ProcessBatchDeband([f, f, f], P, 41, [out[i] for i in range(3)], ww * 4, BGRA8)
    vp.Synchronize()
    rgb = torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda")
    vp.ProcessBatch([f], [rgb], ww * 4)
    vp.Synchronize()
    for i in range(3):
        assert np.array_equal(words_of(out[i], wh, ww), DM.apply(words_of(rgb, wh, ww), RGB10A2, BGRA8, 16, 2, 16, 1, 41 + i)), i
    assert not torch.equal(out[0], out[1]) and not torch.equal(out[1], out[2])
    vp.close()


def test_refusals_write_nothing(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    c = CASES["FusedUp2x-8bit"][0]
    vp, ww, wh = context(c, False)
    k = 3
    frames = noise_frames(torch, c, k)
    base = torch.full((k + 1, wh, ww, 4), 9, dtype=torch.uint8, device="cuda")
    L = vp._L
    arr = C.c_void_p * k
    srcs, dsts = arr(*[f.data_ptr() for f in frames]), arr(*[base[i].data_ptr() for i in range(k)])
    ok, P, E = C.byref(api.DebandParams(16, 2, 4, 1)), api.E_POINTER, api.E_INVALIDARG
    f = L.mpcvr_process_batch_deband
    pitch = ww * 4
    assert f(vp._ctx, k, None, ok, 1, dsts, pitch, 0) == P
    assert f(vp._ctx, k, srcs, None, 1, dsts, pitch, 0) == P
    assert f(vp._ctx, k, srcs, ok, 1, None, pitch, 0) == P
    assert f(vp._ctx, k, srcs, ok, 1, arr(dsts[0], None, dsts[2]), pitch, 0) == P
    assert f(vp._ctx, k, arr(srcs[0], None, srcs[2]), ok, 1, dsts, pitch, 0) == P
    assert f(vp._ctx, 0, srcs, ok, 1, dsts, pitch, 0) == E
    for bad in ((0, 2, 4, 1), (65, 1, 4, 1), (16, 5, 4, 1), (33, 2, 4, 1), (16, 2, 4 * 255 + 1, 1), (16, 2, -1, 1), (16, 2, 4, 2)):
        assert f(vp._ctx, k, srcs, C.byref(api.DebandParams(*bad)), 1, dsts, pitch, 0) == E, bad
    assert f(vp._ctx, k, srcs, ok, 1, dsts, pitch, 2) == E
    assert f(vp._ctx, k, srcs, ok, 1, dsts, pitch - 4, 0) == E
    assert f(vp._ctx, k, srcs, ok, 1, dsts, pitch + 2, 0) == E
    assert f(vp._ctx, k, srcs, ok, 1, arr(dsts[0], dsts[1] + 2, dsts[2]), pitch, 0) == E
    assert f(vp._ctx, k, srcs, ok, 1, arr(dsts[0], dsts[0] + pitch, dsts[2]), pitch, 0) == E          # targets that overlap each other
    assert f(vp._ctx, k, srcs, ok, 1, arr(dsts[0], dsts[1], dsts[1]), pitch, 0) == E                   # one target given twice
    bare = api.VideoProcessor(api.default_settings())
    assert f(bare._ctx, k, srcs, ok, 1, dsts, pitch, 0) == api.E_NOT_VALID_STATE
    bare.close()
    assert "deband_chunks" not in vp.GetLastBatchInfo()
    vp.Synchronize()
    torch.cuda.synchronize()
    assert bool((base == 9).all()), "a refused call wrote"
    # ... and the arguments the refusals were derived from are accepted
    assert f(vp._ctx, k, srcs, ok, 1, dsts, pitch, 0) == 0
    vp.Synchronize()
    want, _, _ = composition(torch, vp, frames, ww, wh, 0, params(16, 2, 4, 1), 1, BGRA8)
    assert torch.equal(base[:k], want) and bool((base[k:] == 9).all())
    vp.close()
