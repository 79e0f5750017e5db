"""mpcvr_process_batch_sharpen on the GPU (extension: sharpening of rendered frames, include/mpcvr.h): the targets against the composition
the header defines them by — mpcvr_process_batch into window-sized RGB targets, then mpcvr_sharpen_pass per frame with seed + i — and
against the numpy model over those targets: 3- and 5-frame batches of 64 x 32-ish sources into small windows, 8- and 10-bit context
output across both target formats, a caller's stream and a context that owns its stream (the batch lanes), a budget that forces more than
one chunk, a seed that wraps, the launch count, the info string, and the refusals.  Everything is byte-for-byte equality."""
import ctypes as C

import numpy as np
import pytest

from tests import sharpen_model as SM
from tests.test_batch_deband_gpu import CASES, SEED, words_of
from tests.test_batch_tensor_gpu import LANES_OFF, context, noise_frames
from tests.test_deband_gpu import pattern
from tests.test_sharpen import model, params

pytestmark = pytest.mark.gpu

BGRA8, RGB10A2 = SM.BGRA8, SM.RGB10A2
assert SEED == 0xfffffffe          # frame 2 of a batch takes seed 0: seed + i wraps mod 2^32


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def composition(torch, vp, frames, ww, wh, fmt, P, seed, dst_fmt):
    """what the header defines the targets by: mpcvr_process_batch into window-sized RGB targets (black: the letterbox is never written),
    then mpcvr_sharpen_pass per frame with seed + i.  -> (the targets as one (k, h, w, 4) uint8 tensor, the RGB frames as (h, w) uint32,
    the launches the batch took)"""
    from videorenderer_amd import api
    rgb = [torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda") for _ in frames]
    vp.ProcessBatch(frames, rgb, ww * 4)
    vp.Synchronize()
    launches = vp.GetLastBatchInfo()["launches"]
    want = torch.zeros((len(frames), wh, ww, 4), dtype=torch.uint8, device="cuda")
    for i, t in enumerate(rgb):
        api.sharpen_pass(t, ww * 4, fmt, ww, wh, P, (seed + i) & 0xffffffff, want[i], ww * 4, dst_fmt, stream=torch.cuda.current_stream().cuda_stream)
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
    m = SM.MAXCODE[fmt]
    with torch.cuda.stream(torch.cuda.Stream()):        # (torch's default stream is NULL = "the context's own stream")
        vp, ww, wh = context(c, own)
        frames = noise_frames(torch, c, k)
        torch.cuda.synchronize()
        on_lanes = own and lane_route and not LANES_OFF
        lay = api.plan_batch_sharpen(ww, wh, k, 0)
        for P, dst_fmt in ((params(2, 64, m // 8, m // 16, 1, 1), BGRA8), (params(3, 200, m // 4, 1, 0, 0), RGB10A2)):
            want, rgb, plain = composition(torch, vp, frames, ww, wh, fmt, P, SEED, dst_fmt)
            assert fragment in vp.GetVPInfo(), (case, vp.GetVPInfo())
            # padded targets inside one patterned buffer: what lies between the rows and the frames survives
            pitch = 4 * ww + 16
            before = pattern(k * wh * pitch)
            for budget, chunks in ((2 * lay["frame_stride"], (k + 1) // 2), (0, 1)):
                vp.SetBatchYuvBudget(budget)
                assert api.plan_batch_sharpen(ww, wh, k, budget)["chunks"] == chunks
                buf = torch.from_numpy(before).cuda()
                torch.cuda.synchronize()
                vp.ProcessBatchSharpen(frames, P, SEED, [buf.data_ptr() + i * wh * pitch for i in range(k)], pitch, dst_fmt)
                vp.Synchronize()
                got = vp.GetLastBatchInfo()
                assert got["frames"] == k and got["sharpen_chunks"] == chunks, (case, got)
                assert "yuv_chunks" not in got and "tensor_chunks" not in got and "lut3d_chunks" not in got and "deband_chunks" not in got, got
                if chunks == 1:                         # the composition's plain + k launches minus (k - chunks): its k passes are one
                    assert got["launches"] == (plain + k) - (k - chunks), (got, plain)
                assert len(got["sharpen_lanes"]) == chunks and set(got["sharpen_lanes"]) <= {-1, 0, 1}, (case, got)
                if not on_lanes:
                    assert got["sharpen_lanes"] == [-1] * chunks, (case, own, got)
                elif k == 5 and chunks > 1:            # chunks of two frames go to the batch lanes (a chunk of one frame never does)
                    assert any(lane >= 0 for lane in got["sharpen_lanes"]), (case, got)
                full = before.copy()
                for i in range(k):
                    SM.place(full, i * wh * pitch, words_of(want[i], wh, ww), pitch)
                assert np.array_equal(buf.cpu().numpy(), full), (case, own, P, dst_fmt, "chunks", chunks, got)
            # ... and the model over the RGB frames read back, with the seed of each frame: the test does not rest on the library alone.
            # The rendered noise takes every branch of the definition at these parameters
            total = dict.fromkeys(SM.BRANCHES, 0)
            for i in range(k):
                counts = {}
                assert np.array_equal(words_of(want[i], wh, ww), model(rgb[i], fmt, dst_fmt, P, (SEED + i) & 0xffffffff, counts)), (case, "frame %d differs from the model" % i)
                for b in SM.BRANCHES:
                    total[b] += counts[b]
            assert all(total[b] > 0 for b in SM.BRANCHES), (case, P, total)
        vp.close()


def test_the_seed_of_a_frame_is_seed_plus_its_index(mpcvr, torch_cuda):
    """the same sample three times in a batch: three different dithered frames, frame i the one a pass with seed + i gives"""
    torch = torch_cuda
    c = CASES["FusedUp2x-10bit"][0]
    vp, ww, wh = context(c, False)
    f = noise_frames(torch, c, 1)[0]
    P = params(2, 32, 16, 8, 1, 1)
    out = torch.zeros((3, wh, ww, 4), dtype=torch.uint8, device="cuda")
    vp.ProcessBatchSharpen([f, f, f], P, 41, [out[i] for i in range(3)], ww * 4, BGRA8)
    vp.Synchronize()
    rgb = torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda")
    vp.ProcessBatch([f], [rgb], ww * 4)
    vp.Synchronize()
    for i in range(3):
        assert np.array_equal(words_of(out[i], wh, ww), model(words_of(rgb, wh, ww), RGB10A2, BGRA8, P, 41 + i)), i
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
    ok, P, E = C.byref(api.SharpenParams(2, 32, 4, 2, 1, 1)), api.E_POINTER, api.E_INVALIDARG
    f = L.mpcvr_process_batch_sharpen
    pitch = ww * 4
    assert f(vp._ctx, k, None, ok, 1, dsts, pitch, 0) == P
    assert f(vp._ctx, k, srcs, None, 1, dsts, pitch, 0) == P
    assert f(vp._ctx, k, srcs, ok, 1, None, pitch, 0) == P
    assert f(vp._ctx, k, srcs, ok, 1, arr(dsts[0], None, dsts[2]), pitch, 0) == P
    assert f(vp._ctx, k, arr(srcs[0], None, srcs[2]), ok, 1, dsts, pitch, 0) == P
    assert f(vp._ctx, 0, srcs, ok, 1, dsts, pitch, 0) == E
    for bad in ((0, 32, 4, 2, 1, 1), (4, 32, 4, 2, 1, 1), (2, 257, 4, 2, 1, 1), (2, -1, 4, 2, 1, 1), (2, 32, 4 * 255 + 1, 2, 1, 1), (2, 32, -1, 2, 1, 1),
                (2, 32, 4, 256, 1, 1), (2, 32, 4, -1, 1, 1), (2, 32, 4, 2, 2, 1), (2, 32, 4, 2, 1, 2)):
        assert f(vp._ctx, k, srcs, C.byref(api.SharpenParams(*bad)), 1, dsts, pitch, 0) == E, bad
    assert f(vp._ctx, k, srcs, ok, 1, dsts, pitch, 2) == E
    assert f(vp._ctx, k, srcs, ok, 1, dsts, pitch - 4, 0) == E
    assert f(vp._ctx, k, srcs, ok, 1, dsts, pitch + 2, 0) == E
    assert f(vp._ctx, k, srcs, ok, 1, arr(dsts[0], dsts[1] + 2, dsts[2]), pitch, 0) == E
    assert f(vp._ctx, k, srcs, ok, 1, arr(dsts[0], dsts[0] + pitch, dsts[2]), pitch, 0) == E          # targets that overlap each other
    assert f(vp._ctx, k, srcs, ok, 1, arr(dsts[0], dsts[1], dsts[1]), pitch, 0) == E                   # one target given twice
    bare = api.VideoProcessor(api.default_settings())
    assert f(bare._ctx, k, srcs, ok, 1, dsts, pitch, 0) == api.E_NOT_VALID_STATE
    bare.close()
    assert "sharpen_chunks" not in vp.GetLastBatchInfo()
    vp.Synchronize()
    torch.cuda.synchronize()
    assert bool((base == 9).all()), "a refused call wrote"
    # ... and the arguments the refusals were derived from are accepted
    assert f(vp._ctx, k, srcs, ok, 1, dsts, pitch, 0) == 0
    vp.Synchronize()
    want, _, _ = composition(torch, vp, frames, ww, wh, 0, params(2, 32, 4, 2, 1, 1), 1, BGRA8)
    assert torch.equal(base[:k], want) and bool((base[k:] == 9).all())
    vp.close()
