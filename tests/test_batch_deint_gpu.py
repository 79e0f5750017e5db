"""mpcvr_process_batch_deint (extension: a batch at field rate, include/mpcvr.h) on the GPU: the targets equal, byte for byte, what
mpcvr_deint_pass into caller samples followed by mpcvr_process_batch leaves — NV12 and P010, both field orders, one and two fields per
frame, both modes, a same-size and a resize route, on a caller's stream and on a context that owns its stream, in one chunk and in three —
with deint_chunks and launches as planned, and the refusals drawing nothing."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import deint_model as M

pytestmark = pytest.mark.gpu

W, H, N = 64, 48, 4
NV12, P010, YUY2 = 1, 2, 4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(autouse=True)
def side_stream(torch_cuda):
    """the tests run on a stream torch made: a context on torch's stream is a context on a caller's stream"""
    with torch_cuda.cuda.stream(torch_cuda.cuda.Stream()):
        yield


def context(api, cformat, out, own_stream=False):
    vp = api.VideoProcessor(api.default_settings(iUpscaling=2), use_torch_stream=not own_stream)
    vp.InitMediaType(cformat, W, H)
    vp.SetWindowRect((0, 0, out[0], out[1]))
    vp.SetVideoRect((0, 0, out[0], out[1]))
    return vp


_frames = {}


def frames(torch, api, cformat):
    """N + 2 interlaced device samples, computed once per format and left unchanged"""
    if cformat not in _frames:
        host = M.noise_samples(api.plan_deint_planes(cformat, W, H), N + 2, 400 + cformat)
        _frames[cformat] = [torch.from_numpy(x).cuda() for x in host]
        torch.cuda.synchronize()
    return _frames[cformat]


def targets(torch, n, out):
    return [torch.zeros((out[1], out[0], 4), dtype=torch.uint8, device="cuda") for _ in range(n)]


def composition(api, torch, vp, fr, cformat, order, fpf, mode, out, cut):
    """n * fpf x mpcvr_deint_pass into caller samples, then mpcvr_process_batch — all at once for the pixels, and cut into runs of `cut`
    frames for the launches a call with such chunks is planned to take.  -> (the targets as arrays, launches of the cut batches, passes per sample)"""
    nbytes, pitch = vp.GetFrameBytes()
    n_out = N * fpf
    samples = [torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for _ in range(n_out)]
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(n_out):
        i = 1 + k // fpf
        keep, first = M.field_parity(order, k % fpf)
        api.deint_pass(fr[i - 1], fr[i], fr[i + 1], cformat, W, H, pitch, keep, first, mode, samples[k], pitch, stream)
    torch.cuda.synchronize()
    dsts = targets(torch, n_out, out)
    torch.cuda.synchronize()
    vp.ProcessBatch(samples, dsts, out[0] * 4)
    vp.Synchronize()
    launches = 0
    for at in range(0, n_out, cut):
        part = samples[at:at + cut]
        scratch = targets(torch, len(part), out)
        torch.cuda.synchronize()
        vp.ProcessBatch(part, scratch, out[0] * 4)
        launches += vp.GetLastBatchInfo()["launches"]
    vp.Synchronize()
    return [d.cpu().numpy() for d in dsts], launches


@pytest.mark.parametrize("own_stream", [False, True], ids=["caller-stream", "own-stream"])
@pytest.mark.parametrize("out", [(W, H), (96, 72)], ids=["same-size", "resize"])
@pytest.mark.parametrize("cformat", [NV12, P010], ids=["nv12", "p010"])
def test_batch_equals_deint_passes_then_process_batch(mpcvr, torch_cuda, cformat, out, own_stream):
    from videorenderer_amd import api
    torch = torch_cuda
    fr = frames(torch, api, cformat)
    vp = context(api, cformat, out, own_stream)
    nbytes, pitch = vp.GetFrameBytes()
    lines = nbytes // pitch
    passes = 2                                          # bi-planar: one k_deint launch for the Y plane, one for the UV plane
    for order, fpf, mode in itertools.product((1, 2), (1, 2), (0, 1)):
        n_out = N * fpf
        stride = (pitch * lines + 255) // 256 * 256
        # one chunk (the default budget), then a budget of three frames and a half: three chunks for the eight pictures at field rate (3 + 3 + 2),
        # two for the four at frame rate (3 + 1)
        for budget, per in ((0, n_out), (3 * stride + stride // 2, 3)):
            chunks = -(-n_out // per)
            assert budget == 0 or chunks == (3 if fpf == 2 else 2)
            assert api.plan_batch_deint(pitch, lines, n_out, budget) == dict(frame_stride=stride, frames_per_chunk=per, chunks=chunks)
            want, planned = composition(api, torch, vp, fr, cformat, order, fpf, mode, out, per)
            vp.SetBatchYuvBudget(budget)
            dsts = targets(torch, n_out, out)
            torch.cuda.synchronize()
            vp.ProcessBatchDeint(fr, dsts, out[0] * 4, order, fpf, mode)
            vp.Synchronize()
            info = vp.GetLastBatchInfo()
            assert info["frames"] == n_out and info["deint_chunks"] == chunks and info["launches"] == planned + passes * chunks, (info, planned, chunks)
            assert "sample_chunks" not in info and "yuv_chunks" not in info
            for k in range(n_out):
                assert want[k].any() and np.array_equal(dsts[k].cpu().numpy(), want[k]), (order, fpf, mode, budget, k)
        if fpf == 2:      # the two fields of a frame are two different pictures
            assert not np.array_equal(want[0], want[1])
    vp.close()


def test_refusals_draw_nothing(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    fr = frames(torch, api, NV12)
    out = (W, H)
    dsts = targets(torch, 2 * N, out)
    torch.cuda.synchronize()
    fa, da = C.c_void_p * (N + 2), C.c_void_p * (2 * N)
    fp, dp = fa(*[x.data_ptr() for x in fr]), da(*[x.data_ptr() for x in dsts])
    pitch = W * 4

    def call(vp, n=N, fp=fp, order=1, fpf=2, mode=0, dp=dp, pitch=pitch):
        return L.mpcvr_process_batch_deint(vp._ctx, n, fp, order, fpf, mode, dp, pitch)

    vp = api.VideoProcessor(api.default_settings())
    assert call(vp) == api.E_NOT_VALID_STATE
    vp.InitMediaType(YUY2, W, H)
    assert call(vp) == api.E_INVALIDARG                 # a packed input
    vp.close()
    vp = context(api, NV12, out)
    holes_f = fa(*[x.data_ptr() for x in fr]); holes_f[N + 1] = None
    holes_d = da(*[x.data_ptr() for x in dsts]); holes_d[2 * N - 1] = None
    odd_d = da(*[x.data_ptr() for x in dsts]); odd_d[1] = dsts[1].data_ptr() + 2
    for kw, hr in ((dict(n=0), api.E_INVALIDARG), (dict(n=-1), api.E_INVALIDARG), (dict(fp=None), api.E_POINTER), (dict(dp=None), api.E_POINTER),
                   (dict(fp=holes_f), api.E_POINTER), (dict(dp=holes_d), api.E_POINTER),
                   (dict(fpf=0), api.E_INVALIDARG), (dict(fpf=3), api.E_INVALIDARG), (dict(order=0), api.E_INVALIDARG), (dict(order=3), api.E_INVALIDARG),
                   (dict(mode=2), api.E_INVALIDARG), (dict(mode=-1), api.E_INVALIDARG),
                   (dict(pitch=pitch - 4), api.E_INVALIDARG), (dict(dp=odd_d), api.E_INVALIDARG)):
        assert call(vp, **kw) == hr, kw
        info = vp.GetLastBatchInfo()
        assert info["launches"] == 0 and "deint_chunks" not in info
    torch.cuda.synchronize()
    assert not any(bool(x.any()) for x in dsts)
    assert call(vp) == 0
    vp.Synchronize()
    assert all(bool(x.any()) for x in dsts) and vp.GetLastBatchInfo()["deint_chunks"] == 1
    vp.close()
    # a 16-bit input: a sample off the component grid
    vp = context(api, P010, out)
    f16 = frames(torch, api, P010)
    off = fa(*[x.data_ptr() for x in f16]); off[2] = f16[2].data_ptr() + 1
    before = [x.clone() for x in dsts]
    assert call(vp, fp=off) == api.E_INVALIDARG
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(dsts, before))
    vp.close()


def test_error_diffusion_behind_the_deint_chunks(mpcvr, torch_cuda):
    """bUseDither = 2: each chunk's samples go through the error-diffusion plan's own chunks and its pass instead of a batch route.  Two
    interior 16 x 8 P010 frames at field rate (four pictures) into 32 x 16 windows, in one chunk and in two chunks of two; each target
    equals, byte for byte, the deinterlacing passes followed by mpcvr_process_batch with the same settings."""
    from videorenderer_amd import api
    torch = torch_cuda
    w, h, n, fpf, order, mode, cformat = 16, 8, 2, 2, 1, 0, P010
    n_out = n * fpf
    fr = [torch.from_numpy(x).cuda() for x in M.noise_samples(api.plan_deint_planes(cformat, w, h), n + 2, 77)]
    vp = api.VideoProcessor(api.default_settings(iUpscaling=4, bUseDither=2))
    vp.InitMediaType(cformat, w, h)
    vp.SetWindowRect((0, 0, 2 * w, 2 * h))
    vp.SetVideoRect((0, 0, 2 * w, 2 * h))
    assert "errdiff" in vp.GetVPInfo()
    nbytes, pitch = vp.GetFrameBytes()
    lines = nbytes // pitch
    samples = [torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for _ in range(n_out)]
    for k in range(n_out):
        i = 1 + k // fpf
        keep, first = M.field_parity(order, k % fpf)
        api.deint_pass(fr[i - 1], fr[i], fr[i + 1], cformat, w, h, pitch, keep, first, mode, samples[k], pitch, torch.cuda.current_stream().cuda_stream)
    dsts = targets(torch, n_out, (2 * w, 2 * h))
    torch.cuda.synchronize()
    vp.ProcessBatch(samples, dsts, 2 * w * 4)
    vp.Synchronize()
    want = [x.cpu().numpy() for x in dsts]
    assert not np.array_equal(want[0], want[1])
    stride = api.plan_batch_deint(pitch, lines, n_out, 0)["frame_stride"]
    for budget, per, chunks in ((0, n_out, 1), (2 * stride + stride // 2, 2, 2)):
        assert api.plan_batch_deint(pitch, lines, n_out, budget) == dict(frame_stride=stride, frames_per_chunk=per, chunks=chunks)
        vp.SetBatchYuvBudget(budget)
        dsts = targets(torch, n_out, (2 * w, 2 * h))
        torch.cuda.synchronize()
        vp.ProcessBatchDeint(fr, dsts, 2 * w * 4, order, fpf, mode)
        vp.Synchronize()
        assert vp.GetLastBatchInfo()["deint_chunks"] == chunks
        for k in range(n_out):
            assert want[k].any() and np.array_equal(dsts[k].cpu().numpy(), want[k]), (budget, k)
    vp.close()
