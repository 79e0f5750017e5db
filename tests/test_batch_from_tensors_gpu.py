"""mpcvr_process_batch_from_tensors on the GPU (extension: a batch whose samples are a model's float tensors, include/mpcvr.h): the render
targets against the composition the header defines them by — mpcvr_sample_pass per frame into samples of the caller's, then
mpcvr_process_batch — on one chunk and on forced chunks of two frames, mpcvr_get_last_batch_info, the reuse of the sample surface by two
calls back to back, and the refusals.  Everything is byte-for-byte equality."""
import ctypes as C

import numpy as np
import pytest

from tests import tensor_in_cases as K
from tests import tensor_in_model as M

pytestmark = pytest.mark.gpu

W, H = 32, 16


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(autouse=True)
def side_stream(torch_cuda):
    """torch's default stream is NULL, which a context takes as "make a stream of your own": the tests run on a stream torch made, so a
    context on torch's stream is a context on a caller's stream and everything queued is ordered on it"""
    with torch_cuda.cuda.stream(torch_cuda.cuda.Stream()):
        yield


def context(api, cformat, scale2=2, flags=0):
    vp = api.VideoProcessor(api.default_settings(iUpscaling=2, flags=flags))
    vp.InitMediaType(cformat, W, H)
    vp.SetWindowRect((0, 0, W * scale2, H * scale2))
    vp.SetVideoRect((0, 0, W * scale2, H * scale2))
    return vp


def pictures(torch, seed, n, dtype, layout):
    """n float pictures in [-0.1, 1.1]: (n, 3, H, W) or (n, H, W, 3)"""
    a = np.random.default_rng(seed).random((n, 3, H, W), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    t = torch.from_numpy(a if layout == "chw" else np.ascontiguousarray(a.transpose(0, 2, 3, 1))).cuda()
    return t.to(dtype)


def targets(torch, n, scale2):
    return [torch.zeros((H * scale2, W * scale2, 4), dtype=torch.uint8, device="cuda") for _ in range(n)]


def composition(api, torch, vp, ts, cformat, scale, bias, order, scale2, cut):
    """n x mpcvr_sample_pass into n caller samples, then mpcvr_process_batch — all n at once for the pixels, and cut into runs of `cut`
    frames for the launches a call with such chunks is planned to take.  -> (the targets as arrays, launches of the cut batches)"""
    n = len(ts)
    nbytes, pitch = vp.GetFrameBytes()
    samples = [torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for _ in range(n)]
    stream = torch.cuda.current_stream().cuda_stream
    for i in range(n):
        d, w, h = api._frame_tensor_desc(ts[i], scale, bias, order)
        assert (w, h) == (W, H)
        api.sample_pass(ts[i], d, W, H, cformat, samples[i], pitch, stream)
    dsts = targets(torch, n, scale2)
    vp.ProcessBatch(samples, dsts, W * scale2 * 4)
    vp.Synchronize()
    launches = 0
    for at in range(0, n, cut):
        part = samples[at:at + cut]
        vp.ProcessBatch(part, targets(torch, len(part), scale2), W * scale2 * 4)
        launches += vp.GetLastBatchInfo()["launches"]
    vp.Synchronize()
    return [d.cpu().numpy() for d in dsts], launches


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("cformat,dtype,layout,order", [(M.GBRP16, "float16", "chw", "rgb"), (M.GBRP8, "float32", "hwc", "bgr"), (M.GBRP10, "bfloat16", "chw", "bgr")],
                         ids=["gbrp16-f16-chw", "gbrp8-f32-hwc-bgr", "gbrp10-bf16-chw-bgr"])
def test_batch_equals_sample_passes_then_process_batch(mpcvr, torch_cuda, cformat, dtype, layout, order, n):
    from videorenderer_amd import api
    torch = torch_cuda
    scale, bias = K.identity_factors(cformat)
    ts = pictures(torch, 100 + n, n, getattr(torch, dtype), layout)
    for scale2, flags in ((2, 0), (1, 0), (2, api.FLAG_NO_FUSED)):
        vp = context(api, cformat, scale2, flags)
        stride = api.plan_batch_from_tensors(vp.GetFrameBytes()[1], H, n, 0)["frame_stride"]
        assert stride == (3 * vp.GetFrameBytes()[1] * H + 255) // 256 * 256
        # one chunk (the default budget), then chunks of two frames
        for budget, per in ((0, n), (2 * stride + stride // 2, min(2, n))):
            want, planned = composition(api, torch, vp, ts, cformat, scale, bias, order, scale2, per)
            chunks = -(-n // per)
            assert api.plan_batch_from_tensors(vp.GetFrameBytes()[1], H, n, budget) == dict(frame_stride=stride, frames_per_chunk=per, chunks=chunks)
            vp.SetBatchYuvBudget(budget)
            dsts = targets(torch, n, scale2)
            vp.ProcessBatchFromTensors(ts, dsts, W * scale2 * 4, scale, bias, order)
            vp.Synchronize()
            info = vp.GetLastBatchInfo()
            assert info["frames"] == n and info["sample_chunks"] == chunks and info["launches"] == planned + chunks, (info, planned, chunks)
            assert "tensor_chunks" not in info and "yuv_chunks" not in info
            for i in range(n):
                assert want[i].any() and np.array_equal(dsts[i].cpu().numpy(), want[i]), (scale2, flags, budget, i)
        vp.close()


def test_two_calls_back_to_back_reuse_the_surface_in_order(mpcvr, torch_cuda):
    """different tensors, no synchronize between the calls, chunks of two: the second call's passes overwrite the surface the first call's
    batches read — stream order must keep them apart"""
    from videorenderer_amd import api
    torch = torch_cuda
    cformat, n = M.GBRP16, 5
    scale, bias = K.identity_factors(cformat)
    a, b = pictures(torch, 1, n, torch.float16, "chw"), pictures(torch, 2, n, torch.float16, "chw")
    vp = context(api, cformat)
    want_a, _ = composition(api, torch, vp, a, cformat, scale, bias, "rgb", 2, n)
    want_b, _ = composition(api, torch, vp, b, cformat, scale, bias, "rgb", 2, n)
    assert not np.array_equal(want_a[0], want_b[0])
    stride = api.plan_batch_from_tensors(vp.GetFrameBytes()[1], H, n, 0)["frame_stride"]
    vp.SetBatchYuvBudget(2 * stride)
    da, db = targets(torch, n, 2), targets(torch, n, 2)
    vp.ProcessBatchFromTensors(a, da, W * 2 * 4, scale, bias)
    vp.ProcessBatchFromTensors(b, db, W * 2 * 4, scale, bias)
    vp.Synchronize()
    for i in range(n):
        assert np.array_equal(da[i].cpu().numpy(), want_a[i]) and np.array_equal(db[i].cpu().numpy(), want_b[i]), i
    vp.close()


def test_refusals_draw_nothing(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    n = 2
    ts = pictures(torch, 5, n, torch.float16, "chw")
    d, _, _ = api._frame_tensor_desc(ts[0], (255.0,) * 3, (0.0,) * 3, "rgb")
    dsts = targets(torch, n, 2)
    arr = C.c_void_p * n
    tp, dp = arr(*[t.data_ptr() for t in ts]), arr(*[x.data_ptr() for x in dsts])
    pitch = W * 2 * 4

    def call(vp, n=n, tp=tp, desc=d, dp=dp, pitch=pitch):
        return L.mpcvr_process_batch_from_tensors(vp._ctx, n, tp, C.byref(desc) if desc is not None else None, dp, pitch)

    vp = api.VideoProcessor(api.default_settings())
    assert call(vp) == api.E_NOT_VALID_STATE
    vp.InitMediaType(1, W, H)
    assert call(vp) == api.E_INVALIDARG                 # not a planar RGB input
    vp.close()
    vp = context(api, M.GBRP8)
    bad = api.tensor_desc(M.F16, M.PLANAR, d.row_pitch, d.plane_pitch, (255.0, float("nan"), 255.0), (0.0,) * 3)
    odd = api.tensor_desc(M.F16, M.PLANAR, d.row_pitch + 1, d.plane_pitch, (255.0,) * 3, (0.0,) * 3)
    for kw, hr in ((dict(n=0), api.E_INVALIDARG), (dict(n=-1), api.E_INVALIDARG), (dict(tp=None), api.E_POINTER), (dict(dp=None), api.E_POINTER), (dict(desc=None), api.E_POINTER),
                   (dict(tp=arr(ts[0].data_ptr(), None)), api.E_POINTER), (dict(dp=arr(dsts[0].data_ptr(), None)), api.E_POINTER),
                   (dict(desc=bad), api.E_INVALIDARG), (dict(desc=odd), api.E_INVALIDARG), (dict(tp=arr(ts[0].data_ptr(), ts[1].data_ptr() + 1)), api.E_INVALIDARG),
                   (dict(pitch=pitch - 4), api.E_INVALIDARG), (dict(dp=arr(dsts[0].data_ptr(), dsts[1].data_ptr() + 2)), api.E_INVALIDARG)):
        assert call(vp, **kw) == hr, kw
        info = vp.GetLastBatchInfo()
        assert info["launches"] == 0 and "sample_chunks" not in info
    torch.cuda.synchronize()
    assert not any(bool(x.any()) for x in dsts)
    assert call(vp) == 0
    vp.Synchronize()
    assert all(bool(x.any()) for x in dsts) and vp.GetLastBatchInfo()["sample_chunks"] == 1
    vp.close()


def test_error_diffusion_behind_the_sample_chunks(mpcvr, torch_cuda):
    """bUseDither = 2: each chunk's samples go through the error-diffusion plan's own chunks and its pass instead of a batch route.  Four
    16 x 8 GBRP16 frames into 32 x 16 windows, in one chunk and in two chunks of two; each target equals, byte for byte, the sample passes
    followed by mpcvr_process_batch with the same settings."""
    from videorenderer_amd import api
    torch = torch_cuda
    w, h, n, cformat = 16, 8, 4, M.GBRP16
    scale, bias = K.identity_factors(cformat)
    a = np.random.default_rng(31).random((n, 3, h, w), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    ts = torch.from_numpy(a).cuda().to(torch.float16)
    vp = api.VideoProcessor(api.default_settings(iUpscaling=4, bUseDither=2))
    vp.InitMediaType(cformat, w, h)
    vp.SetWindowRect((0, 0, 2 * w, 2 * h))
    vp.SetVideoRect((0, 0, 2 * w, 2 * h))
    assert "errdiff" in vp.GetVPInfo()
    nbytes, pitch = vp.GetFrameBytes()
    samples = [torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for _ in range(n)]
    for i in range(n):
        d, _, _ = api._frame_tensor_desc(ts[i], scale, bias, "rgb")
        api.sample_pass(ts[i], d, w, h, cformat, samples[i], pitch, torch.cuda.current_stream().cuda_stream)
    new = lambda: [torch.zeros((2 * h, 2 * w, 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    dsts = new()
    vp.ProcessBatch(samples, dsts, 2 * w * 4)
    vp.Synchronize()
    want = [x.cpu().numpy() for x in dsts]
    assert not np.array_equal(want[0], want[1])
    stride = api.plan_batch_from_tensors(pitch, h, n, 0)["frame_stride"]
    for budget, per, chunks in ((0, n, 1), (2 * stride + stride // 2, 2, 2)):
        assert api.plan_batch_from_tensors(pitch, h, n, budget) == dict(frame_stride=stride, frames_per_chunk=per, chunks=chunks)
        vp.SetBatchYuvBudget(budget)
        dsts = new()
        vp.ProcessBatchFromTensors(ts, dsts, 2 * w * 4, scale, bias)
        vp.Synchronize()
        assert vp.GetLastBatchInfo()["sample_chunks"] == chunks
        for i in range(n):
            assert want[i].any() and np.array_equal(dsts[i].cpu().numpy(), want[i]), (budget, i)
    vp.close()
