"""mpcvr_process_batch_tensor on the GPU (extension: a batch written as float tensors, include/mpcvr.h): the tensors against the composition
the header defines them by — mpcvr_process_batch into window-sized RGB targets, then mpcvr_tensor_pass per frame — and against the numpy
model over those targets, for a lane route and a route that stays on the context stream, on a caller's stream and on a context that owns
its stream; the shapes of `out` VideoProcessor.ProcessBatchTensor accepts, mpcvr_get_last_batch_info, queue order and the refusals.
Everything is byte-for-byte equality."""
import os

import numpy as np
import pytest

from tests import tensor_model as TM
from tests.golden.cases import GOLDEN_CASES, HDR10, SETTING_KEYS, case_frame, case_geometry
from tests.test_tensor_gpu import BIAS, SCALE, bits_of

pytestmark = pytest.mark.gpu

# (case, GetVPInfo fragment, does the route take the batch lanes).  Windows of odd size: the tensor call has no evenness condition.
ROUTES = {
    # exact 2x, 128 x 18 -> 256 x 36 at (1, 1) of a 259 x 39 window: a tail lane in a second wavefront piece, and a letterbox
    "FusedUp2x": (dict(cformat=2, w=128, h=18, kind="noise", seed=911, dst=(256, 36), window=(259, 39), offset=(1, 1), exfmt=HDR10, iUpscaling=4), "fused_up2x", True),
    # a quarter turn into a 10-bit target: the whole-batch launches of the pass-per-kernel path, 48 x 40, on the context stream
    "WholeBatchLaunches": (dict(GOLDEN_CASES["rot90_two_pass_down_up"], output_format=1), "rot90", False),
}
# the even-windowed twin of the lane route, for the call beside ProcessBatchYuv
EVEN = dict(ROUTES["FusedUp2x"][0], window=(258, 38))
LANES_OFF = os.environ.get("MPCVR_NO_BATCH_LANES") == "1"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def noise_frames(torch, c, n, seed0=0):
    c = dict(c, kind="noise")
    return [torch.from_numpy(case_frame(dict(c, seed=c["seed"] + seed0 + 100 * i))[0]).cuda() for i in range(n)]


def context(c, own):
    """a context for the case: on torch's current stream, or (own) on a stream of its own, where batches may take the lanes"""
    from videorenderer_amd import api
    kw = {k: c[k] for k in SETTING_KEYS if k in c}
    vp = api.VideoProcessor(api.default_settings(**kw), use_torch_stream=not own)
    (ww, wh), vr = case_geometry(c)
    vp.InitMediaType(c["cformat"], c["w"], c["h"], extfmt=c.get("exfmt", 0))
    vp.SetWindowRect((0, 0, ww, wh))
    vp.SetVideoRect(vr)
    if "rotation" in c:
        vp.SetRotation(c["rotation"])
    return vp, ww, wh


def composition(torch, vp, frames, ww, wh, fmt, dtype, layout, order):
    """what the header defines the tensors by: mpcvr_process_batch into window-sized RGB targets (black: the letterbox is never written),
    then mpcvr_tensor_pass per frame into a dense tensor.  -> (the tensors as one (n, ...) tensor, the RGB targets as (h, w) uint32, the
    launches the batch took)"""
    from videorenderer_amd import api
    n = len(frames)
    rgb = [torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda") for _ in frames]
    vp.ProcessBatch(frames, rgb, ww * 4)
    vp.Synchronize()
    launches = vp.GetLastBatchInfo()["launches"]
    want = torch.zeros((n, 3, wh, ww) if layout == "chw" else (n, wh, ww, 3), dtype=dtype, device="cuda")
    es = want.element_size()
    d = api.tensor_desc(api._tensor_dtype(dtype), TM.PLANAR if layout == "chw" else TM.INTERLEAVED, es * ww * (1 if layout == "chw" else 3), es * ww * wh, SCALE, BIAS,
                        api._tensor_order(order))
    for i, t in enumerate(rgb):         # (on the stream `want` was cleared on)
        api.tensor_pass(t, ww * 4, fmt, ww, wh, d, want[i], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return want, [t.cpu().numpy().view(np.uint32).reshape(wh, ww) for t in rgb], launches


def same_bytes(torch, a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("own", [False, True], ids=["callers_stream", "own_stream"])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_tensors_equal_process_batch_then_tensor_pass_and_the_model(mpcvr, torch_cuda, route, own):
    from videorenderer_amd import api
    torch = torch_cuda
    c, fragment, lane_route = ROUTES[route]
    fmt = c.get("output_format", 0)
    n = 8               # chunks of 3, 3 and 2: unequal, and none of a single frame (which no route puts on a lane)
    with torch.cuda.stream(torch.cuda.Stream()):        # (torch's default stream is NULL = "the context's own stream")
        vp, ww, wh = context(c, own)
        frames = noise_frames(torch, c, n)
        torch.cuda.synchronize()
        on_lanes = own and lane_route and not LANES_OFF
        # out as a contiguous (N, 3, H, W) tensor, as (N, H, W, 3), and as a strided slice of a larger tensor
        big = torch.full((n + 1, 3, wh + 2, ww + 3), -2.0, dtype=torch.float32, device="cuda")
        outs = (("chw", "rgb", torch.full((n, 3, wh, ww), -2.0, dtype=torch.float16, device="cuda")),
                ("hwc", "bgr", torch.full((n, wh, ww, 3), -2.0, dtype=torch.bfloat16, device="cuda")),
                ("chw", "bgr", big[1:, :, 1:wh + 1, 2:ww + 2]))
        lay = api.plan_batch_tensor(ww, wh, n, 0)
        for layout, order, out in outs:
            want, rgb, plain = composition(torch, vp, frames, ww, wh, fmt, out.dtype, layout, order)
            assert fragment in vp.GetVPInfo(), (route, vp.GetVPInfo())
            # the launches the composition's batches take when cut as the chunks are
            cut = 0
            for at in (0, 3, 6):
                part = frames[at:at + 3]
                vp.ProcessBatch(part, [torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda") for _ in part], ww * 4)
                cut += vp.GetLastBatchInfo()["launches"]
            vp.Synchronize()
            for budget, chunks, launches in ((3 * lay["frame_stride"], 3, cut + 3), (0, 1, plain + 1)):
                vp.SetBatchYuvBudget(budget)
                assert api.plan_batch_tensor(ww, wh, n, budget)["chunks"] == chunks
                out.fill_(-2.0)
                torch.cuda.synchronize()
                vp.ProcessBatchTensor(frames, out, SCALE, BIAS, order)
                vp.Synchronize()
                got = vp.GetLastBatchInfo()
                assert got["frames"] == n and got["tensor_chunks"] == chunks and got["launches"] == launches and "yuv_chunks" not in got, (route, got)
                if on_lanes:            # the chunks take turns on the two batch lanes
                    lanes = set(got["tensor_lanes"])
                    assert len(got["tensor_lanes"]) == chunks and lanes <= {0, 1} and (chunks == 1 or lanes == {0, 1}), (route, got)
                else:
                    assert got["tensor_lanes"] == [-1] * chunks, (route, own, got)
                assert same_bytes(torch, out, want), (route, own, layout, order, out.dtype, "chunks", chunks, got)
            # ... and the model over the RGB targets read back: the test does not rest on the library alone
            dt, lt, ot = api._tensor_dtype(out.dtype), TM.PLANAR if layout == "chw" else TM.INTERLEAVED, api._tensor_order(order)
            for i in range(n):
                assert np.array_equal(bits_of(out[i]), TM.tensor(rgb[i], fmt, dt, lt, ot, SCALE, BIAS)), (route, "frame %d differs from the model" % i)
            assert not same_bytes(torch, out[0], out[1])
        # around the slice nothing was written
        keep = big.clone()
        keep[1:, :, 1:wh + 1, 2:ww + 2] = -2.0
        assert bool((keep == -2.0).all()), "a byte outside the slice's elements was written"
        vp.close()


def test_launch_counts_beside_process_batch_yuv(mpcvr, torch_cuda):
    """the same 8 frames through ProcessBatch, ProcessBatchYuv and ProcessBatchTensor on one context: one launch for the route, one more
    for either pass; one frame per chunk: a draw and a pass each.  ProcessBatchYuv counts what it counted."""
    from videorenderer_amd import api
    from tests.golden.cases import M709, MPEG2, TV, ext
    torch = torch_cuda
    vp, ww, wh = context(EVEN, False)
    n = 8
    frames = noise_frames(torch, EVEN, n)
    rgb = [torch.zeros((wh, ww, 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    ys = [torch.zeros((wh, ww + 2), dtype=torch.uint8, device="cuda") for _ in range(n)]
    uvs = [torch.zeros((wh // 2, ww + 2), dtype=torch.uint8, device="cuda") for _ in range(n)]
    out = torch.zeros((n, 3, wh, ww), dtype=torch.float16, device="cuda")
    desc = ext(MPEG2, TV, M709)
    for budget, chunks in ((0, 1), (api.plan_batch_tensor(ww, wh, n, 0)["frame_stride"], 8)):
        vp.SetBatchYuvBudget(budget)
        vp.ProcessBatch(frames, rgb, ww * 4)
        plain = vp.GetLastBatchInfo()
        assert plain["launches"] == 1 and "tensor_chunks" not in plain and "yuv_chunks" not in plain, plain
        vp.ProcessBatchYuv(frames, 1, desc, ys, ww + 2, uvs, ww + 2)
        yuv = vp.GetLastBatchInfo()
        vp.ProcessBatchTensor(frames, out)
        ten = vp.GetLastBatchInfo()
        vp.Synchronize()
        assert yuv["launches"] == 2 * chunks and yuv["yuv_chunks"] == chunks and "tensor_chunks" not in yuv, yuv
        assert ten["launches"] == 2 * chunks and ten["tensor_chunks"] == chunks and len(ten["tensor_lanes"]) == chunks and "yuv_chunks" not in ten, ten
        assert ten["uploads"] == yuv["uploads"], (ten, yuv)
    vp.close()


def test_two_calls_into_overlapping_tensors_stay_in_queue_order(mpcvr, torch_cuda):
    """A context that owns its stream deals chunks to the two batch lanes.  Call A writes frames 0 .. 3 of a buffer of five, call B frames
    1 .. 4 from other samples, without a synchronise in between: frame 0 is A's, frames 1 .. 4 are B's.  Several rounds, chunks of two, so
    that both lanes hold both calls' chunks."""
    from videorenderer_amd import api
    torch = torch_cuda
    c = ROUTES["FusedUp2x"][0]
    fmt = c.get("output_format", 0)
    vp, ww, wh = context(c, True)
    n = 4
    a, b = noise_frames(torch, c, n, seed0=1), noise_frames(torch, c, n, seed0=2)
    want_a, _, _ = composition(torch, vp, a, ww, wh, fmt, torch.float16, "chw", "rgb")
    want_b, _, _ = composition(torch, vp, b, ww, wh, fmt, torch.float16, "chw", "rgb")
    vp.SetBatchYuvBudget(2 * api.plan_batch_tensor(ww, wh, n, 0)["frame_stride"])
    buf = torch.zeros((n + 1, 3, wh, ww), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    lanes = set()
    for r in range(4):
        first, second, wf, ws = (a, b, want_a, want_b) if r & 1 == 0 else (b, a, want_b, want_a)
        vp.ProcessBatchTensor(first, buf[:n], SCALE, BIAS)
        lanes |= set(vp.GetLastBatchInfo()["tensor_lanes"])
        vp.ProcessBatchTensor(second, buf[1:], SCALE, BIAS)
        info = vp.GetLastBatchInfo()
        lanes |= set(info["tensor_lanes"])
        vp.Synchronize()
        assert same_bytes(torch, buf[0], wf[0]), "round %d: frame 0 is not the first call's" % r
        assert same_bytes(torch, buf[1:], ws), ("round %d: a chunk of the first call overtook the second call's" % r, info)
    assert lanes == ({-1} if LANES_OFF else {0, 1}), lanes
    vp.close()


def test_refusals_write_nothing(mpcvr, torch_cuda):
    import ctypes as C
    from videorenderer_amd import api
    torch = torch_cuda
    c = ROUTES["FusedUp2x"][0]
    vp, ww, wh = context(c, False)
    n = 3
    frames = noise_frames(torch, c, n)
    base = torch.full((n + 2, 3, wh, ww), -2.0, dtype=torch.float16, device="cuda")
    plane = wh * ww
    # overlapping frames within a batch: frame i + 1 starts at frame i's second plane
    lapped = base.as_strided((n, 3, wh, ww), (plane, plane, ww, 1))
    with pytest.raises(api.MpcvrError) as e:
        vp.ProcessBatchTensor(frames, lapped)
    assert e.value.args[0].startswith("HRESULT 0x80070057") and "overlap" in e.value.args[0]
    # one tensor given twice
    with pytest.raises(api.MpcvrError):
        vp.ProcessBatchTensor(frames, base[:1].expand(n, 3, wh, ww))
    # what Python refuses before any call
    for bad in (base[:n, :, :, ::2], base[:n - 1], base[:n, :2], base[:n].to(torch.float64), base[:n].permute(0, 2, 3, 1), base[:n].cpu(),
                base[:n, :, :wh - 1]):
        with pytest.raises(ValueError):
            vp.ProcessBatchTensor(frames, bad)
    with pytest.raises(ValueError):
        vp.ProcessBatchTensor(frames, base[:n], channel_order="grb")
    # what the C call refuses: NULLs, an empty batch, a scale outside the set
    L = vp._L
    arr = C.c_void_p * n
    srcs, dsts = arr(*[f.data_ptr() for f in frames]), arr(*[base[i].data_ptr() for i in range(n)])
    d = api.tensor_desc(TM.F16, TM.PLANAR, 2 * ww, 2 * plane, SCALE, BIAS)
    assert L.mpcvr_process_batch_tensor(vp._ctx, n, None, C.byref(d), dsts) == api.E_POINTER
    assert L.mpcvr_process_batch_tensor(vp._ctx, n, srcs, None, dsts) == api.E_POINTER
    assert L.mpcvr_process_batch_tensor(vp._ctx, n, srcs, C.byref(d), None) == api.E_POINTER
    assert L.mpcvr_process_batch_tensor(vp._ctx, n, srcs, C.byref(d), arr(dsts[0], None, dsts[2])) == api.E_POINTER
    assert L.mpcvr_process_batch_tensor(vp._ctx, 0, srcs, C.byref(d), dsts) == api.E_INVALIDARG
    assert L.mpcvr_process_batch_tensor(vp._ctx, n, srcs, C.byref(d), arr(dsts[0], dsts[1] + 1, dsts[2])) == api.E_INVALIDARG
    bad = api.tensor_desc(TM.F16, TM.PLANAR, 2 * ww, 2 * plane, (1.0, float("inf"), 1.0), BIAS)
    assert L.mpcvr_process_batch_tensor(vp._ctx, n, srcs, C.byref(bad), dsts) == api.E_INVALIDARG
    bare = api.VideoProcessor(api.default_settings())
    assert L.mpcvr_process_batch_tensor(bare._ctx, n, srcs, C.byref(d), dsts) == api.E_NOT_VALID_STATE
    bare.close()
    vp.Synchronize()
    torch.cuda.synchronize()
    assert bool((base == -2.0).all()), "a refused call wrote into the tensors"
    # ... and the arguments the refusals were derived from are accepted
    assert L.mpcvr_process_batch_tensor(vp._ctx, n, srcs, C.byref(d), dsts) == 0
    vp.Synchronize()
    want, _, _ = composition(torch, vp, frames, ww, wh, c.get("output_format", 0), torch.float16, "chw", "rgb")
    assert same_bytes(torch, base[:n], want) and bool((base[n:] == -2.0).all())
    vp.close()
