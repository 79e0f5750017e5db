"""k_deint (extension: motion-adaptive deinterlacing at field rate, include/mpcvr.h: mpcvr_deint_pass) on the GPU: every instantiation word
for word against the numpy model (tests/deint_model.py) at the shapes where the kernel changes path, one whole sample per format family,
every alignment class of sources and destination and padded pitches with the padding poisoned two ways — always inside patterned buffers
whose every other byte must survive —, aliased sources, rows that span more than 4 GiB, the refusals, and mpcvr_copy_sample_fields against
mpcvr_deint_pass + mpcvr_copy_sample.  Everything is bits: no tolerance anywhere."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from tests import deint_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_POINTER, E_INVALIDARG, E_NOT_VALID_STATE = -2147467261, -2147024809, -2147019873      # 0x80004003, 0x80070057, 0x8007139F
NV12, P010, YV12, YUV422P10, YUV444P16, GBRP8, Y8, Y16, YUY2 = 1, 2, 14, 22, 25, 26, 37, 39, 4
# (bytes, cs) of the kernel and the format whose plane drives it: the gray formats for cs = 1 (any width), the bi-planar ones for cs = 2
# (their UV plane; the Y plane runs the cs = 1 instantiation beside it at twice the steps and lines)
DRIVERS = {(1, 1): Y8, (2, 1): Y16, (1, 2): NV12, (2, 2): P010}


def tile():
    """(steps of a wavefront, steps of a workgroup, rows of a strip, rows of a workgroup), the constants vp_deint.h exports"""
    text = open(os.path.join(ROOT, "videorenderer_amd", "csrc", "vp_deint.h")).read()
    v = {k: int(n) for k, n in re.findall(r"constexpr int (kDeint\w+) = (\d+);", text)}
    assert re.search(r"kDeintWaveCols = 64 \* kDeintLaneSteps;", text) and re.search(r"kDeintGroupCols = kDeintWaveCols;", text)
    assert re.search(r"kDeintGroupRows = kDeintWaves \* kDeintStripRows;", text)
    wave = 64 * v["kDeintLaneSteps"]
    return wave, wave, v["kDeintStripRows"], v["kDeintWaves"] * v["kDeintStripRows"]


WAVE_COLS, GROUP_COLS, STRIP_ROWS, GROUP_ROWS = tile()
WIDTHS = sorted({1, 2, 3, 4, 5, 7, 8, WAVE_COLS - 1, WAVE_COLS, WAVE_COLS + 1, GROUP_COLS + 1})      # in channel steps
LINES = sorted({2, 3, 5, 6, STRIP_ROWS + 1, 2 * STRIP_ROWS + 1})


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(autouse=True)
def side_stream(torch_cuda):
    """the tests run on a stream torch made: a context on torch's stream is a context on a caller's stream (tests/test_tensor_in_gpu.py)"""
    with torch_cuda.cuda.stream(torch_cuda.cuda.Stream()):
        yield


def pattern(n):
    return ((np.arange(n, dtype=np.int64) * 131 + 17) & 255).astype(np.uint8)


def run_pass(torch, cformat, w, h, keep, first, mode, seed=1, pitch=0, dst_pitch=0, src_off=(0, 0, 0), dst_off=0, poison=0xee, alias=None):
    """One mpcvr_deint_pass over three noise samples that start src_off[i] bytes behind 256-byte boundaries of ONE allocation, into a sample
    dst_off bytes behind one inside a patterned buffer with a guard in front and behind.  alias: 'prev' makes prev the very sample cur is.
    Asserts the WHOLE destination buffer — the pixels are the model's, every other byte holds the pattern — and that the sources are unchanged."""
    from videorenderer_amd import api
    sp = api.plan_deint_planes(cformat, w, h, pitch)
    dp = api.plan_deint_planes(cformat, w, h, dst_pitch)
    samples = M.noise_samples(sp, 3, seed, poison)
    size = M.sample_size(sp)
    slot = (size + 64 + 255) // 256 * 256
    host = np.full(3 * slot, poison, dtype=np.uint8)
    at = [i * slot + src_off[i] for i in range(3)]
    if alias == "prev":
        at[0], samples[0] = at[1], samples[1]
    for a, s in zip(at, samples):
        host[a:a + size] = s
    src = torch.from_numpy(host).cuda()
    dsize = M.sample_size(dp)
    guard = 4096
    before = pattern(guard + dst_off + dsize + guard)
    buf = torch.from_numpy(before).cuda()
    assert src.data_ptr() % 256 == 0 and buf.data_ptr() % 256 == 0
    api.deint_pass(src.data_ptr() + at[0], src.data_ptr() + at[1], src.data_ptr() + at[2], cformat, w, h, pitch, keep, first, mode,
                   buf.data_ptr() + guard + dst_off, dst_pitch, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    want = before.copy()
    M.deint_sample(sp, samples[0], samples[1], samples[2], keep, first, mode, want[guard + dst_off:], dp)
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError("format %d %dx%d keep %d first %d mode %d, pitch %d -> %d, sources +%s, destination +%d: %d bytes differ, the first %d bytes "
                             "from the sample's first (got %#x, want %#x, pattern %#x)" % (cformat, w, h, keep, first, mode, sp[0]["pitch"], dp[0]["pitch"], src_off,
                                                                                         dst_off, bad.size, int(bad[0]) - guard - dst_off, got[bad[0]],
                                                                                         want[bad[0]], before[bad[0]]))
    assert src.cpu().numpy().tobytes() == host.tobytes()


@pytest.mark.parametrize("mode", [0, 1], ids=["check", "nocheck"])
@pytest.mark.parametrize("nbytes,cs", sorted(DRIVERS), ids=["%dB-cs%d" % k for k in sorted(DRIVERS)])
def test_every_instantiation_at_the_shapes_where_the_kernel_changes_path(torch_cuda, nbytes, cs, mode):
    cformat = DRIVERS[(nbytes, cs)]
    parity = itertools.cycle(itertools.product((0, 1), (0, 1)))
    for steps, lines in itertools.product(WIDTHS, LINES):
        keep, first = next(parity)
        w, h = (steps, lines) if cs == 1 else (2 * steps, 2 * lines)
        run_pass(torch_cuda, cformat, w, h, keep, first, mode, seed=steps * 100 + lines)
    for keep, first in itertools.product((0, 1), (0, 1)):      # every parity at the shape that takes every path at once
        w, h = (GROUP_COLS + 1, 2 * STRIP_ROWS + 1) if cs == 1 else (2 * GROUP_COLS + 2, 4 * STRIP_ROWS + 2)
        run_pass(torch_cuda, cformat, w, h, keep, first, mode, seed=5)


@pytest.mark.parametrize("cformat,w,h", [(NV12, 70, 36), (P010, 70, 36), (YV12, 70, 36), (YUV422P10, 70, 19), (YUV444P16, 67, 19), (GBRP8, 67, 19), (Y16, 67, 19)],
                         ids=["nv12", "p010", "yv12", "yuv422p10", "yuv444p16", "gbrp8", "y16"])
def test_a_whole_sample_per_format_family(torch_cuda, cformat, w, h):
    for keep, first, mode in ((0, 1, 0), (1, 0, 0), (1, 1, 1), (0, 0, 1)):
        run_pass(torch_cuda, cformat, w, h, keep, first, mode, seed=cformat)


@pytest.mark.parametrize("nbytes,cs", sorted(DRIVERS), ids=["%dB-cs%d" % k for k in sorted(DRIVERS)])
def test_every_alignment_class_and_padded_pitches_poisoned_two_ways(torch_cuda, nbytes, cs):
    """the vector paths ask for sources / destination and pitch on 4 cs bytes: every residue of the component size up to that, for the
    sources (one of the three off the grid is enough to leave the path) and for the destination, and pitches on and off the grid"""
    cformat = DRIVERS[(nbytes, cs)]
    grid = 4 * cs * nbytes
    w, h = (37, 7) if cs == 1 else (74, 14)
    row = w * nbytes
    offs = list(range(0, grid + 1, nbytes))
    for i, off in enumerate(offs):
        mode, (keep, first) = i & 1, ((0, 1), (1, 0), (1, 1), (0, 0))[i % 4]
        run_pass(torch_cuda, cformat, w, h, keep, first, mode, seed=off, src_off=(off, off, off), dst_off=0)
        run_pass(torch_cuda, cformat, w, h, keep, first, mode, seed=off, src_off=(0, 0, off), dst_off=0)
        run_pass(torch_cuda, cformat, w, h, keep, first, mode, seed=off, src_off=(0, 0, 0), dst_off=off)
    for pad in (nbytes, 4, grid, 2 * grid, 64 - row % 64):
        for poison in (0x00, 0xff):
            run_pass(torch_cuda, cformat, w, h, 0, 1, 0, seed=pad, pitch=row + pad, dst_pitch=row, poison=poison)
            run_pass(torch_cuda, cformat, w, h, 1, 0, 1, seed=pad, pitch=row + pad, dst_pitch=row + pad, poison=poison)
            run_pass(torch_cuda, cformat, w, h, 1, 1, 0, seed=pad, pitch=row, dst_pitch=row + pad, poison=poison)


def test_sources_as_views_of_one_allocation_and_prev_equal_to_cur(torch_cuda):
    for cformat, w, h in ((NV12, 70, 36), (Y16, 67, 19)):
        for keep, first, mode in itertools.product((0, 1), (0, 1), (0, 1)):
            run_pass(torch_cuda, cformat, w, h, keep, first, mode, seed=9, alias="prev")


def test_rows_that_span_more_than_4_gib(torch_cuda):
    """one Y8 frame of 64 x 6 whose rows lie 2^30 + 256 bytes apart: the sources are views of one allocation at small offsets, the destination
    lives in a second one.  The pixels are the model's, and the bytes in front of and behind every destination row survive"""
    from videorenderer_amd import api
    torch = torch_cuda
    w, h, pitch = 64, 6, (1 << 30) + 256
    span = (h - 1) * pitch + w
    assert span > 1 << 32
    f = M.noise(h, w, 1, 4242)
    src = torch.empty(span + 256, dtype=torch.uint8, device="cuda")
    dst = torch.empty(span + 256, dtype=torch.uint8, device="cuda")
    offs = (0, 64, 128)
    mark = torch.from_numpy(pattern(w + 128)).cuda()
    for y in range(h):
        for k in range(3):
            src[y * pitch + offs[k]: y * pitch + offs[k] + w] = torch.from_numpy(np.ascontiguousarray(f[k][y])).cuda()
        dst[y * pitch: y * pitch + w + 128] = mark
    base = 64                                                   # the destination sample starts 64 bytes into the marked stretch of every row
    for keep, first, mode in ((0, 1, 0), (1, 0, 1)):
        api.deint_pass(src.data_ptr() + offs[0], src.data_ptr() + offs[1], src.data_ptr() + offs[2], Y8, w, h, pitch, keep, first, mode,
                       dst.data_ptr() + base, pitch, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        want = M.deint_plane(f[0], f[1], f[2], keep, first, mode, 1, 255).astype(np.uint8)
        for y in range(h):
            got = dst[y * pitch: y * pitch + w + 128].cpu().numpy()
            exp = pattern(w + 128)
            exp[base:base + w] = want[y]
            assert np.array_equal(got, exp), (keep, first, mode, y)
    del src, dst
    torch.cuda.empty_cache()


def test_refusals_leave_the_destination_untouched(torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    w, h = 64, 48
    size = w * h * 3 // 2
    s = [torch.from_numpy(x).cuda() for x in M.noise_samples(api.plan_deint_planes(NV12, w, h), 3, 3)]
    before = pattern(4 * size)
    d = torch.from_numpy(before).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(prev=s[0].data_ptr(), cur=s[1].data_ptr(), nxt=s[2].data_ptr(), cf=NV12, w=w, h=h, pitch=0, keep=0, first=1, mode=0, dst=d.data_ptr() + 256, dp=0):
        return L.mpcvr_deint_pass(C.c_void_p(prev), C.c_void_p(cur), C.c_void_p(nxt), cf, w, h, pitch, keep, first, mode, C.c_void_p(dst), dp, stream)
    cases = [(E_POINTER, dict(prev=None)), (E_POINTER, dict(cur=None)), (E_POINTER, dict(nxt=None)), (E_POINTER, dict(dst=None)),
             (E_INVALIDARG, dict(cf=YUY2)), (E_INVALIDARG, dict(cf=0)), (E_INVALIDARG, dict(cf=30)),
             (E_INVALIDARG, dict(keep=2)), (E_INVALIDARG, dict(keep=-1)), (E_INVALIDARG, dict(first=2)), (E_INVALIDARG, dict(mode=2)), (E_INVALIDARG, dict(mode=-1)),
             (E_INVALIDARG, dict(w=63)), (E_INVALIDARG, dict(h=2)), (E_INVALIDARG, dict(h=47)), (E_INVALIDARG, dict(w=0)), (E_INVALIDARG, dict(w=16386)),
             (E_INVALIDARG, dict(pitch=63)), (E_INVALIDARG, dict(dp=63)), (E_INVALIDARG, dict(pitch=-64)),
             (E_INVALIDARG, dict(cf=P010, w=16, h=16, pitch=33)), (E_INVALIDARG, dict(cf=P010, w=16, h=16, dst=d.data_ptr() + 257)),
             (E_INVALIDARG, dict(cf=P010, w=16, h=16, prev=s[0].data_ptr() + 1)),
             # a destination plane over a source plane: the very sample, its last byte, its UV plane from below; and destination planes over each other
             (E_INVALIDARG, dict(dst=s[1].data_ptr())), (E_INVALIDARG, dict(dst=s[2].data_ptr() + size - 1)), (E_INVALIDARG, dict(dst=s[0].data_ptr() - size + 1)),
             (E_INVALIDARG, dict(cur=d.data_ptr() + 256 + size - 1)), (E_INVALIDARG, dict(nxt=d.data_ptr() + 256 - size + 1))]
    for hr, kw in cases:
        assert call(**kw) == hr, kw
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), before), "a refused pass wrote"
    for i in range(3):
        assert s[i].numel() == size
    # what merely touches is taken: the destination directly behind a source
    both = torch.from_numpy(pattern(2 * size)).cuda()
    assert L.mpcvr_deint_pass(C.c_void_p(both.data_ptr()), C.c_void_p(both.data_ptr()), C.c_void_p(both.data_ptr()), NV12, w, h, 0, 0, 1, 0,
                              C.c_void_p(both.data_ptr() + size), 0, stream) == 0
    torch.cuda.synchronize()


def _context(api, torch, cformat, w, h, out=None):
    vp = api.VideoProcessor(api.default_settings(), device=0)
    vp.InitMediaType(cformat, w, h)
    ow, oh = out or (w, h)
    vp.SetWindowRect((0, 0, ow, oh))
    vp.SetVideoRect((0, 0, ow, oh))
    return vp


@pytest.mark.parametrize("cformat", [NV12, P010, YV12], ids=["nv12", "p010", "yv12"])
def test_copy_sample_fields_is_the_pass_then_copy_sample(torch_cuda, cformat):
    from videorenderer_amd import api
    torch = torch_cuda
    w, h = 64, 48
    planes = api.plan_deint_planes(cformat, w, h)
    s = [torch.from_numpy(x).cuda() for x in M.noise_samples(planes, 3, 50 + cformat)]
    size = M.sample_size(planes)
    vp = _context(api, torch, cformat, w, h, (96, 72))
    assert vp.GetFrameBytes() == (size, planes[0]["pitch"])
    ref = _context(api, torch, cformat, w, h, (96, 72))
    stream = torch.cuda.current_stream().cuda_stream
    last = None
    for order, field, mode in itertools.product((1, 2), (0, 1), (0, 1)):
        got = torch.zeros((72, 96, 4), dtype=torch.uint8, device="cuda")
        want = torch.zeros((72, 96, 4), dtype=torch.uint8, device="cuda")
        vp.CopySampleFields(s[0], s[1], s[2], order, field, mode)
        vp.Process(got, 96 * 4)
        keep, first = M.field_parity(order, field)
        tmp = torch.zeros(size, dtype=torch.uint8, device="cuda")
        api.deint_pass(s[0], s[1], s[2], cformat, w, h, 0, keep, first, mode, tmp, 0, stream)
        ref.CopySample(tmp, mem_kind=api.MEM_DEVICE)
        ref.Process(want, 96 * 4)
        vp.Synchronize(); ref.Synchronize()
        assert torch.equal(got, want), (order, field, mode)
        assert int(got.max()) > 0
        last = want
    # a refused call: nothing is touched, the previous sample stays current
    L = api.load_library()
    p = [C.c_void_p(x.data_ptr()) for x in s]
    for hr, args in ((E_INVALIDARG, (p[0], p[1], p[2], 0, 0, 0)), (E_INVALIDARG, (p[0], p[1], p[2], 3, 0, 0)), (E_INVALIDARG, (p[0], p[1], p[2], 1, 2, 0)),
                     (E_INVALIDARG, (p[0], p[1], p[2], 1, 0, 2)), (E_POINTER, (None, p[1], p[2], 1, 0, 0)), (E_POINTER, (p[0], p[1], None, 1, 0, 0))):
        assert L.mpcvr_copy_sample_fields(vp._ctx, *args) == hr, args
    again = torch.zeros((72, 96, 4), dtype=torch.uint8, device="cuda")
    vp.Process(again, 96 * 4)
    vp.Synchronize()
    assert torch.equal(again, last), "the previous sample did not survive a refused call"
    vp.close(); ref.close()


def test_copy_sample_fields_refuses_a_packed_input_and_a_context_without_input(torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    x = torch.zeros(64 * 48 * 2, dtype=torch.uint8, device="cuda")
    p = C.c_void_p(x.data_ptr())
    vp = api.VideoProcessor(api.default_settings(), device=0)
    assert L.mpcvr_copy_sample_fields(vp._ctx, p, p, p, 1, 0, 0) == E_NOT_VALID_STATE
    vp.InitMediaType(YUY2, 64, 48)
    assert L.mpcvr_copy_sample_fields(vp._ctx, p, p, p, 1, 0, 0) == E_INVALIDARG
    vp.close()
