"""k_sharpen (extension: sharpening of rendered frames, include/mpcvr.h) on the GPU: every instantiation — source depth, target depth, mode
and radius are its template arguments — texel for texel against the numpy model (tests/sharpen_model.py) at the shapes where the kernel
takes another path: one texel, one row, one column, frames smaller than the radius-3 halo, the workgroup tile's extent - 1 / 0 / + 1 and
twice that + 1, widths that are no multiple of 4; every alignment of source and destination inside a patterned buffer whose every other
byte must survive, poisoned source padding, random A / X bits, rows more than 4 GiB apart, seeds, mpcvr_render_sharpen, and the refusals
that need a device pointer.  Everything is bits: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from tests import sharpen_model as SM
from tests.test_deband import PAIR_IDS, PAIRS, noise
from tests.test_deband_gpu import pattern
from tests.test_sharpen import K, MODES, RADII, gpu_params, gpu_surface, model, params

pytestmark = pytest.mark.gpu

BGRA8, RGB10A2 = SM.BGRA8, SM.RGB10A2
TW, TH = K["kSharpenTileCols"], K["kSharpenTileRows"]
# (w, h): one texel, one column, one row; 2 x 2 and 3 x 5, smaller than the radius-3 halo (every tap clamps); a frame inside one tile; the
# tile's extent - 1 / 0 / + 1 and twice that + 1 in each direction; widths that are no multiple of 4 (67, 70, 2 TW - 3)
SHAPES = [(1, 1), (1, 67), (67, 1), (2, 2), (3, 5), (70, 40), (TW - 1, TH + 1), (TW, TH), (TW + 1, TH - 1), (2 * TW + 1, 9), (9, 2 * TH + 1),
          (2 * TW + 1, 2 * TH + 1), (2 * TW - 3, 20)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def run_pass(torch, words, src_fmt, dst_fmt, P, seed, src_off=0, src_pitch=None, dst_off=0, dst_pitch=None, want=None, poison=None):
    """One mpcvr_sharpen_pass of `words` ((h, w) uint32) from a source src_off bytes behind a 256-byte boundary into a destination dst_off
    bytes behind one, each inside a patterned (source: or poisoned) buffer with a guard of one pitch + 4 KiB in front and behind.  Asserts
    the WHOLE destination buffer: the texels equal the model's, every other byte (pitch padding, guards) holds the pattern; the source is
    as it was.  Returns the texels."""
    from videorenderer_amd import api
    h, w = words.shape
    src_pitch, dst_pitch = src_pitch or 4 * w, dst_pitch or 4 * w
    sguard = (src_pitch + 4096 + 255) // 256 * 256
    n = sguard + src_off + h * src_pitch + sguard
    shost = SM.place(pattern(n) if poison is None else np.full(n, poison, dtype=np.uint8), sguard + src_off, words, src_pitch)
    src = torch.from_numpy(shost).cuda()
    guard = (dst_pitch + 4096 + 255) // 256 * 256
    before = pattern(guard + dst_off + h * dst_pitch + guard)
    buf, at = torch.from_numpy(before).cuda(), guard + dst_off
    assert src.data_ptr() % 256 == 0 and buf.data_ptr() % 256 == 0
    api.sharpen_pass(src.data_ptr() + sguard + src_off, src_pitch, src_fmt, w, h, P, seed, buf.data_ptr() + at, dst_pitch, dst_fmt)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    if want is None:
        want = model(words, src_fmt, dst_fmt, P, seed)
    full = SM.place(before.copy(), at, want, dst_pitch)
    if not np.array_equal(got, full):
        bad = np.nonzero(got != full)[0]
        off = int(bad[0]) - at
        raise AssertionError("%dx%d %s -> %s %r seed %d, source +%d pitch %d, destination +%d pitch %d: %d bytes differ, the first %d bytes from "
                             "the destination's first = row %d column %d (got %#x, want %#x, pattern %#x)"
                             % (w, h, "rgb10" if src_fmt else "bgra8", "rgb10" if dst_fmt else "bgra8", P, seed, src_off,
                                src_pitch, dst_off, dst_pitch, bad.size, off, off // dst_pitch, off % dst_pitch // 4, got[bad[0]], full[bad[0]], before[bad[0]]))
    assert src.cpu().numpy().tobytes() == shost.tobytes()
    return want


@pytest.mark.parametrize("mode", MODES, ids=["rgb", "luma"])
@pytest.mark.parametrize("radius", RADII, ids=["r1", "r2", "r3"])
@pytest.mark.parametrize("src_fmt,dst_fmt", PAIRS, ids=PAIR_IDS)
def test_every_instantiation_equals_the_model_texel_for_texel(mpcvr, torch_cuda, src_fmt, dst_fmt, radius, mode):
    """k_sharpen<IN10, OUT10, MODE, R> as the test's id names it, over every shape, tight source and destination, at parameters that take
    every branch on these surfaces (tests/test_sharpen.py: test_the_gpu_tests_surfaces_take_every_branch); the dither on for odd radii"""
    full = gpu_surface(src_fmt)
    P = gpu_params(radius, mode, radius & 1)
    for w, h in SHAPES:
        run_pass(torch_cuda, np.ascontiguousarray(full[:h, :w]), src_fmt, dst_fmt, P, 1000 + radius)


@pytest.mark.parametrize("src_fmt,dst_fmt", PAIRS, ids=PAIR_IDS)
def test_noise_and_the_extreme_parameters(mpcvr, torch_cuda, src_fmt, dst_fmt):
    """noise across two tiles in both directions: amount 256 with no coring and no overshoot, all the overshoot there is, amount 0, and a
    threshold that cores everything"""
    words = np.ascontiguousarray(noise(src_fmt, TH + 3, 2 * TW + 1, 50 + src_fmt))
    m = SM.MAXCODE[src_fmt]
    for r, mode, a, t, o, di in ((3, 0, 256, 0, 0, 1), (3, 1, 256, 0, m, 0), (1, 1, 0, 0, 0, 0), (2, 0, 256, 4 * m, 0, 1), (2, 1, 64, 5, 3, 1)):
        run_pass(torch_cuda, words, src_fmt, dst_fmt, params(r, a, t, o, mode, di), 77)


@pytest.mark.parametrize("mode", MODES, ids=["rgb", "luma"])
@pytest.mark.parametrize("src_fmt,dst_fmt", [(RGB10A2, BGRA8), (BGRA8, RGB10A2)], ids=["rgb10-to-bgra8", "bgra8-to-rgb10"])
def test_alignments_and_pitches_leave_every_other_byte_alone(mpcvr, torch_cuda, src_fmt, dst_fmt, mode):
    """Source and destination at +0 / +4 / +8 / +12 behind a 256-byte boundary with pitches that are and are not multiples of 16 (the
    16-byte loads and stores step aside independently): the same texels, and the pattern around them survives.  13 columns: three full
    lanes and a tail; TW + 3: a second tile of three columns."""
    full = gpu_surface(src_fmt)
    P = gpu_params(3 - mode, mode)
    for w, h in ((13, 3), (TW + 3, 6)):
        words = np.ascontiguousarray(full[:h, :w])
        want = model(words, src_fmt, dst_fmt, P, 9)
        up = (4 * w + 15) // 16 * 16
        for src_off in (0, 4, 8, 12):
            for src_pitch in (4 * w, up + 16, up + 4):
                for dst_off, dst_pitch in ((0, 4 * w), (0, up + 64), (4, up + 64), (8, up + 4), (12, up + 64)):
                    run_pass(torch_cuda, words, src_fmt, dst_fmt, P, 9, src_off=src_off, src_pitch=src_pitch, dst_off=dst_off, dst_pitch=dst_pitch, want=want)
        for dst_off in (4, 8, 12):
            for dst_pitch in (4 * w, up + 64, up + 4):
                run_pass(torch_cuda, words, src_fmt, dst_fmt, P, 9, dst_off=dst_off, dst_pitch=dst_pitch, want=want)


@pytest.fixture(autouse=True)
def _no_override(monkeypatch):
    monkeypatch.delenv("MPCVR_SHARPEN_STAGING", raising=False)


def test_the_staging_override_gives_identical_bytes(mpcvr, torch_cuda, monkeypatch):
    """MPCVR_SHARPEN_STAGING=dword, read per launch: a source that allows 16-byte loads staged with dword loads — the same bytes"""
    words = np.ascontiguousarray(gpu_surface(RGB10A2)[:TH + 3, :2 * TW + 1])
    for r, mode in ((1, 1), (3, 0)):
        P = gpu_params(r, mode)
        want = run_pass(torch_cuda, words, RGB10A2, BGRA8, P, 5, src_pitch=4 * (2 * TW + 4))
        monkeypatch.setenv("MPCVR_SHARPEN_STAGING", "dword")
        run_pass(torch_cuda, words, RGB10A2, BGRA8, P, 5, src_pitch=4 * (2 * TW + 4), want=want)
        monkeypatch.delenv("MPCVR_SHARPEN_STAGING")


def test_poisoned_source_padding_does_not_show(mpcvr, torch_cuda):
    """the bytes between the source's rows and around it, filled with two patterns: the same frame — a clamped tap reads the edge texel,
    never the padding.  A frame smaller than the halo, and one a tile and a tail wide"""
    for w, h in ((3, 5), (TW + 5, 7)):
        words = np.ascontiguousarray(noise(RGB10A2, 40, TW + 8, 5)[:h, :w])
        P = params(3, 256, 0, 1023, 0, 1)
        want = model(words, RGB10A2, BGRA8, P, 3)
        for poison in (0x00, 0xff):
            for off, pitch in ((0, (4 * w + 15) // 16 * 16 + 32), (4, 4 * w + 4)):
                run_pass(torch_cuda, words, RGB10A2, BGRA8, P, 3, src_off=off, src_pitch=pitch, want=want, poison=poison)


@pytest.mark.parametrize("src_fmt", (BGRA8, RGB10A2), ids=["bgra8", "rgb10"])
def test_source_alpha_bits_do_not_matter(mpcvr, torch_cuda, src_fmt):
    full = np.ascontiguousarray(gpu_surface(src_fmt)[:40, :70])
    keep = np.uint32(0x3fffffff if src_fmt else 0x00ffffff)
    rs = np.random.default_rng(8)
    for mode in MODES:
        P = gpu_params(2, mode)
        want = model(full & keep, src_fmt, 1 - src_fmt, P, 4)
        for _ in range(2):
            a = rs.integers(0, 2 ** 32, size=full.shape, dtype=np.uint64).astype(np.uint32) & ~keep
            run_pass(torch_cuda, (full & keep) | a, src_fmt, 1 - src_fmt, P, 4, want=want)


def test_seeds(mpcvr, torch_cuda):
    """two seeds give different dithered frames; the same seed gives the same bytes twice; 0 and 0xffffffff are seeds like any other"""
    words = np.ascontiguousarray(gpu_surface(RGB10A2)[:40, :70])
    P = gpu_params(2, 1)
    got = {s: run_pass(torch_cuda, words, RGB10A2, BGRA8, P, s) for s in (0, 1, 0xffffffff)}
    again = run_pass(torch_cuda, words, RGB10A2, BGRA8, P, 1)
    assert np.array_equal(again, got[1])
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[0xffffffff])


def test_rows_that_span_more_than_4_gib(mpcvr, torch_cuda):
    """an 8 x 5 picture whose rows lie 2^30 + 256 bytes apart in source and destination, so that the last row begins beyond 4 GiB: the
    texels are the model's, and 4 KiB either side of every destination row survive.  Only the rows are touched."""
    from videorenderer_amd import api
    torch = torch_cuda
    w, h, pitch, lead = 8, 5, (1 << 30) + 256, 4096
    span = (h - 1) * pitch + 4 * w
    assert span > 1 << 32
    words = np.ascontiguousarray(gpu_surface(RGB10A2)[:h, :w])
    src = torch.empty(lead + span + lead, dtype=torch.uint8, device="cuda")
    dst = torch.empty(lead + span + lead, dtype=torch.uint8, device="cuda")
    mark = pattern(lead + 4 * w + lead)
    for y in range(h):
        src[lead + y * pitch: lead + y * pitch + 4 * w] = torch.from_numpy(words[y].view(np.uint8).copy()).cuda()
        dst[y * pitch: y * pitch + mark.size] = torch.from_numpy(mark).cuda()
    for P, dst_fmt in ((gpu_params(3, 0), BGRA8), (gpu_params(2, 1), RGB10A2)):
        api.sharpen_pass(src.data_ptr() + lead, pitch, RGB10A2, w, h, P, 21, dst.data_ptr() + lead, pitch, dst_fmt, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        want = model(words, RGB10A2, dst_fmt, P, 21)
        for y in range(h):
            exp = mark.copy()
            exp[lead:lead + 4 * w] = want[y].view(np.uint8)
            assert np.array_equal(dst[y * pitch: y * pitch + mark.size].cpu().numpy(), exp), (P, y)
            assert np.array_equal(src[lead + y * pitch: lead + y * pitch + 4 * w].cpu().numpy(), words[y].view(np.uint8)), "the source changed"
    del src, dst
    torch.cuda.empty_cache()


@pytest.mark.parametrize("label", ["sdr_8bit", "hdr10_rgb10a2", "letterboxed_odd_window"])
def test_render_sharpen_equals_render_then_the_model_and_leaves_the_back_buffer(mpcvr, torch_cuda, label):
    from tests.test_measure_gpu import device_words
    from tests.test_tensor_gpu import RENDER_CASES, rendered
    from videorenderer_amd import api
    torch = torch_cuda
    c = RENDER_CASES[label]
    fmt = c.get("output_format", 0)
    vp, keep, ww, wh = rendered(mpcvr, torch, c)
    assert vp.Render(1) == 0
    vp.Synchronize()
    ptr, _, bw, bh = vp.GetBackBuffer()
    assert (bw, bh) == (ww, wh)
    frame = device_words(ptr, ww * wh).reshape(wh, ww).copy()       # what a plain Render leaves
    for P, seed, dst_fmt in ((gpu_params(2, 1), 5, 1 - fmt), (params(3, 256, 0, 4, 0, 0), 0xffffffff, fmt)):
        pitch = ww * 4 + 12
        before = pattern(wh * pitch + 512)
        buf = torch.from_numpy(before).cuda()
        assert vp.RenderSharpen(P, seed, dst_fmt, out=buf.data_ptr() + 256, out_pitch=pitch) is not None
        vp.Synchronize()
        assert np.array_equal(buf.cpu().numpy(), SM.place(before.copy(), 256, model(frame, fmt, dst_fmt, P, seed), pitch)), (label, P)
        ptr1, _, bw1, bh1 = vp.GetBackBuffer()
        assert (bw1, bh1) == (ww, wh) and np.array_equal(device_words(ptr1, ww * wh).reshape(wh, ww), frame), "the back buffer changed"
    # an allocated target with the defaults of the context's format
    out = vp.RenderSharpen(seed=3)
    vp.Synchronize()
    d = api.sharpen_params_default(fmt)
    assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(wh, ww),
                          SM.apply(frame, fmt, fmt, d.radius, d.amount, d.threshold, d.overshoot, d.mode, d.dither, 3))
    # refusals come before anything is drawn: the target over the back buffer, NULLs, a parameter, a format, a pitch
    L, E = vp._L, api.E_INVALIDARG
    ok = C.byref(api.SharpenParams(2, 32, 4, 2, 1, 1))
    keep_buf = buf.clone()
    t = C.c_void_p(buf.data_ptr() + 256)
    assert L.mpcvr_render_sharpen(vp._ctx, 1, ok, 0, C.c_void_p(vp.GetBackBuffer()[0] + 4 * ww), 4 * ww, 0) == E
    assert L.mpcvr_render_sharpen(vp._ctx, 1, C.byref(api.SharpenParams(4, 32, 4, 2, 1, 1)), 0, t, pitch, 0) == E
    assert L.mpcvr_render_sharpen(vp._ctx, 1, ok, 0, t, pitch, 2) == E
    assert L.mpcvr_render_sharpen(vp._ctx, 1, ok, 0, t, 4 * ww - 4, 0) == E
    assert L.mpcvr_render_sharpen(vp._ctx, 1, None, 0, t, pitch, 0) == api.E_POINTER
    assert L.mpcvr_render_sharpen(vp._ctx, 1, ok, 0, None, pitch, 0) == api.E_POINTER
    vp.Synchronize()
    assert torch.equal(buf, keep_buf)
    vp.close()


def test_render_sharpen_without_a_sample(mpcvr, torch_cuda):
    from videorenderer_amd import api
    torch = torch_cuda
    vp = api.VideoProcessor(api.default_settings())
    vp.InitMediaType(1, 96, 64)
    vp.SetWindowRect((0, 0, 96, 64))
    vp.SetVideoRect((0, 0, 96, 64))
    out = torch.full((64, 96, 4), 7, dtype=torch.uint8, device="cuda")
    assert vp.RenderSharpen(out=out) is None
    vp.Synchronize()
    assert bool((out == 7).all())
    vp.close()


def test_overlap_with_device_surfaces_is_refused_and_writes_nothing(mpcvr, torch_cuda):
    """the refusals that need a device pointer: a destination over the source in every way, with nothing written; the arguments they were
    derived from are accepted, a destination that begins where the source ends included"""
    from videorenderer_amd import api
    torch = torch_cuda
    L = api.load_library()
    w, h = 16, 8
    before = pattern(1 << 15)
    buf = torch.from_numpy(before).cuda()
    base = buf.data_ptr()
    s0, d0 = base + 4096, base + 8192
    P = (2, 200, 3, 1, 0, 0)

    def call(d=d0):
        return L.mpcvr_sharpen_pass(C.c_void_p(s0), w * 4, BGRA8, w, h, C.byref(api.SharpenParams(*P)), 6, C.c_void_p(d), w * 4, RGB10A2, None)

    for d in (s0, s0 + 4, s0 + 64, s0 - 7 * 64 - 60, s0 + 7 * 64 + 60):
        assert call(d) == api.E_INVALIDARG, d - s0
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), before), "a refused call wrote"
    assert call() == 0 and call(s0 + 8 * 64) == 0
    torch.cuda.synchronize()
    words = before[4096:4096 + 4 * w * h].view(np.uint32).reshape(h, w)
    m = model(words, BGRA8, RGB10A2, params(*P), 6)
    want = SM.place(SM.place(before.copy(), 8192, m, 4 * w), 4096 + 8 * 64, m, 4 * w)
    assert np.array_equal(buf.cpu().numpy(), want)
